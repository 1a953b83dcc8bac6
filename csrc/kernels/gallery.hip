// K27 (appearance search): a crop's feature map becomes an int8 embedding, the embedding is
// scored against a gallery of enrolled embeddings and the best few rows per crop are kept, all
// inside the captured step.  Integer arithmetic throughout: every output equals
// ops.reference.embed_quantize / ops.reference.gallery_match bit for bit.
//
// (a) embed_quantize: features bf16 [M, HW, C] -> codes int8 [M, C], nrm2 int32 [M].
//   f = rintf(clamp(NaN -> 0, -16384, 16384) * 256) (an integer, |f| <= 2^22), s[c] = sum over
//   the HW positions (int32, |s| <= 2^30, exact in any order), mx = max |s|,
//   e = max(0, bitlen(mx) - 7), code = sign(s) min(127, (|s| + (e ? 1 << (e - 1) : 0)) >> e),
//   nrm2 = sum code^2.  ONE WORKGROUP OF 256 PER ROW.  A thread reads 16 bytes (8 channels) of
//   one position at a time; where C / 8 < 256 the spare threads split the positions.  The
//   per-channel sums meet in LDS (int atomics: exact, order-free), the maximum and nrm2 go
//   through wave shuffles and one LDS word per wave, the codes leave as packed dwords.
//
// (b) gallery_match: q int8 [M, D], gallery codes int8 [cap, D], scale fp32 [cap], count int32
//   [1] in device memory.  Row j counts if j < min(count, cap) and scale[j] > 0;
//   score = (float)dot_i32(q, g_j) * scale[j]; kept: the K best under (score descending, row
//   ascending), a total order.
//   Split: a workgroup of 4 waves takes a GALLERY BLOCK of 128 rows (32 per wave) against a
//   QUERY TILE of up to 256 queries (NT column tiles of 32; grid.y walks further query blocks,
//   so with M <= 256 the gallery streams from memory exactly once).  Workgroups are persistent:
//   workgroup x walks the blocks x, x + grid.x, ... below min(count, cap); blocks past it are
//   never read.
//   K loop: D in chunks of 64 bytes.  Gallery operands go global -> registers directly: lane
//   (i = lane % 32, h = lane / 32) reads the 32 bytes [64 c + 32 h, +32) of its row, so two
//   lanes consume a row's 64 bytes and each gallery byte is read once.  Queries go through a
//   double-buffered LDS stage (thread t stages query t's 64 bytes, rows padded to 80 bytes),
//   read back in the same (column, h) shape.  Two v_mfma_i32_32x32x32_i8 per chunk and column
//   tile: the s-th uses the s-th 16 bytes of both sides.  That is a permutation of k applied
//   to both operands alike, which a dot product does not see.  Next chunk's global loads are
//   issued before the current chunk's MFMAs; one barrier per chunk.
//   Accumulators: acc[t][r] of lane (j, h) is query 32 t + j against gallery row
//   8 (r / 4) + 4 h + r % 4 of the wave's 32: a lane's accumulators all belong to one query per
//   column tile, so selection starts in-lane.
//   Selection: every wave keeps a sorted list [256][K] of (score, row) in LDS.  A lane compares
//   its 16 candidates per column tile against the list's last entry and inserts the few that
//   beat it; the two half-waves that share a query take turns (wave-level ordering only, no
//   workgroup barrier).  After the walk thread q merges the four wave lists of query q and
//   writes the workgroup's partial list part[q][x][K]: no atomics.
//
// (c) gallery_merge: one wavefront per query, K rounds over its grid.x K partial entries: the
//   best entry strictly after the previous pick, by wave shuffles.  Rows are distinct, so the
//   result does not depend on how blocks fell to workgroups.  Empty slots: score 0, row -1.
#include "common.h"
#include "kvedge_kernels.h"
#include "resample.h"  // rs_in_alloc

namespace kvedge {
namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int kGlThreads = 256, kGlWaves = kGlThreads / kWave;
constexpr int kGlBlock = 128;      // gallery rows per block (32 per wave)
constexpr int kGlQTile = 256;      // queries per workgroup
constexpr int kGlChunk = 64;       // bytes of D per step
constexpr int kGlQStride = 80;     // LDS bytes per staged query row (64 + 16: spreads the banks)
constexpr int kGlMaxTop = 8, kGlMaxDim = 4096, kGlMaxCap = 1 << 20, kGlMaxM = 65535;
constexpr int kGlNoRow = 0x7fffffff;  // an empty list slot: (-inf, kGlNoRow), worse than any row

struct Cand {
  float s;
  int r;
};
// the total order: score descending, then row ascending
__device__ __forceinline__ bool better(float s, int r, float ts, int tr) {
  return s > ts || (s == ts && r < tr);
}

// ------------------------------------------------------------------------------------------
// (a) embed_quantize
// ------------------------------------------------------------------------------------------
constexpr int kEqThreads = 256, kEqWaves = kEqThreads / kWave;

__device__ __forceinline__ int eq_fixed(unsigned short bits) {
  float v = __uint_as_float((unsigned)bits << 16);
  v = (v != v) ? 0.f : v;
  v = v < -16384.f ? -16384.f : (v > 16384.f ? 16384.f : v);
  return (int)rintf(v * 256.0f);
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(kEqThreads) void embed_quantize_kernel(
    const unsigned short* __restrict__ x, signed char* __restrict__ codes, int* __restrict__ nrm2,
    int HW, int C) {
  __shared__ int sum[kGlMaxDim];
  __shared__ int red[2 * kEqWaves];
  const int tid = threadIdx.x, m = blockIdx.x;
  const int G = C >> 3;  // 16-byte groups of 8 channels: 8..512
  for (int c = tid; c < C; c += kEqThreads) sum[c] = 0;
  __syncthreads();
  // G >= 256: thread owns groups tid, tid + 256 over every position; else P = 256 / G threads
  // share a group and split the positions
  const int P = G >= kEqThreads ? 1 : kEqThreads / G;
  const int g0 = G >= kEqThreads ? tid : tid % G;
  const int p0 = G >= kEqThreads ? 0 : tid / G;
  const unsigned short* xr = x + (long long)m * HW * C;
  if (p0 < P) {
    for (int g = g0; g < G; g += kEqThreads) {
      int acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int p = p0; p < HW; p += P) {
        const uint4 v = *reinterpret_cast<const uint4*>(xr + (long long)p * C + g * 8);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          acc[2 * k] += eq_fixed((unsigned short)(w[k] & 0xffffu));
          acc[2 * k + 1] += eq_fixed((unsigned short)(w[k] >> 16));
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (P == 1) sum[g * 8 + k] = acc[k];
        else atomicAdd(&sum[g * 8 + k], acc[k]);
      }
    }
  }
  __syncthreads();
  int mx = 0;
  for (int c = tid; c < C; c += kEqThreads) mx = max(mx, abs(sum[c]));
  mx = wave_max(mx);
  if ((tid & (kWave - 1)) == 0) red[tid / kWave] = mx;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int w = 1; w < kEqWaves; ++w) mx = max(mx, red[w]);
  const int bl = mx ? 32 - __clz(mx) : 0;
  const int e = max(0, bl - 7);
  const int rnd = e ? 1 << (e - 1) : 0;
  int n2 = 0;
  unsigned* out = reinterpret_cast<unsigned*>(codes + (long long)m * C);
  for (int d = tid; d < (C >> 2); d += kEqThreads) {
    unsigned pk = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int s = sum[d * 4 + k];
      const int a = min(127, (abs(s) + rnd) >> e);
      const int c = s < 0 ? -a : a;
      n2 += c * c;
      pk |= (unsigned)(c & 0xff) << (8 * k);
    }
    out[d] = pk;
  }
  n2 = wave_sum(n2);
  if ((tid & (kWave - 1)) == 0) red[kEqWaves + tid / kWave] = n2;
  __syncthreads();
  if (tid == 0) {
    int t = 0;
#pragma unroll
    for (int w = 0; w < kEqWaves; ++w) t += red[kEqWaves + w];
    nrm2[m] = t;
  }
}

// ------------------------------------------------------------------------------------------
// (b) gallery_match
// ------------------------------------------------------------------------------------------
// LDS: query stage 2 x 256 x 80 bytes | wave lists 4 x 256 x K x 8 bytes
constexpr int kGlStageBytes = 2 * kGlQTile * kGlQStride;
__host__ __device__ constexpr int gl_lds_bytes(int K) {
  return kGlStageBytes + kGlWaves * kGlQTile * K * 8;
}

// insert (s, r) into the sorted list l[0..K) if it beats the last entry
__device__ __forceinline__ void list_insert(Cand* l, int K, float s, int r) {
  if (!better(s, r, l[K - 1].s, l[K - 1].r)) return;
  int k = K - 1;
  while (k > 0 && better(s, r, l[k - 1].s, l[k - 1].r)) {
    l[k] = l[k - 1];
    --k;
  }
  l[k].s = s;
  l[k].r = r;
}

template <int NT>
__global__ __launch_bounds__(kGlThreads) void gallery_match_kernel(
    const signed char* __restrict__ q, const signed char* __restrict__ g,
    const float* __restrict__ scale, const int* __restrict__ count, Cand* __restrict__ part,
    int M, int D, int cap, int K) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  unsigned char* stage = lds;
  Cand* lists = reinterpret_cast<Cand*>(lds + kGlStageBytes);

  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int j = lane & 31, h = lane >> 5;
  const int q0 = blockIdx.y * kGlQTile;  // first query of this workgroup's tile
  const int nwg = gridDim.x;
  const int n = min(max(*count, 0), cap);
  const int nch = D / kGlChunk;

  Cand* mine = lists + (long long)wave * kGlQTile * K;  // this wave's lists [256][K]
  for (int i = tid; i < kGlWaves * kGlQTile * K; i += kGlThreads) {
    lists[i].s = -INFINITY;
    lists[i].r = kGlNoRow;
  }
  __syncthreads();

  // the query this thread stages (threads past the tile's queries stage nothing)
  const bool stager = tid < NT * 32;
  const bool q_ok = stager && q0 + tid < M;
  const signed char* qrow = q + (long long)(q_ok ? q0 + tid : 0) * D;

  for (int blk = blockIdx.x; (long long)blk * kGlBlock < n; blk += nwg) {
    const int row0 = blk * kGlBlock + wave * 32;
    // rows past cap are never read: the lane re-reads the last row, masked out below
    const int arow = min(row0 + j, cap - 1);
    const signed char* ap = g + (long long)arow * D + h * 32;

    i32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0;

    // prologue: chunk 0 of the queries into stage 0, chunk 0 of the gallery into registers
    i32x4 qn[4], a_cur[2], a_nxt[2];
    if (stager) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        qn[s] = q_ok ? *reinterpret_cast<const i32x4*>(qrow + s * 16) : i32x4{0, 0, 0, 0};
        *reinterpret_cast<i32x4*>(stage + tid * kGlQStride + s * 16) = qn[s];
      }
    }
    a_cur[0] = *reinterpret_cast<const i32x4*>(ap);
    a_cur[1] = *reinterpret_cast<const i32x4*>(ap + 16);
    __syncthreads();

    for (int c = 0; c < nch; ++c) {
      const bool more = c + 1 < nch;
      if (more) {
        if (stager) {
#pragma unroll
          for (int s = 0; s < 4; ++s)
            qn[s] = q_ok ? *reinterpret_cast<const i32x4*>(qrow + (c + 1) * kGlChunk + s * 16)
                         : i32x4{0, 0, 0, 0};
        }
        a_nxt[0] = *reinterpret_cast<const i32x4*>(ap + (c + 1) * kGlChunk);
        a_nxt[1] = *reinterpret_cast<const i32x4*>(ap + (c + 1) * kGlChunk + 16);
      }
      const unsigned char* sb = stage + (c & 1) * (kGlQTile * kGlQStride) + h * 32;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const i32x4 b0 = *reinterpret_cast<const i32x4*>(sb + (t * 32 + j) * kGlQStride);
        const i32x4 b1 = *reinterpret_cast<const i32x4*>(sb + (t * 32 + j) * kGlQStride + 16);
        acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a_cur[0], b0, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a_cur[1], b1, acc[t], 0, 0, 0);
      }
      if (more) {
        if (stager) {
          unsigned char* db = stage + ((c + 1) & 1) * (kGlQTile * kGlQStride) + tid * kGlQStride;
#pragma unroll
          for (int s = 0; s < 4; ++s) *reinterpret_cast<i32x4*>(db + s * 16) = qn[s];
        }
        a_cur[0] = a_nxt[0];
        a_cur[1] = a_nxt[1];
      }
      __syncthreads();
    }

    // epilogue: the lane's 16 gallery rows and their scales (0 = the row does not count)
    float sc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = row0 + 8 * (r >> 2) + 4 * h + (r & 3);
      const float v = row < n ? scale[row] : 0.f;
      sc[r] = v > 0.f ? v : 0.f;
    }
    // the half-waves share queries: h = 0 inserts first, then h = 1 (same wave: LDS keeps the
    // order of the wave's own instructions)
#pragma unroll
    for (int turn = 0; turn < 2; ++turn) {
      if (h == turn) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          Cand* l = mine + (t * 32 + j) * K;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (sc[r] > 0.f)
              list_insert(l, K, (float)acc[t][r] * sc[r], row0 + 8 * (r >> 2) + 4 * h + (r & 3));
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    // the next block's prologue overwrites stage 0: every wave is past its last read of it
    // (the K loop's closing barrier), and the lists are per wave
  }
  __syncthreads();

  // thread qi merges the four wave lists of query q0 + qi into the workgroup's partial list
  if (tid < NT * 32 && q0 + tid < M) {
    int pos[kGlWaves] = {0, 0, 0, 0};
    Cand* out = part + ((long long)(q0 + tid) * nwg + blockIdx.x) * K;
    for (int k = 0; k < K; ++k) {
      float bs = -INFINITY;
      int br = kGlNoRow, bw = 0;
#pragma unroll
      for (int w = 0; w < kGlWaves; ++w) {
        if (pos[w] < K) {
          const Cand c = lists[((long long)w * kGlQTile + tid) * K + pos[w]];
          if (better(c.s, c.r, bs, br)) {
            bs = c.s;
            br = c.r;
            bw = w;
          }
        }
      }
#pragma unroll
      for (int w = 0; w < kGlWaves; ++w) pos[w] += (w == bw && br != kGlNoRow) ? 1 : 0;
      out[k].s = bs;
      out[k].r = br;
    }
  }
}

// ------------------------------------------------------------------------------------------
// (c) gallery_merge: block = one wavefront = one query
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kWave) void gallery_merge_kernel(const Cand* __restrict__ part,
                                                              float* __restrict__ score,
                                                              int* __restrict__ row, int nwg,
                                                              int K) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const Cand* p = part + (long long)m * nwg * K;
  const int total = nwg * K;
  float ls = INFINITY;  // the previous pick; the first round accepts everything
  int lr = -1;
  for (int k = 0; k < K; ++k) {
    float bs = -INFINITY;
    int br = kGlNoRow;
    for (int i = lane; i < total; i += kWave) {
      const Cand c = p[i];
      if (c.r != kGlNoRow && better(ls, lr, c.s, c.r) && better(c.s, c.r, bs, br)) {
        bs = c.s;
        br = c.r;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float os = __shfl_xor(bs, o);
      const int orow = __shfl_xor(br, o);
      if (better(os, orow, bs, br)) {
        bs = os;
        br = orow;
      }
    }
    const bool found = br != kGlNoRow;
    if (lane == 0) {
      score[(long long)m * K + k] = found ? bs : 0.f;
      row[(long long)m * K + k] = found ? br : -1;
    }
    if (!found) {  // nothing left: the remaining slots are empty too (uniform across the wave)
      for (int k2 = k + 1 + lane; k2 < K; k2 += kWave) {
        score[(long long)m * K + k2] = 0.f;
        row[(long long)m * K + k2] = -1;
      }
      break;
    }
    ls = bs;
    lr = br;
  }
}

int gl_workgroups(int cap) {
  static int cus = 0;
  if (cus == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        v < 1)
      v = 256;
    cus = v;
  }
  const int blocks = (cap + kGlBlock - 1) / kGlBlock;
  return blocks < cus ? blocks : cus;
}

template <int NT>
int gl_launch(const signed char* q, const signed char* g, const float* scale, const int* count,
              Cand* part, int M, int D, int cap, int K, int nwg, hipStream_t s) {
  const int lds = gl_lds_bytes(K);
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(gallery_match_kernel<NT>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
    return -100;
  const dim3 grid((unsigned)nwg, (unsigned)((M + kGlQTile - 1) / kGlQTile));
  hipLaunchKernelGGL(gallery_match_kernel<NT>, grid, dim3(kGlThreads), (unsigned)lds, s, q, g,
                     scale, count, part, M, D, cap, K);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}

}  // namespace
}  // namespace kvedge

using namespace kvedge;

extern "C" int kv_embed_quantize(const void* x, signed char* codes, int* nrm2, int M, int HW,
                                 int C, hipStream_t s) {
  if (C < 64 || C > kGlMaxDim || C % 64) return -1;
  if (HW < 1 || HW > 256) return -2;
  if (M < 0 || M > kGlMaxM) return -3;
  if ((reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(codes) & 3) ||
      (reinterpret_cast<uintptr_t>(nrm2) & 3))
    return -7;
  if (M == 0) return 0;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(x, (long long)M * HW * C * 2)) return -20;
  if (!rs_in_alloc(codes, (long long)M * C)) return -21;
  if (!rs_in_alloc(nrm2, (long long)M * 4)) return -22;
#endif
  hipLaunchKernelGGL(embed_quantize_kernel, dim3((unsigned)M), dim3(kEqThreads), 0, s,
                     static_cast<const unsigned short*>(x), codes, nrm2, HW, C);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}

extern "C" int kv_gallery_workgroups(int cap) {
  if (cap < 1 || cap > kGlMaxCap) return -1;
  return gl_workgroups(cap);
}

extern "C" int kv_gallery_match(const signed char* q, const signed char* codes,
                                const float* scale, const int* count, void* part,
                                long long part_bytes, float* score, int* row, int M, int D,
                                int cap, int K, hipStream_t s) {
  if (D < 64 || D > kGlMaxDim || D % 64) return -1;
  if (M < 1 || M > kGlMaxM) return -2;
  if (cap < 1 || cap > kGlMaxCap) return -3;
  if (K < 1 || K > kGlMaxTop) return -4;
  const int nwg = gl_workgroups(cap);
  if (part_bytes < (long long)M * nwg * K * 8) return -5;
  if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(codes)) & 15) return -7;
  if ((reinterpret_cast<uintptr_t>(scale) | reinterpret_cast<uintptr_t>(count) |
       reinterpret_cast<uintptr_t>(score) | reinterpret_cast<uintptr_t>(row)) & 3)
    return -7;
  if (reinterpret_cast<uintptr_t>(part) & 7) return -7;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(q, (long long)M * D)) return -20;
  if (!rs_in_alloc(codes, (long long)cap * D)) return -21;
  if (!rs_in_alloc(scale, (long long)cap * 4)) return -22;
  if (!rs_in_alloc(count, 4)) return -23;
  if (!rs_in_alloc(part, (long long)M * nwg * K * 8)) return -24;
  if (!rs_in_alloc(score, (long long)M * K * 4)) return -25;
  if (!rs_in_alloc(row, (long long)M * K * 4)) return -26;
#endif
  Cand* p = static_cast<Cand*>(part);
  const int mt = M < kGlQTile ? M : kGlQTile;
  int rc;
  if (mt <= 32) rc = gl_launch<1>(q, codes, scale, count, p, M, D, cap, K, nwg, s);
  else if (mt <= 64) rc = gl_launch<2>(q, codes, scale, count, p, M, D, cap, K, nwg, s);
  else if (mt <= 128) rc = gl_launch<4>(q, codes, scale, count, p, M, D, cap, K, nwg, s);
  else rc = gl_launch<8>(q, codes, scale, count, p, M, D, cap, K, nwg, s);
  if (rc) return rc;
  hipLaunchKernelGGL(gallery_merge_kernel, dim3((unsigned)M), dim3(kWave), 0, s, p, score, row,
                     nwg, K);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}
