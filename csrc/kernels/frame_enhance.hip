// K26 (frame enhance): low-light enhancement of the model-size frames, one camera per batch
// row -- contrast-limited adaptive histogram equalisation (CLAHE) of the luma, blended in at a
// per-camera weight, chroma kept.  Two launches inside the captured step, the per-camera
// settings in device memory, all of it integer arithmetic: byte-identical to
// ops.reference.frame_enhance, where the rules are written out.
//
// Device memory (an ops.FrameEnhance):
//   params int32 [S, 8] = mode (0 off, 1 on, 2 auto), strength (0..256), clip_q8 (256..16384),
//     lo16, hi16 (1/16 luma), 0 x3 -- read only, clamped into those ranges whatever they hold
//     (hi16 further to >= lo16 + 16), so a setter takes effect on the next replay and a bad
//     word can neither index outside a table nor divide by zero;
//   axis int32 [W + H + TY + 2] = per column, then per row, cell | w << 8 (cell k of an axis
//     reads the tables of tiles max(k - 1, 0) and min(k, T - 1), w / 64 of the way to the
//     second), then the first row of each of the TY + 1 row bands and H;
//   luts uint8 [S, TY TX, 256] and sums uint32 [S, TY TX]: written by the first launch, read
//     by the second.
//
// Launch 1, tables: one workgroup of four waves per (camera, tile).
//   The tile's rows are cut into groups of four pixels = three aligned dwords where the frame
//   allows it (W % 4 == 0 and a dword-aligned base; the up to three pixels in front of and
//   behind the aligned run, and every pixel of other frames, go byte by byte).  The lanes are
//   laid over (row, group) with a power-of-two row pitch, so no index is divided.
//   Histogram: every wave owns COPIES interleaved 256-bin copies in LDS (bin v of copy c at
//   v COPIES + c; a lane adds to copy lane % COPIES with ds_add_u32).  A dark frame puts nearly
//   every pixel of a wave-instruction into a handful of bins, the worst same-address case
//   there is; the copies cut the lanes per address by COPIES and spread them over banks.
//   32-bit counters: a tile may hold 2^24 pixels.
//   After the merge (one thread per bin, one barrier) wave 0 holds four bins per lane and
//   finishes alone, no further barrier: the tile's luma sum (sum of v hist[v]), the clip, the
//   excess by wave reduction, the closed-form redistribution, the prefix sum by a wave scan,
//   four divisions per lane, and one dword store per lane = the 256-byte table.
// Launch 2, apply: one workgroup per (row chunk, row band, camera); band b = the rows between
//   two rows of tile centres, which share their two table rows.
//   Every workgroup sums the camera's tile sums (<= 256 words) for mean16 and alpha and leaves
//   at once when alpha == 0 in place.  It stages, for each of the TX + 1 column cells, 256
//   dwords {A, B, C, D} = the four corner tables of that cell interleaved per luma value
//   (<= 17 KiB of LDS), so one ds_read_b32 per pixel delivers all four corners.  Then it
//   streams its rows: a lane takes four pixels (three dwords in, three out) when W % 4 == 0
//   and both bases are dword-aligned, else one pixel byte by byte.  Only bytes of the image
//   are ever stored; all image offsets are 64-bit.
// No matrix instruction fits: histogram, scan and a table gather.
#include "common.h"
#include "kvedge_kernels.h"
#include "resample.h"  // rs_in_alloc

namespace kvedge {
namespace {

constexpr int kFeMaxExtent = 4096, kFeMaxTiles = 16;
constexpr int kFeThreads = 256, kFeWaves = kFeThreads / kWave;
constexpr int kFeParamStride = 8;
constexpr int kFeChunkRows = 16;  // rows of a band per apply workgroup

__device__ __forceinline__ int fe_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ int fe_luma(int r, int g, int b) {
  return (77 * r + 150 * g + 29 * b + 128) >> 8;
}

__device__ __forceinline__ int fe_byte(unsigned w, int i) { return (int)((w >> (8 * i)) & 0xffu); }

template <int COPIES>
__global__ __launch_bounds__(kFeThreads) void frame_enhance_tables_kernel(
    const uint8_t* __restrict__ src, const int* __restrict__ params, uint8_t* __restrict__ luts,
    unsigned* __restrict__ sums, int slot0, int H, int W, int TX, int th, int tw, int vec_ok,
    int lpr_shift) {
  __shared__ unsigned s_hist[kFeWaves * 256 * COPIES];
  __shared__ __attribute__((aligned(16))) unsigned s_bins[256];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int tx = (int)blockIdx.x, ty = (int)blockIdx.y, n = (int)blockIdx.z;
  const int TY = (int)gridDim.y;
  for (int i = tid; i < kFeWaves * 256 * COPIES; i += kFeThreads) s_hist[i] = 0;
  __syncthreads();

  const int x0 = tx * tw, cw = min(tw, W - x0);
  const int y0 = ty * th, rows = min(th, H - y0);
  const uint8_t* img = src + (long long)n * H * W * 3;
  unsigned* hist = s_hist + wave * 256 * COPIES + (lane & (COPIES - 1));
  auto count = [&](int r, int g, int b) { atomicAdd(hist + fe_luma(r, g, b) * COPIES, 1u); };

  // the aligned run of the tile's rows: pixels [head, head + 4 nvec)
  const int head = vec_ok ? min((4 - (x0 & 3)) & 3, cw) : cw;
  const int nvec = (cw - head) >> 2;
  const int tail0 = head + 4 * nvec;
  {
    const int lpr = 1 << lpr_shift;
    const int c = tid & (lpr - 1);
    for (int y = tid >> lpr_shift; y < rows; y += kFeThreads >> lpr_shift) {
      const uint8_t* rowp = img + ((long long)(y0 + y) * W + x0 + head) * 3;
      for (int g = c; g < nvec; g += lpr) {
        const unsigned* p = reinterpret_cast<const unsigned*>(rowp + 12 * g);
        const unsigned w0 = p[0], w1 = p[1], w2 = p[2];
        count(fe_byte(w0, 0), fe_byte(w0, 1), fe_byte(w0, 2));
        count(fe_byte(w0, 3), fe_byte(w1, 0), fe_byte(w1, 1));
        count(fe_byte(w1, 2), fe_byte(w1, 3), fe_byte(w2, 0));
        count(fe_byte(w2, 1), fe_byte(w2, 2), fe_byte(w2, 3));
      }
    }
  }
  // what is left of every row, byte by byte
  const int left = cw - 4 * nvec;
  for (int i = tid; i < rows * left; i += kFeThreads) {
    const int y = i / left, j = i - y * left;
    const int x = j < head ? j : tail0 + (j - head);
    const uint8_t* p = img + ((long long)(y0 + y) * W + x0 + x) * 3;
    count(p[0], p[1], p[2]);
  }
  __syncthreads();

  {  // merge: thread v sums bin v over the waves and their copies
    unsigned t = 0;
#pragma unroll
    for (int w = 0; w < kFeWaves; ++w)
#pragma unroll
      for (int c = 0; c < COPIES; ++c) t += s_hist[w * 256 * COPIES + tid * COPIES + c];
    s_bins[tid] = t;
  }
  __syncthreads();
  if (wave != 0) return;

  // wave 0: bins 4 lane .. 4 lane + 3
  const uint4 q = reinterpret_cast<const uint4*>(s_bins)[lane];
  unsigned b[4] = {q.x, q.y, q.z, q.w};
  const unsigned npx = (unsigned)(rows * cw);  // 1 .. 2^24
  const int clip_q8 =
      fe_clamp(params[(long long)(slot0 + n) * kFeParamStride + 2], 256, 16384);
  const unsigned L = max(1u, (unsigned)(((unsigned long long)clip_q8 * npx) >> 16));
  unsigned lsum = 0, excess = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    lsum += (unsigned)(4 * lane + k) * b[k];  // <= 255 * 2^24
    excess += b[k] > L ? b[k] - L : 0u;
    b[k] = min(b[k], L);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lsum += __shfl_xor(lsum, o, kWave);
    excess += __shfl_xor(excess, o, kWave);
  }
  const unsigned every = excess >> 8, r = excess & 255u;
  const unsigned step = r ? 256u / r : 1u;
  unsigned c[4];
  unsigned run = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned v = (unsigned)(4 * lane + k);
    run += b[k] + every + ((r && v % step == 0 && v / step < r) ? 1u : 0u);
    c[k] = run;
  }
  unsigned incl = run;  // inclusive scan of the lanes' totals
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const unsigned u = __shfl_up(incl, o, kWave);
    if (lane >= o) incl += u;
  }
  const unsigned before = incl - run;
  unsigned word = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)  // 255 c + n / 2 < 2^32
    word |= ((255u * (c[k] + before) + npx / 2) / npx) << (8 * k);
  const long long tile = (long long)(slot0 + n) * (TY * TX) + ty * TX + tx;
  reinterpret_cast<unsigned*>(luts + tile * 256)[lane] = word;
  if (lane == 0) sums[tile] = lsum;
}

// one pixel: the four corners from the staged cell table, the bilinear blend, the luma shift
__device__ __forceinline__ int fe_shift(const unsigned* s_tab, int xw, int TX, int wy, int Y,
                                        int alpha) {
  const int cell = min(xw & 0xff, TX), wx = min((xw >> 8) & 0xff, 64);
  const unsigned t = s_tab[cell * 256 + Y];
  const int top = (64 - wx) * fe_byte(t, 0) + wx * fe_byte(t, 1);
  const int bot = (64 - wx) * fe_byte(t, 2) + wx * fe_byte(t, 3);
  const int Y2 = ((64 - wy) * top + wy * bot + 2048) >> 12;
  return ((Y2 - Y) * alpha) >> 8;  // arithmetic: floor
}

__device__ __forceinline__ unsigned fe_sat(int v) { return (unsigned)fe_clamp(v, 0, 255); }

template <bool VEC>
__global__ __launch_bounds__(kFeThreads) void frame_enhance_apply_kernel(
    const uint8_t* src, uint8_t* dst, const int* __restrict__ params,
    const int* __restrict__ axis, const uint8_t* __restrict__ luts,
    const unsigned* __restrict__ sums, int* __restrict__ stats, int slot0, int H, int W, int TY,
    int TX, FastDiv per_row) {
  __shared__ __attribute__((aligned(16))) unsigned s_tab[(kFeMaxTiles + 1) * 256];
  __shared__ unsigned long long s_part[kFeWaves];
  __shared__ int s_alpha;
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
  const int band = (int)blockIdx.y, n = (int)blockIdx.z, cam = slot0 + n;
  const int* xtab = axis;
  const int* ytab = axis + W;
  const int* ystart = ytab + H;
  const bool first = blockIdx.x == 0 && band == 0;  // writes the camera's stats
  const int yb0 = fe_clamp(ystart[band], 0, H), yb1 = fe_clamp(ystart[band + 1], yb0, H);
  const int ya = min(yb0 + (int)blockIdx.x * kFeChunkRows, yb1);
  const int yb = min(ya + kFeChunkRows, yb1);
  if (ya >= yb && !first) return;  // (uniform: before the first barrier)

  const int T = TY * TX;  // <= 256 tiles: one per thread
  unsigned long long part = tid < T ? sums[(long long)cam * T + tid] : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, kWave);
  if (lane == 0) s_part[wave] = part;
  __syncthreads();
  if (tid == 0) {
    unsigned long long total = 0;
#pragma unroll
    for (int w = 0; w < kFeWaves; ++w) total += s_part[w];
    const unsigned long long P = (unsigned long long)H * W;
    const int mean16 = (int)((16ull * total + P / 2) / P);
    const int* par = params + (long long)cam * kFeParamStride;
    const int mode = fe_clamp(par[0], 0, 2), strength = fe_clamp(par[1], 0, 256);
    const int lo16 = fe_clamp(par[3], 0, 4080);
    const int hi16 = max(fe_clamp(par[4], 16, 4096), lo16 + 16);
    int alpha = 0;
    if (mode == 1) alpha = strength;
    if (mode == 2)  // (a negative quotient clamps to 0 whichever way it rounds)
      alpha = (strength * fe_clamp((hi16 - mean16) * 256 / (hi16 - lo16), 0, 256)) >> 8;
    if (first) {
      stats[2 * n] = mean16;
      stats[2 * n + 1] = alpha;
    }
    s_alpha = alpha;
  }
  __syncthreads();
  const int alpha = s_alpha;
  if (ya >= yb || (alpha == 0 && src == dst)) return;

  {  // stage: thread task = (column cell k, luma values 4 q .. 4 q + 3)
    const int t0y = max(band - 1, 0), t1y = min(band, TY - 1);
    const unsigned* L = reinterpret_cast<const unsigned*>(luts + (long long)cam * T * 256);
    for (int task = tid; task < (TX + 1) * 64; task += kFeThreads) {
      const int k = task >> 6, q = task & 63;
      const int t0x = max(k - 1, 0), t1x = min(k, TX - 1);
      const unsigned a = L[(t0y * TX + t0x) * 64 + q], b = L[(t0y * TX + t1x) * 64 + q];
      const unsigned c = L[(t1y * TX + t0x) * 64 + q], d = L[(t1y * TX + t1x) * 64 + q];
      unsigned o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        o[j] = (unsigned)(fe_byte(a, j) | (fe_byte(b, j) << 8) | (fe_byte(c, j) << 16)) |
               ((unsigned)fe_byte(d, j) << 24);
      reinterpret_cast<uint4*>(s_tab)[task] = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
  __syncthreads();

  const long long frame = (long long)n * H * W * 3;
  const int items = (yb - ya) * per_row.d;  // <= 16 * 4096: fdiv's range
  for (int i = tid; i < items; i += kFeThreads) {
    const int ry = per_row.d == 1 ? i : fdiv(i, per_row);  // (no 32-bit magic for 1)
    const int rx = fmod_(i, ry, per_row);
    const int y = ya + ry;
    const int wy = min((ytab[y] >> 8) & 0xff, 64);
    if constexpr (VEC) {
      const long long off = frame + ((long long)y * W + 4 * rx) * 3;
      const unsigned* p = reinterpret_cast<const unsigned*>(src + off);
      const unsigned w0 = p[0], w1 = p[1], w2 = p[2];
      const int4 xw = reinterpret_cast<const int4*>(xtab)[rx];
      int c[12] = {fe_byte(w0, 0), fe_byte(w0, 1), fe_byte(w0, 2), fe_byte(w0, 3),
                   fe_byte(w1, 0), fe_byte(w1, 1), fe_byte(w1, 2), fe_byte(w1, 3),
                   fe_byte(w2, 0), fe_byte(w2, 1), fe_byte(w2, 2), fe_byte(w2, 3)};
      const int xws[4] = {xw.x, xw.y, xw.z, xw.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int Y = fe_luma(c[3 * k], c[3 * k + 1], c[3 * k + 2]);
        const int d = fe_shift(s_tab, xws[k], TX, wy, Y, alpha);
        c[3 * k] += d;
        c[3 * k + 1] += d;
        c[3 * k + 2] += d;
      }
      unsigned o[3];
#pragma unroll
      for (int k = 0; k < 3; ++k)
        o[k] = fe_sat(c[4 * k]) | (fe_sat(c[4 * k + 1]) << 8) | (fe_sat(c[4 * k + 2]) << 16) |
               (fe_sat(c[4 * k + 3]) << 24);
      unsigned* out = reinterpret_cast<unsigned*>(dst + off);
      out[0] = o[0];
      out[1] = o[1];
      out[2] = o[2];
    } else {
      const long long off = frame + ((long long)y * W + rx) * 3;
      const int r = src[off], g = src[off + 1], b = src[off + 2];
      const int d = fe_shift(s_tab, xtab[rx], TX, wy, fe_luma(r, g, b), alpha);
      dst[off] = (uint8_t)fe_sat(r + d);
      dst[off + 1] = (uint8_t)fe_sat(g + d);
      dst[off + 2] = (uint8_t)fe_sat(b + d);
    }
  }
}

}  // namespace
}  // namespace kvedge

using namespace kvedge;

extern "C" int kv_frame_enhance(const unsigned char* src, unsigned char* dst, const int* params,
                                const int* axis, unsigned char* luts, int* sums, int* stats,
                                int N, int S, int slot0, int H, int W, int TY, int TX,
                                int hist_copies, hipStream_t s) {
  if (H < 1 || H > kFeMaxExtent || W < 1 || W > kFeMaxExtent) return -1;
  if (N < 0 || S < 0 || slot0 < 0 || (long long)slot0 + N > S) return -2;
  if (TY < 1 || TY > kFeMaxTiles || TX < 1 || TX > kFeMaxTiles) return -3;
  const int th = (H + TY - 1) / TY, tw = (W + TX - 1) / TX;
  if ((TY - 1) * th >= H || (TX - 1) * tw >= W) return -4;  // an empty tile
  if (hist_copies != 1 && hist_copies != 2 && hist_copies != 4 && hist_copies != 8) return -5;
  if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(luts) |
       reinterpret_cast<uintptr_t>(sums) | reinterpret_cast<uintptr_t>(stats)) & 3)
    return -7;
  if (reinterpret_cast<uintptr_t>(axis) & 15) return -8;
  if (N > 65535) return -9;  // grid z
  if (N == 0) return 0;
  const long long frame_bytes = (long long)H * W * 3;
#ifdef KVEDGE_CHECKS
  const long long T = (long long)TY * TX;
  if (!rs_in_alloc(src, N * frame_bytes)) return -20;
  if (!rs_in_alloc(dst, N * frame_bytes)) return -21;
  if (!rs_in_alloc(params + (long long)slot0 * kFeParamStride, (long long)N * kFeParamStride * 4))
    return -22;
  if (!rs_in_alloc(axis, ((long long)W + H + TY + 2) * 4)) return -23;
  if (!rs_in_alloc(luts + slot0 * T * 256, N * T * 256)) return -24;
  if (!rs_in_alloc(sums + slot0 * T, N * T * 4)) return -25;
  if (!rs_in_alloc(stats, (long long)N * 2 * 4)) return -26;
#endif
  const bool w4 = W % 4 == 0;
  const int vec_in = w4 && (reinterpret_cast<uintptr_t>(src) & 3) == 0;
  const bool vec_io = vec_in && (reinterpret_cast<uintptr_t>(dst) & 3) == 0;
  // lanes per tile row in the table launch: the power of two that covers its dword groups
  int lpr_shift = 0;
  while ((1 << lpr_shift) < tw / 4 && lpr_shift < 8) ++lpr_shift;
  const dim3 tgrid((unsigned)TX, (unsigned)TY, (unsigned)N);
#define KV_FE_TABLES(C)                                                                       \
  hipLaunchKernelGGL((frame_enhance_tables_kernel<C>), tgrid, dim3(kFeThreads), 0, s, src,    \
                     params, luts, reinterpret_cast<unsigned*>(sums), slot0, H, W, TX, th, tw, \
                     vec_in, lpr_shift)
  if (hist_copies == 1) KV_FE_TABLES(1);
  else if (hist_copies == 2) KV_FE_TABLES(2);
  else if (hist_copies == 4) KV_FE_TABLES(4);
  else KV_FE_TABLES(8);
#undef KV_FE_TABLES
  if (hipGetLastError() != hipSuccess) return -100;
  const dim3 agrid((unsigned)((th + kFeChunkRows - 1) / kFeChunkRows), (unsigned)(TY + 1),
                   (unsigned)N);
  if (vec_io)
    hipLaunchKernelGGL(frame_enhance_apply_kernel<true>, agrid, dim3(kFeThreads), 0, s, src, dst,
                       params, axis, luts, reinterpret_cast<const unsigned*>(sums), stats, slot0,
                       H, W, TY, TX, make_fastdiv(W / 4));
  else
    hipLaunchKernelGGL(frame_enhance_apply_kernel<false>, agrid, dim3(kFeThreads), 0, s, src, dst,
                       params, axis, luts, reinterpret_cast<const unsigned*>(sums), stats, slot0,
                       H, W, TY, TX, make_fastdiv(W));
  return hipGetLastError() == hipSuccess ? 0 : -100;
}
