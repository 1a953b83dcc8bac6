// K23 (motion regions): groups the moving cells of the frame watch's grid (K20) into connected
// blobs and reports the largest of them as detection rows -- where is something moving, and how
// large is it -- one launch, inside the captured step, no host in the loop.
//
// Per camera: mask uint8 [GH, GW] (bit 0 = the cell moved; K20's motion_mask) and ignore uint8
// [GH, GW] (non-zero = masked out: a tree, a road, a clock overlay).  GH = ceil(Hs / cell), GW =
// ceil(Ws / cell), C = GH GW <= 32768 cells.  Camera n of the launch is stream slot0 + n: its
// ignore row and its int32 [4] parameter row = min_cells, cls, 0, 0 (read only; clamped here into
// 1..C and 0..65535 whatever the row holds).
//
// The rule (ops.reference.motion_blobs writes it as a flood fill; this equals it bit for bit):
//   active = (mask & 1) != 0 && ignore == 0; components of the active cells under 4- or
//   8-connectivity; per component n cells, the inclusive cell box cx0 cy0 cx1 cy1, first = its
//   smallest linear index y GW + x.  Kept: n >= min_cells.  Kept components ordered by n
//   descending, then first ascending; the first R (det's rows, 1..64) are reported:
//   count = min(kept, R); det[r] = (cx0 cell, cy0 cell, min((cx1 + 1) cell, Ws),
//   min((cy1 + 1) cell, Hs), n, cls) as fp32 (all exact integers), rows >= count all zero;
//   labels int32 [GH, GW] = r on the cells of reported blob r, -1 everywhere else.
//   Every element of det, count and labels is written.
//
// Launch shape: ONE WORKGROUP OF 1024 PER CAMERA, everything between the first read and the last
// write in LDS.  The unit of labelling is the RUN (a maximal horizontal stretch of active cells),
// not the cell: a row of GW cells has at most ceil(GW / 2) runs, so NRcap = GH ceil(GW / 2)
// <= 16640 run slots, and a long horizontal stretch is one node whatever its length.
// LDS, in ints (W = GH WPR words of row bits, WPR = ceil(GW / 32); < 154 KB at the worst grid):
//   parent [NRcap] | cnt [NRcap] | bits [W] | starts [W] | wbase [W] | the selection's scratch
//  (1) bits: the mask and then the ignore bytes are read once in 16-byte chunks (the edge chunks
//      of a row that does not start on 16 bytes byte by byte), squeezed to one bit per cell and
//      ORed (mask) / AND-NOTed (ignore) into the row words with LDS atomics.
//  (2) runs: starts = bits & ~(bits << 1 with the carry of the word to the left); a workgroup
//      exclusive scan of popcount(starts) gives wbase, so the run of cell (w, b) has the id
//      wbase[w] + popcount(starts[w] & bits <= b) - 1: ids ascend in raster order, the smallest
//      id of a component is the run that holds `first`.
//  (3) union-find over run ids, a half-wave per row word, a lane per cell: a cell unions its run
//      with the run above it where one of the two starts (once per overlapping pair), and under
//      8-connectivity with the run up-left / up-right when neither the cell above nor the cell
//      beside it bridges the gap.  find halves paths with LDS atomicMin; union hooks the larger
//      root under the smaller with LDS atomicMin and goes on with whatever it displaced, so the
//      cost follows the number of runs, not the diameter of a component.  Then every run's
//      parent is flattened to its root.
//  (4) cnt[root] += run length (LDS atomicAdd by the lane of the run's first cell).
//  (5) selection without a list: thread t owns the slots t, t + 1024, ... and keeps the largest
//      key = n << 15 | (32767 - root) among its kept roots; R rounds of a workgroup argmax (wave
//      shuffles, 16 wave maxima double-buffered in LDS, one barrier a round); keys are distinct,
//      so every lane agrees on the winner, whose owner records it, drops it and rescans its
//      slots.  A round that finds nothing ends it: count.
//  (6) cnt becomes the map root -> r (-1: not reported); the runs of reported blobs take the
//      box with LDS atomicMin / atomicMax on [64] words (only where the word would change).
//  (7) labels: a lane per cell, whole dwords, consecutive lanes consecutive cells; det and
//      count by the first R lanes.
// No global atomics, no second launch, streams outside [slot0, slot0 + N) are not touched.
#include "common.h"
#include "kvedge_kernels.h"
#include "resample.h"  // rs_in_alloc

namespace kvedge {
namespace {

constexpr int kMbThreads = 1024, kMbWaves = kMbThreads / kWave;
constexpr int kMbMaxCells = 32768, kMbMaxBlobs = 64, kMbMaxExtent = 4096;
constexpr int kMbSmall = 6 * kMbMaxBlobs + 3 * kMbWaves;  // sel root, n, box [4] | wmax [2] | scan
constexpr int kMbMaxLds = 160 * 1024;

struct MbGeom {
  int GH, GW, C, WPR, W, NRcap;
};

__host__ __device__ inline MbGeom mb_geom(int Hs, int Ws, int cell) {
  MbGeom g;
  g.GH = (Hs + cell - 1) / cell;
  g.GW = (Ws + cell - 1) / cell;
  g.C = g.GH * g.GW;
  g.WPR = (g.GW + 31) / 32;
  g.W = g.GH * g.WPR;
  g.NRcap = g.GH * ((g.GW + 1) / 2);
  return g;
}

__host__ __device__ inline int mb_lds_ints(const MbGeom& g) {
  return 2 * g.NRcap + 3 * g.W + kMbSmall;
}

__device__ __forceinline__ int mb_ld(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// bytes 0..3 of x -> bits 0..3: bit 0 of every byte (mask), or byte != 0 (ignore)
template <bool IGNORE>
__device__ __forceinline__ unsigned mb_nib(unsigned x) {
  unsigned t;
  if constexpr (IGNORE) t = ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) >> 7) & 0x01010101u;
  else t = x & 0x01010101u;
  return (t * 0x01020408u) >> 24 & 0xfu;
}

// (1): the C bytes at p, one bit per cell, into the row words: OR for the mask, AND-NOT for
// the ignore bytes.  Chunk k covers the 16-byte-aligned bytes [16 k - a, 16 k - a + 16) of p.
template <bool IGNORE>
__device__ __forceinline__ void mb_scatter(const uint8_t* __restrict__ p, const MbGeom& g,
                                           unsigned* bits, int tid) {
  const int a = (int)(reinterpret_cast<uintptr_t>(p) & 15);
  const int nchunk = (a + g.C + 15) >> 4;
  for (int k = tid; k < nchunk; k += kMbThreads) {
    int c = k * 16 - a;
    unsigned v = 0;
    if (c >= 0 && c + 16 <= g.C) {
      const uint4 q = *reinterpret_cast<const uint4*>(p + c);
      v = mb_nib<IGNORE>(q.x) | mb_nib<IGNORE>(q.y) << 4 | mb_nib<IGNORE>(q.z) << 8 |
          mb_nib<IGNORE>(q.w) << 12;
    } else {
      for (int i = 0; i < 16; ++i) {
        const int ci = c + i;
        if (ci >= 0 && ci < g.C && (IGNORE ? p[ci] != 0 : (p[ci] & 1) != 0)) v |= 1u << i;
      }
    }
    if (c < 0) {
      v >>= -c;
      c = 0;
    }
    if (v == 0) continue;
    int y = c / g.GW, x = c - y * g.GW;
    while (v) {  // v's bit 0 is cell (y, x); set bits lie inside the grid
      const int take = min(min(16, g.GW - x), 32 - (x & 31));
      const unsigned part = (v & ((1u << take) - 1u)) << (x & 31);
      if (part) {
        unsigned* w = bits + y * g.WPR + (x >> 5);
        if constexpr (IGNORE) atomicAnd(w, ~part);
        else atomicOr(w, part);
      }
      v >>= take;
      x += take;
      if (x == g.GW) {
        x = 0;
        ++y;
      }
    }
  }
}

// id of the run that holds the active cell at bit b of word w
__device__ __forceinline__ int mb_run(const unsigned* starts, const int* wbase, int w, int b) {
  const unsigned upto = b == 31 ? ~0u : (2u << b) - 1u;
  return wbase[w] + __popc(starts[w] & upto) - 1;
}

// cells of the run that starts at bit b of word w, word j of its row
__device__ __forceinline__ int mb_run_len(const unsigned* bits, int w, int j, int b, int WPR) {
  const unsigned rest = ~(bits[w] >> b);  // the shifted-in zeros end it at the word's edge
  int len = __ffs(rest) - 1;              // rest == 0: b == 0 and a full word
  if (rest == 0u) len = 32;
  if (b + len < 32) return len;
  for (++j, ++w; j < WPR; ++j, ++w) {
    const unsigned t = ~bits[w];
    if (t) return len + __ffs(t) - 1;
    len += 32;
  }
  return len;
}

__device__ __forceinline__ int mb_find(int* parent, int x) {
  int p = mb_ld(parent + x);
  while (p != x) {
    const int gp = mb_ld(parent + p);
    if (gp != p) atomicMin(parent + x, gp);  // path halving: only ever an ancestor, only down
    x = p;
    p = gp;
  }
  return x;
}

__device__ __forceinline__ void mb_union(int* parent, int a, int b) {
  for (;;) {
    a = mb_find(parent, a);
    b = mb_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(parent + a, b);
    if (old == a) return;  // a was still a root: hooked
    a = old;               // a had been hooked meanwhile: what it pointed at still has to meet b
  }
}

__device__ __forceinline__ int mb_wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, kWave));
  return v;
}

// a thread's best key among the slots it owns
__device__ __forceinline__ int mb_best(const int* parent, const int* cnt, int NR, int minc,
                                       int tid) {
  int best = 0;
  for (int i = tid; i < NR; i += kMbThreads) {
    const int n = cnt[i];
    if (parent[i] == i && n >= minc) best = max(best, n << 15 | (32767 - i));
  }
  return best;
}

__global__ __launch_bounds__(kMbThreads) void motion_blobs_kernel(
    const uint8_t* __restrict__ mask, const int* __restrict__ params,
    const uint8_t* __restrict__ ignore, float* __restrict__ det, int* __restrict__ count,
    int* __restrict__ labels, int slot0, int cell, int Hs, int Ws, int R, int conn8) {
  extern __shared__ __attribute__((aligned(16))) int mb_lds[];
  const MbGeom g = mb_geom(Hs, Ws, cell);
  int* parent = mb_lds;
  int* cnt = parent + g.NRcap;
  unsigned* bits = reinterpret_cast<unsigned*>(cnt + g.NRcap);
  unsigned* starts = bits + g.W;
  int* wbase = reinterpret_cast<int*>(starts + g.W);
  int* sel_root = wbase + g.W;
  int* sel_n = sel_root + kMbMaxBlobs;
  int* box = sel_n + kMbMaxBlobs;  // x0 [64] | y0 | x1 | y1
  int* wmax = box + 4 * kMbMaxBlobs;
  int* scan = wmax + 2 * kMbWaves;

  const int n = (int)blockIdx.x, tid = (int)threadIdx.x;
  const int lane = tid & (kWave - 1), wave = tid >> 6;
  const int hw = tid >> 5, bit = tid & 31;  // (3)..(7): a half-wave per row word
  const int* par = params + (long long)(slot0 + n) * 4;
  const int minc = min(max(par[0], 1), g.C);
  const int cls = min(max(par[1], 0), 65535);

  // (1)
  for (int w = tid; w < g.W; w += kMbThreads) bits[w] = 0u;
  __syncthreads();
  mb_scatter<false>(mask + (long long)n * g.C, g, bits, tid);
  __syncthreads();
  mb_scatter<true>(ignore + (long long)(slot0 + n) * g.C, g, bits, tid);
  __syncthreads();

  // (2) thread t takes the words [t wpt, t wpt + wpt): the scan runs in raster order
  const int wpt = (g.W + kMbThreads - 1) / kMbThreads;
  int mine = 0;
  for (int i = 0; i < wpt; ++i) {
    const int w = tid * wpt + i;
    if (w >= g.W) break;
    const unsigned b = bits[w];
    const unsigned left = (w % g.WPR) ? bits[w - 1] >> 31 : 0u;
    const unsigned s = b & ~(b << 1 | left);
    starts[w] = s;
    mine += __popc(s);
  }
  int incl = mine;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int t = __shfl_up(incl, o, kWave);
    if (lane >= o) incl += t;
  }
  if (lane == kWave - 1) scan[wave] = incl;
  __syncthreads();
  int base = incl - mine, NR = 0;
#pragma unroll
  for (int k = 0; k < kMbWaves; ++k) {
    const int t = scan[k];
    if (k < wave) base += t;
    NR += t;
  }
  for (int i = 0; i < wpt; ++i) {
    const int w = tid * wpt + i;
    if (w >= g.W) break;
    wbase[w] = base;
    base += __popc(starts[w]);
  }
  for (int i = tid; i < NR; i += kMbThreads) {
    parent[i] = i;
    cnt[i] = 0;
  }
  __syncthreads();

  // (3)
  for (int w = g.WPR + hw; w < g.W; w += kMbThreads / 32) {
    const int j = w % g.WPR, u = w - g.WPR;
    const unsigned cur = bits[w], up = bits[u];
    if (!(cur >> bit & 1u)) continue;
    const unsigned m4 = up & (starts[w] | starts[u]);
    unsigned mul = 0u, mur = 0u;
    if (conn8) {
      const bool l = j > 0, r = j + 1 < g.WPR;
      const unsigned cur_l = cur << 1 | (l ? bits[w - 1] >> 31 : 0u);
      const unsigned up_l = up << 1 | (l ? bits[u - 1] >> 31 : 0u);
      const unsigned cur_r = cur >> 1 | (r ? bits[w + 1] << 31 : 0u);
      const unsigned up_r = up >> 1 | (r ? bits[u + 1] << 31 : 0u);
      mul = up_l & ~up & ~cur_l;
      mur = up_r & ~up & ~cur_r;
    }
    if (!((m4 | mul | mur) >> bit & 1u)) continue;
    const int me = mb_run(starts, wbase, w, bit);
    if (m4 >> bit & 1u) mb_union(parent, me, mb_run(starts, wbase, u, bit));
    if (mul >> bit & 1u)
      mb_union(parent, me, bit ? mb_run(starts, wbase, u, bit - 1)
                               : mb_run(starts, wbase, u - 1, 31));
    if (mur >> bit & 1u)
      mb_union(parent, me, bit < 31 ? mb_run(starts, wbase, u, bit + 1)
                                    : mb_run(starts, wbase, u + 1, 0));
  }
  __syncthreads();
  for (int i = tid; i < NR; i += kMbThreads) {
    int x = i, p = mb_ld(parent + x);
    while (p != x) {
      x = p;
      p = mb_ld(parent + x);
    }
    parent[i] = x;  // others may still walk through i: the root is an ancestor too
  }
  __syncthreads();

  // (4)
  for (int w = hw; w < g.W; w += kMbThreads / 32) {
    if (!(starts[w] >> bit & 1u)) continue;
    const int len = mb_run_len(bits, w, w % g.WPR, bit, g.WPR);
    atomicAdd(cnt + parent[mb_run(starts, wbase, w, bit)], len);
  }
  __syncthreads();

  // (5)
  int best = mb_best(parent, cnt, NR, minc, tid);
  int found = 0;
  for (; found < R; ++found) {
    const int wm = mb_wave_max(best);
    int* slot = wmax + (found & 1) * kMbWaves;
    if (lane == 0) slot[wave] = wm;
    __syncthreads();
    int win = 0;
#pragma unroll
    for (int k = 0; k < kMbWaves; ++k) win = max(win, slot[k]);
    if (win == 0) break;  // the same for every lane
    if (best == win) {    // keys are distinct: one owner
      const int root = 32767 - (win & 32767);
      sel_root[found] = root;
      sel_n[found] = win >> 15;
      cnt[root] = 0;
      best = mb_best(parent, cnt, NR, minc, tid);
    }
  }
  __syncthreads();

  // (6)
  for (int i = tid; i < NR; i += kMbThreads) cnt[i] = -1;
  if (tid < kMbMaxBlobs) {
    box[tid] = box[kMbMaxBlobs + tid] = 0x7fffffff;
    box[2 * kMbMaxBlobs + tid] = box[3 * kMbMaxBlobs + tid] = -1;
  }
  __syncthreads();
  if (tid < found) cnt[sel_root[tid]] = tid;
  __syncthreads();
  for (int w = hw; w < g.W; w += kMbThreads / 32) {
    if (!(starts[w] >> bit & 1u)) continue;
    const int r = cnt[parent[mb_run(starts, wbase, w, bit)]];
    if (r < 0) continue;
    const int y = w / g.WPR, j = w - y * g.WPR;
    const int x0 = j * 32 + bit, x1 = x0 + mb_run_len(bits, w, j, bit, g.WPR) - 1;
    // a stale read is only ever on the safe side: the words move one way
    if (x0 < mb_ld(box + r)) atomicMin(box + r, x0);
    if (y < mb_ld(box + kMbMaxBlobs + r)) atomicMin(box + kMbMaxBlobs + r, y);
    if (x1 > mb_ld(box + 2 * kMbMaxBlobs + r)) atomicMax(box + 2 * kMbMaxBlobs + r, x1);
    if (y > mb_ld(box + 3 * kMbMaxBlobs + r)) atomicMax(box + 3 * kMbMaxBlobs + r, y);
  }
  __syncthreads();

  // (7)
  int* lab = labels + (long long)n * g.C;
  for (int w = hw; w < g.W; w += kMbThreads / 32) {
    const int y = w / g.WPR, x = (w - y * g.WPR) * 32 + bit;
    if (x >= g.GW) continue;
    int r = -1;
    if (bits[w] >> bit & 1u) r = cnt[parent[mb_run(starts, wbase, w, bit)]];
    lab[y * g.GW + x] = r;
  }
  if (tid < R) {
    float* d = det + ((long long)n * R + tid) * 6;
    const bool on = tid < found;
    d[0] = on ? (float)(box[tid] * cell) : 0.f;
    d[1] = on ? (float)(box[kMbMaxBlobs + tid] * cell) : 0.f;
    d[2] = on ? (float)min((box[2 * kMbMaxBlobs + tid] + 1) * cell, Ws) : 0.f;
    d[3] = on ? (float)min((box[3 * kMbMaxBlobs + tid] + 1) * cell, Hs) : 0.f;
    d[4] = on ? (float)sel_n[tid] : 0.f;
    d[5] = on ? (float)cls : 0.f;
  }
  if (tid == 0) count[n] = found;
}

}  // namespace
}  // namespace kvedge

using namespace kvedge;

extern "C" int kv_motion_blobs_max_cells(void) { return kMbMaxCells; }

extern "C" int kv_motion_blobs(const unsigned char* mask, const int* params,
                               const unsigned char* ignore, float* det, int* count, int* labels,
                               int N, int S, int slot0, int Hs, int Ws, int cell, int max_blobs,
                               int connectivity, hipStream_t s) {
  if (Hs < 1 || Hs > kMbMaxExtent || Ws < 1 || Ws > kMbMaxExtent) return -1;
  if (N < 0 || S < 0 || slot0 < 0 || (long long)slot0 + N > S) return -2;
  if (cell != 8 && cell != 16 && cell != 32) return -3;
  const MbGeom g = mb_geom(Hs, Ws, cell);
  const int lds = mb_lds_ints(g) * 4;
  if (g.C > kMbMaxCells || lds > kMbMaxLds) return -4;
  if (max_blobs < 1 || max_blobs > kMbMaxBlobs) return -5;
  if (connectivity != 4 && connectivity != 8) return -6;
  if ((reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(det) |
       reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(labels)) & 3)
    return -7;
  if (N > 65535) return -9;
  if (N == 0) return 0;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(mask, (long long)N * g.C)) return -20;
  if (!rs_in_alloc(params + (long long)slot0 * 4, (long long)N * 16)) return -21;
  if (!rs_in_alloc(ignore + (long long)slot0 * g.C, (long long)N * g.C)) return -22;
  if (!rs_in_alloc(det, (long long)N * max_blobs * 24)) return -23;
  if (!rs_in_alloc(count, (long long)N * 4)) return -24;
  if (!rs_in_alloc(labels, (long long)N * g.C * 4)) return -25;
#endif
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(motion_blobs_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
    return -100;
  hipLaunchKernelGGL(motion_blobs_kernel, dim3((unsigned)N), dim3(kMbThreads), (unsigned)lds, s,
                     mask, params, ignore, det, count, labels, slot0, cell, Hs, Ws, max_blobs,
                     connectivity == 8 ? 1 : 0);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}
