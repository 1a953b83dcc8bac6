// K20 (frame watch): looks at the frames themselves, one camera per batch row -- is anything
// moving, and is the picture usable (dark, covered, frozen, knocked to a new view).  One
// streaming pass over the luma of the native-resolution frames already in device memory, state
// in device memory, no host in the loop, inside the captured step.
//
// The frame is cut into cell x cell pixel cells (cell 8 / 16 / 32; GH = ceil(Hs / cell) rows of
// GW = ceil(Ws / cell) cells, the last row / column may be partial); of every cell only the rows
// y % row_step == 0 are sampled (row_step 1 / 2 / 4, so a cell's first row is always sampled).
// Luma of a pixel: the Y byte (NV12; the chroma rows are never read) or
// (77 R + 150 G + 29 B + 128) >> 8 (RGB).
//
// Per stream, in ints (kv_watch_state_stride(C) = 24 + 3 C of them, C = GH * GW):
//   primed @0 | run [5] @1 | raised [5] @6 | 0 x5 | params [6] @16 = motion_thr16,
//   motion_share_q, scene_share_q, dark16, flat16, hold (read only here; clamped into 0..4080,
//   0..1024, 0..1024, 0..4096, 0..4096, 1..255 whatever the row holds) | 0 x2
//   | acc [C] @24 | sum [C] | grad [C]
//
// Per cell, over its sampled pixels: n their number, sum their luma sum, grad the sum of
// |Y(x+1, y) - Y(x, y)| over horizontal neighbours both in the cell;
//   v = (16 sum + n / 2) / n                      (1/16 luma, truncating)
//   moved = primed && |v - (acc >> k)| > motion_thr16
//   acc  = primed ? acc + v - (acc >> k) : v << k      (k = bg_shift; k = 0: frame differencing)
//   same = (sum, grad) == the stored pair; the pair is then stored.
// Per camera, totals in int64, P sampled pixels, Q = sampled rows * (Ws - GW) neighbour pairs:
//   mean16 = (16 Ssum + P / 2) / P, sharp16 = (16 Sgrad + Q / 2) / Q, moving = moved cells;
//   conditions: bit 0 motion = moving > 0 && moving * 1024 >= motion_share_q * C, bit 1 scene
//   the same with scene_share_q, bit 2 dark = mean16 < dark16, bit 3 flat = sharp16 < flat16,
//   bit 4 frozen = primed && every cell same;
//   run[c] = cond ? min(run[c] + 1, 65535) : 0; alarm bit c = run[c] >= hold; raised[c] += 1
//   (wrapping) in the frame where run[c] == hold; then primed = 1.
//   stats [16] = mean16, sharp16, moving, C, conditions, alarms, run[5], raised[5].
// All of it integer arithmetic, so any reduction order gives the same answer: bit-identical to
// ops.reference.frame_watch.
//
// Launch shape, two launches:
//   cells: one lane = one cell, one wavefront = up to 64 neighbouring cells of one cell row (a
//     wave-instruction reads one contiguous run of luma, or three interleaved ones for RGB),
//     four cell rows per workgroup.  A lane walks its sampled rows with 16-byte loads (8-byte
//     for an 8-pixel NV12 cell) when the frame base and pitch are so aligned and its cell is
//     whole, byte by byte otherwise.  sum / grad / v stay in registers; the lane updates its
//     own three state words and writes its mask byte: bit 0 moved, bit 1 "pair changed" for
//     the second launch.  No LDS, no cross-lane traffic, no atomics.
//   totals: one workgroup per camera sums the per-cell results, clears bit 1 of the mask bytes,
//     and one thread steps the conditions, run counters and alarms.
// Streams outside [slot0, slot0 + N) are not touched.
#include "common.h"
#include "kvedge_kernels.h"
#include "resample.h"  // rs_in_alloc

namespace kvedge {
namespace {

constexpr int kFwHdr = 24, kFwRun = 1, kFwRaised = 6, kFwParams = 16;
constexpr int kFwConds = 5;
constexpr int kFwRowsPerBlock = 4;
constexpr int kFwMaxExtent = 4096;

__host__ __device__ constexpr int fw_vec_bytes(int bpp, int cell) {
  return (bpp * cell) % 16 == 0 ? 16 : 8;
}

__device__ __forceinline__ int fw_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <int BPP>
__device__ __forceinline__ int fw_luma(const uint8_t* p) {
  if constexpr (BPP == 1) return p[0];
  else return (77 * (int)p[0] + 150 * (int)p[1] + 29 * (int)p[2] + 128) >> 8;
}

template <int IDX, int NW>
__device__ __forceinline__ int fw_byte(const unsigned (&w)[NW]) {
  return (int)((w[IDX >> 2] >> ((IDX & 3) * 8)) & 0xffu);
}

// one whole cell row held in registers: CELL pixels = NW words
template <int BPP, int CELL, int NW>
__device__ __forceinline__ void fw_row_regs(const unsigned (&w)[NW], int& sum, int& grad) {
  if constexpr (BPP == 1) {
    // four pixels per word: v_sad_u8 against 0 sums them, against the row shifted by one
    // pixel sums the neighbour differences (the last pixel is paired with itself: 0)
    unsigned s = (unsigned)sum, g = (unsigned)grad;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      const unsigned next = w[i + 1 < NW ? i + 1 : i];  // (the last word has no next)
      const unsigned nx = i + 1 < NW ? __builtin_amdgcn_alignbyte(next, w[i], 1)
                                     : ((w[i] >> 8) | (w[i] & 0xff000000u));
      s = __builtin_amdgcn_sad_u8(w[i], 0u, s);
      g = __builtin_amdgcn_sad_u8(w[i], nx, g);
    }
    sum = (int)s;
    grad = (int)g;
  } else {
    int prev = 0;
    static_range<0, CELL>([&](auto ic) {
      constexpr int P = decltype(ic)::value;
      const int y = (77 * fw_byte<3 * P>(w) + 150 * fw_byte<3 * P + 1>(w) +
                     29 * fw_byte<3 * P + 2>(w) + 128) >> 8;
      sum += y;
      if constexpr (P > 0) grad += abs(y - prev);
      prev = y;
    });
  }
}

template <int BPP, int CELL>
__device__ __forceinline__ void fw_load_row(const uint8_t* p, unsigned (&w)[BPP * CELL / 4]) {
  constexpr int NW = BPP * CELL / 4;
  if constexpr (fw_vec_bytes(BPP, CELL) == 16) {
#pragma unroll
    for (int i = 0; i < NW / 4; ++i) {
      const uint4 v = reinterpret_cast<const uint4*>(p)[i];
      w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int i = 0; i < NW / 2; ++i) {
      const uint2 v = reinterpret_cast<const uint2*>(p)[i];
      w[2 * i] = v.x; w[2 * i + 1] = v.y;
    }
  }
}

// R sampled rows of a whole cell with all their loads in flight at once, while at least R remain
template <int BPP, int CELL, int R>
__device__ __forceinline__ void fw_rows(const uint8_t* p, long long step, int rows, int& r,
                                        int& sum, int& grad) {
  constexpr int NW = BPP * CELL / 4;
  for (; r + R <= rows; r += R) {
    unsigned w[R][NW];
#pragma unroll
    for (int q = 0; q < R; ++q) fw_load_row<BPP, CELL>(p + (r + q) * step, w[q]);
#pragma unroll
    for (int q = 0; q < R; ++q) fw_row_regs<BPP, CELL, NW>(w[q], sum, grad);
  }
}

template <int BPP, int CELL>
__global__ __launch_bounds__(kFwRowsPerBlock * kWave) void frame_watch_cells_kernel(
    const uint8_t* __restrict__ src, int* __restrict__ state, uint8_t* __restrict__ mask,
    int slot0, int Hs, int Ws, int GH, int GW, long long frame_bytes, int pitch, int row_step,
    int bg_shift, long long stride, int vec_ok) {
  constexpr int NW = BPP * CELL / 4;
  // rows in flight per lane: up to 64 registers of pixels (a whole NV12 cell of 8 or 16)
  constexpr int R = NW <= 4 ? (CELL < 16 ? CELL : 16) : NW <= 8 ? 8 : NW <= 12 ? 4 : 2;
  const int lane = (int)threadIdx.x & (kWave - 1);
  const int j = (int)blockIdx.x * kWave + lane;
  const int i = (int)blockIdx.y * kFwRowsPerBlock + ((int)threadIdx.x >> 6);
  const int n = (int)blockIdx.z;
  if (i >= GH || j >= GW) return;  // no barrier in this kernel
  const int C = GH * GW;
  const int x0 = j * CELL, cw = min(CELL, Ws - x0);
  const int y0 = i * CELL, y1 = min(Hs, y0 + CELL);
  const int rows = (y1 - y0 + row_step - 1) / row_step;  // y0 % row_step == 0
  const long long step = (long long)pitch * row_step;
  const uint8_t* p = src + (long long)n * frame_bytes + (long long)y0 * pitch + x0 * BPP;

  // the lane's state words, asked for before the pass over the pixels so that their latency
  // hides behind it
  int* st = state + (long long)(slot0 + n) * stride;
  const int c = i * GW + j;
  int* cellp = st + kFwHdr + c;
  const int primed = st[0] != 0;
  const int thr = fw_clamp(st[kFwParams + 0], 0, 4080);
  const int acc = cellp[0], old_sum = cellp[C], old_grad = cellp[2 * C];

  int sum = 0, grad = 0;
  if (vec_ok && cw == CELL) {
    int r = 0;
    fw_rows<BPP, CELL, R>(p, step, rows, r, sum, grad);
    if constexpr (R > 8) fw_rows<BPP, CELL, 8>(p, step, rows, r, sum, grad);
    if constexpr (R > 4) fw_rows<BPP, CELL, 4>(p, step, rows, r, sum, grad);
    if constexpr (R > 2) fw_rows<BPP, CELL, 2>(p, step, rows, r, sum, grad);
    fw_rows<BPP, CELL, 1>(p, step, rows, r, sum, grad);
  } else {
    for (int r = 0; r < rows; ++r) {
      const uint8_t* q = p + r * step;
      int prev = fw_luma<BPP>(q);
      sum += prev;
      for (int x = 1; x < cw; ++x) {
        const int y = fw_luma<BPP>(q + x * BPP);
        sum += y;
        grad += abs(y - prev);
        prev = y;
      }
    }
  }

  const int npx = rows * cw;  // >= 1
  const int v = (int)((unsigned)(16 * sum + npx / 2) / (unsigned)npx);
  const int bg = acc >> bg_shift;
  const bool moved = primed && abs(v - bg) > thr;
  cellp[0] = primed ? acc + v - bg : v << bg_shift;
  const bool changed = old_sum != sum || old_grad != grad;
  cellp[C] = sum;
  cellp[2 * C] = grad;
  mask[(long long)n * C + c] = (uint8_t)((moved ? 1 : 0) | (changed ? 2 : 0));
}

constexpr int kFwTotThreads = 1024;

__global__ __launch_bounds__(kFwTotThreads) void frame_watch_totals_kernel(
    int* __restrict__ state, uint8_t* __restrict__ mask, int* __restrict__ stats, int slot0,
    int C, long long P, long long Q, long long stride) {
  __shared__ unsigned long long s_sum[kFwTotThreads / kWave], s_grad[kFwTotThreads / kWave];
  __shared__ int s_mov[kFwTotThreads / kWave], s_chg[kFwTotThreads / kWave];
  const int n = (int)blockIdx.x, tid = (int)threadIdx.x;
  int* st = state + (long long)(slot0 + n) * stride;
  const int* c_sum = st + kFwHdr + C;
  const int* c_grad = c_sum + C;
  uint8_t* m = mask + (long long)n * C;
  unsigned long long ts = 0, tg = 0;
  int mov = 0, chg = 0;
  for (int c = tid; c < C; c += kFwTotThreads) {
    const int b = m[c];
    ts += (unsigned)c_sum[c];
    tg += (unsigned)c_grad[c];
    mov += b & 1;
    if (b & 2) {
      ++chg;
      m[c] = (uint8_t)(b & 1);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ts += __shfl_xor(ts, o, kWave);
    tg += __shfl_xor(tg, o, kWave);
    mov += __shfl_xor(mov, o, kWave);
    chg += __shfl_xor(chg, o, kWave);
  }
  if ((tid & (kWave - 1)) == 0) {
    s_sum[tid >> 6] = ts;
    s_grad[tid >> 6] = tg;
    s_mov[tid >> 6] = mov;
    s_chg[tid >> 6] = chg;
  }
  __syncthreads();
  if (tid != 0) return;
  ts = tg = 0;
  mov = chg = 0;
#pragma unroll
  for (int w = 0; w < kFwTotThreads / kWave; ++w) {
    ts += s_sum[w];
    tg += s_grad[w];
    mov += s_mov[w];
    chg += s_chg[w];
  }
  const int primed = st[0] != 0;
  const int share_m = fw_clamp(st[kFwParams + 1], 0, 1024);
  const int share_s = fw_clamp(st[kFwParams + 2], 0, 1024);
  const int dark16 = fw_clamp(st[kFwParams + 3], 0, 4096);
  const int flat16 = fw_clamp(st[kFwParams + 4], 0, 4096);
  const int hold = fw_clamp(st[kFwParams + 5], 1, 255);
  const int mean16 = (int)((16ull * ts + (unsigned long long)(P / 2)) / (unsigned long long)P);
  const int sharp16 = (int)((16ull * tg + (unsigned long long)(Q / 2)) / (unsigned long long)Q);
  int cond = 0;
  if (mov > 0 && mov * 1024 >= share_m * C) cond |= 1;
  if (mov > 0 && mov * 1024 >= share_s * C) cond |= 2;
  if (mean16 < dark16) cond |= 4;
  if (sharp16 < flat16) cond |= 8;
  if (primed && chg == 0) cond |= 16;
  int* out = stats + (long long)n * 16;
  int alarms = 0;
#pragma unroll
  for (int k = 0; k < kFwConds; ++k) {
    const int run = (cond >> k) & 1 ? min(st[kFwRun + k] + 1, 65535) : 0;
    int raised = st[kFwRaised + k];
    if (run >= hold) alarms |= 1 << k;
    if (run == hold) raised = (int)((unsigned)raised + 1u);
    st[kFwRun + k] = run;
    st[kFwRaised + k] = raised;
    out[6 + k] = run;
    out[11 + k] = raised;
  }
  st[0] = 1;
  out[0] = mean16;
  out[1] = sharp16;
  out[2] = mov;
  out[3] = C;
  out[4] = cond;
  out[5] = alarms;
}

template <int BPP, int CELL>
int fw_launch(const uint8_t* src, int* state, uint8_t* mask, int N, int slot0, int Hs, int Ws,
              int GH, int GW, long long frame_bytes, int pitch, int row_step, int bg_shift,
              long long stride, hipStream_t s) {
  constexpr int VB = fw_vec_bytes(BPP, CELL);
  const int vec_ok = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)frame_bytes |
                       (uintptr_t)pitch) % VB) == 0;
  const dim3 grid((unsigned)((GW + kWave - 1) / kWave),
                  (unsigned)((GH + kFwRowsPerBlock - 1) / kFwRowsPerBlock), (unsigned)N);
  hipLaunchKernelGGL((frame_watch_cells_kernel<BPP, CELL>), grid,
                     dim3(kFwRowsPerBlock * kWave), 0, s, src, state, mask, slot0, Hs, Ws, GH, GW,
                     frame_bytes, pitch, row_step, bg_shift, stride, vec_ok);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}

}  // namespace
}  // namespace kvedge

using namespace kvedge;

extern "C" int kv_watch_state_stride(int cells) { return kFwHdr + 3 * cells; }

extern "C" int kv_frame_watch(const unsigned char* src, int* state, int* stats,
                              unsigned char* mask, int N, int S, int slot0, int Hs, int Ws,
                              int nv12, int cell, int row_step, int bg_shift, hipStream_t s) {
  if (Hs < 1 || Hs > kFwMaxExtent || Ws < 2 || Ws > kFwMaxExtent) return -1;
  if (N < 0 || S < 0 || slot0 < 0 || (long long)slot0 + N > S) return -2;
  if (cell != 8 && cell != 16 && cell != 32) return -3;
  if (row_step != 1 && row_step != 2 && row_step != 4) return -4;
  if (bg_shift < 0 || bg_shift > 8) return -5;
  if (nv12 && ((Hs | Ws) & 1)) return -6;
  if ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(stats)) & 3) return -7;
  if (N > 65535) return -9;  // grid z
  if (N == 0) return 0;
  const int GH = (Hs + cell - 1) / cell, GW = (Ws + cell - 1) / cell;
  const int C = GH * GW;
  const long long stride = kv_watch_state_stride(C);
  const int pitch = nv12 ? Ws : Ws * 3;
  const long long frame_bytes = nv12 ? (long long)(Hs * 3 / 2) * Ws : (long long)Hs * pitch;
#ifdef KVEDGE_CHECKS
  // NV12: only the Hs luma rows of the last frame are read, but the frames are whole
  if (!rs_in_alloc(src, (long long)N * frame_bytes)) return -20;
  if (!rs_in_alloc(state + (long long)slot0 * stride, (long long)N * stride * 4)) return -21;
  if (!rs_in_alloc(stats, (long long)N * 16 * 4)) return -22;
  if (!rs_in_alloc(mask, (long long)N * C)) return -23;
#endif
  int rc;
#define KV_FW(B, CL) \
  fw_launch<B, CL>(src, state, mask, N, slot0, Hs, Ws, GH, GW, frame_bytes, pitch, row_step, \
                   bg_shift, stride, s)
  if (nv12) rc = cell == 8 ? KV_FW(1, 8) : cell == 16 ? KV_FW(1, 16) : KV_FW(1, 32);
  else rc = cell == 8 ? KV_FW(3, 8) : cell == 16 ? KV_FW(3, 16) : KV_FW(3, 32);
#undef KV_FW
  if (rc) return rc;
  const int sampled_rows = (Hs + row_step - 1) / row_step;
  const long long P = (long long)sampled_rows * Ws, Q = (long long)sampled_rows * (Ws - GW);
  hipLaunchKernelGGL(frame_watch_totals_kernel, dim3((unsigned)N), dim3(kFwTotThreads), 0, s,
                     state, mask, stats, slot0, C, P, Q, stride);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}
