// K16 (frame resize from NV12) and K17 (ROI crop from NV12): K13 and K15 reading the frame as
// cameras and video decoders deliver it -- a full-resolution Y plane followed by a
// half-resolution interleaved UV plane, 1.5 bytes per pixel (layout and colour: nv12.h) -- so
// a native batch is half the bytes of packed RGB through the ring and over PCIe, and no RGB
// copy of the native frame is ever written.
//
// Order: each of the four source taps is converted to RGB (integer BT.601 limited range,
// nearest-neighbour chroma), then the taps are blended with exactly K13's 11-bit fixed-point
// bilinear (resample.h).  Hence, byte for byte,
//   frame_resize_nv12(f, plan) == frame_resize(nv12_to_rgb(f), plan)
//   roi_crop_nv12(f, det, ..)  == roi_crop(nv12_to_rgb(f), det, ..)
// which is what the tests check against the CPU reference.
//
// Launch shapes are K13's and K15's: one workgroup per (image, band of destination rows),
// grid-striding the bands, resp. one per (ROI, band); the per-column tap table is built in LDS
// once per workgroup and holds pixel columns (not byte offsets: Y and UV index differently);
// each thread makes 4 destination pixels = three dword stores; padding and invalid slots are
// written by the same threads, so every destination byte is written on every launch.  Per tap
// one Y byte and one 16-bit UV pair are loaded: 8 loads per destination pixel against the RGB
// kernels' 12.  The chroma cell of a tap comes from its absolute frame coordinate -- for a crop
// window with an odd origin, (x0 + q) & ~1 and (y0 + q) >> 1, never the window-relative one.
#include "common.h"
#include "kvedge_kernels.h"
#include "nv12.h"      // nv12_tap
#include "resample.h"  // RsAxis, rs_tap, roi_window, rs_axis_ok

namespace kvedge {
namespace {

constexpr int kNvBlock = 256;
constexpr int kNvBand = 8;     // destination rows per workgroup step (K13's)
constexpr int kNvRoiBand = 8;  // K15's built-in band
constexpr unsigned kNvPadCol = 0xffffffffu;

// 4 destination pixels of one destination row: taps of rows ya / yb (Y) and ua / ub (their
// chroma rows), columns and wx from the LDS table `col` (x = q0 | q1 << 16, y = wx or
// kNvPadCol), blended with wy; three dword stores
__device__ __forceinline__ void nv12_quad(const uint8_t* __restrict__ ya,
                                          const uint8_t* __restrict__ yb,
                                          const uint8_t* __restrict__ ua,
                                          const uint8_t* __restrict__ ub, const uint2* col, int wy,
                                          unsigned pad, uint32_t* __restrict__ out) {
  unsigned px[12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint2 c = col[j];
    if (c.y == kNvPadCol) {
      px[3 * j] = px[3 * j + 1] = px[3 * j + 2] = pad;
      continue;
    }
    const int q0 = (int)(c.x & 0xffffu), q1 = (int)(c.x >> 16);
    const int wx = (int)c.y;
    int t[4][3];  // taps a b / c d
    nv12_tap(ya, ua, q0, t[0][0], t[0][1], t[0][2]);
    nv12_tap(ya, ua, q1, t[1][0], t[1][1], t[1][2]);
    nv12_tap(yb, ub, q0, t[2][0], t[2][1], t[2][2]);
    nv12_tap(yb, ub, q1, t[3][0], t[3][1], t[3][2]);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int top = t[0][ch] * (2048 - wx) + t[1][ch] * wx;
      const int bot = t[2][ch] * (2048 - wx) + t[3][ch] * wx;
      px[3 * j + ch] = (unsigned)((top * (2048 - wy) + bot * wy + (1 << 21)) >> 22);
    }
  }
  out[0] = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
  out[1] = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
  out[2] = px[8] | (px[9] << 8) | (px[10] << 16) | (px[11] << 24);
}

__global__ __launch_bounds__(kNvBlock) void frame_resize_nv12_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int Hs, int Ws, int Hd, int Wd,
    RsAxis ay, RsAxis ax, unsigned pad, int bands_per_img, long long n_bands) {
  // per destination column: x = pixel columns of the two taps (< 2^13, low / high half),
  // y = wx (kNvPadCol: padding)
  extern __shared__ __attribute__((aligned(16))) uint2 nv_col[];
  for (int x = threadIdx.x; x < Wd; x += kNvBlock) {
    int q0, q1, w;
    rs_tap(ax, x, q0, q1, w);
    nv_col[x] = make_uint2((unsigned)q0 | ((unsigned)q1 << 16), w < 0 ? kNvPadCol : (unsigned)w);
  }
  __syncthreads();
  const unsigned pad4 = pad * 0x01010101u;
  const int W4 = Wd >> 2;
  const int items = kNvBand * W4;
  const long long frame = (long long)(Hs >> 1) * 3 * Ws;  // Hs * Ws * 3 / 2, Hs even
  for (long long band = blockIdx.x; band < n_bands; band += gridDim.x) {
    const int n = (int)(band / bands_per_img);
    const int d0 = (int)(band - (long long)n * bands_per_img) * kNvBand;
    const uint8_t* simg = src + (long long)n * frame;  // 64-bit: b1024 at 1080p > 2^31 B
    uint8_t* dimg = dst + (long long)n * Hd * Wd * 3;
    for (int it = threadIdx.x; it < items; it += kNvBlock) {
      const int row = it / W4, x4 = it - row * W4;
      const int d = d0 + row;
      if (d >= Hd) break;  // rows only grow with it
      uint32_t* out = reinterpret_cast<uint32_t*>(dimg + ((long long)d * Wd + x4 * 4) * 3);
      int y0, y1, wy;
      rs_tap(ay, d, y0, y1, wy);
      if (wy < 0) {
        out[0] = pad4;
        out[1] = pad4;
        out[2] = pad4;
        continue;
      }
      // y < Hs: Y row y, chroma row Hs + (y >> 1) <= Hs + Hs / 2 - 1
      nv12_quad(simg + (long long)y0 * Ws, simg + (long long)y1 * Ws,
                simg + (long long)(Hs + (y0 >> 1)) * Ws, simg + (long long)(Hs + (y1 >> 1)) * Ws,
                nv_col + x4 * 4, wy, pad, out);
    }
  }
}

template <int BAND>
__global__ __launch_bounds__(kNvBlock) void roi_crop_nv12_kernel(
    const uint8_t* __restrict__ src, const float* __restrict__ det, const int* __restrict__ count,
    uint8_t* __restrict__ dst, int Hs, int Ws, int max_det, int K, int D, unsigned pad,
    int bands_per_roi) {
  // per destination column: x = frame columns x0 + q of the two taps (< 2^13, low / high
  // half), y = wx
  extern __shared__ __attribute__((aligned(16))) uint2 nv_roi_col[];
  const int roi = (int)(blockIdx.x / (unsigned)bands_per_roi);
  const int d0 = (int)(blockIdx.x - (unsigned)roi * (unsigned)bands_per_roi) * BAND;
  const int n = roi / K, k = roi - n * K;
  // wave-uniform: the compiler keeps these in scalar registers
  const bool valid = k < min(max(count[n], 0), max_det);
  const float* box = det + ((long long)n * max_det + k) * 6;  // k < K <= max_det: in bounds
  int x0, y0, w, h;
  roi_window(box[0], box[2], Ws, x0, w);
  roi_window(box[1], box[3], Hs, y0, h);
  const RsAxis ax{w, D, 0, 0, D}, ay{h, D, 0, 0, D};
  for (int x = threadIdx.x; x < D; x += kNvBlock) {
    int q0, q1, wx;
    rs_tap(ax, x, q0, q1, wx);  // taps < w: x0 + q < Ws
    nv_roi_col[x] = make_uint2((unsigned)(x0 + q0) | ((unsigned)(x0 + q1) << 16), (unsigned)wx);
  }
  __syncthreads();
  const unsigned pad4 = pad * 0x01010101u;
  const int W4 = D >> 2;
  const int items = BAND * W4;
  // 64-bit offsets; frame stride Hs * Ws * 3 / 2, Hs even
  const uint8_t* simg = src + (long long)n * ((long long)(Hs >> 1) * 3 * Ws);
  uint8_t* crop = dst + (long long)roi * D * D * 3;
  for (int it = threadIdx.x; it < items; it += kNvBlock) {
    const int row = it / W4, x4 = it - row * W4;
    const int d = d0 + row;
    if (d >= D) break;  // rows only grow with it
    uint32_t* out = reinterpret_cast<uint32_t*>(crop + ((long long)d * D + x4 * 4) * 3);
    if (!valid) {
      out[0] = pad4;
      out[1] = pad4;
      out[2] = pad4;
      continue;
    }
    int q0, q1, wy;
    rs_tap(ay, d, q0, q1, wy);  // q0, q1 < h: frame rows y0 + q < Hs
    const int ya = y0 + q0, yb = y0 + q1;
    nv12_quad(simg + (long long)ya * Ws, simg + (long long)yb * Ws,
              simg + (long long)(Hs + (ya >> 1)) * Ws, simg + (long long)(Hs + (yb >> 1)) * Ws,
              nv_roi_col + x4 * 4, wy, pad, out);
  }
}

template <int BAND>
int roi_nv12_launch(const uint8_t* src, const float* det, const int* count, uint8_t* dst, int N,
                    int Hs, int Ws, int max_det, int K, int D, int pad, hipStream_t s) {
  const int bands_per_roi = (D + BAND - 1) / BAND;
  const long long wgs = (long long)N * K * bands_per_roi;
  if (wgs >= (1ll << 31)) return -6;
  hipLaunchKernelGGL(roi_crop_nv12_kernel<BAND>, dim3((unsigned)wgs), dim3(kNvBlock),
                     (unsigned)(D * sizeof(uint2)), s, src, det, count, dst, Hs, Ws, max_det, K, D,
                     (unsigned)pad, bands_per_roi);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}

}  // namespace
}  // namespace kvedge

using namespace kvedge;

extern "C" int kv_frame_resize_nv12(const uint8_t* src, uint8_t* dst, int N, int Hs, int Ws,
                                    int Hd, int Wd, const int* axis_y, const int* axis_x, int pad,
                                    hipStream_t s) {
  if (Wd % 4) return -1;
  if (Hs < 1 || Hs > kRsMaxExtent || Ws < 1 || Ws > kRsMaxExtent || Hd < 1 ||
      Hd > kRsMaxExtent || Wd < 1 || Wd > kRsMaxExtent || N < 0)
    return -2;
  if (!rs_axis_ok(axis_y, Hs, Hd) || !rs_axis_ok(axis_x, Ws, Wd)) return -3;
  if (pad < 0 || pad > 255) return -4;
  if (reinterpret_cast<uintptr_t>(dst) & 3) return -5;  // dword stores
  if ((Hs | Ws) & 1) return -8;                         // 2 x 2 chroma cells
  if (reinterpret_cast<uintptr_t>(src) & 1) return -9;  // 16-bit UV loads
  if (N == 0) return 0;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(src, (long long)N * Hs * Ws * 3 / 2)) return -20;
  if (!rs_in_alloc(dst, (long long)N * Hd * Wd * 3)) return -23;
#endif
  const int bands_per_img = (Hd + kNvBand - 1) / kNvBand;
  const long long n_bands = (long long)N * bands_per_img;
  const unsigned grid = (unsigned)(n_bands < 2048 ? n_bands : 2048);  // 256 CUs x 8, stride the rest
  const RsAxis ay{axis_y[0], axis_y[1], axis_y[2], axis_y[3], axis_y[4]};
  const RsAxis ax{axis_x[0], axis_x[1], axis_x[2], axis_x[3], axis_x[4]};
  hipLaunchKernelGGL(frame_resize_nv12_kernel, dim3(grid), dim3(kNvBlock),
                     (unsigned)(Wd * sizeof(uint2)), s, src, dst, Hs, Ws, Hd, Wd, ay, ax,
                     (unsigned)pad, bands_per_img, n_bands);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}

extern "C" int kv_roi_crop_nv12_band(const uint8_t* src, const float* det, const int* count,
                                     uint8_t* dst, int N, int Hs, int Ws, int max_det, int K,
                                     int D, int pad, int band, hipStream_t s) {
  if (D % 4) return -1;
  if (Hs < 1 || Hs > kRsMaxExtent || Ws < 1 || Ws > kRsMaxExtent || D < 1 || D > kRsMaxExtent)
    return -2;
  if (K < 1 || K > max_det) return -3;
  if (pad < 0 || pad > 255) return -4;
  if (reinterpret_cast<uintptr_t>(dst) & 3) return -5;  // dword stores
  if (N < 0) return -6;
  if ((Hs | Ws) & 1) return -8;                         // 2 x 2 chroma cells
  if (reinterpret_cast<uintptr_t>(src) & 1) return -9;  // 16-bit UV loads
  if (N == 0) return 0;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(src, (long long)N * Hs * Ws * 3 / 2)) return -20;
  if (!rs_in_alloc(det, (long long)N * max_det * 6 * 4)) return -21;
  if (!rs_in_alloc(count, (long long)N * 4)) return -22;
  if (!rs_in_alloc(dst, (long long)N * K * D * D * 3)) return -23;
#endif
  switch (band ? band : kNvRoiBand) {
    case 4: return roi_nv12_launch<4>(src, det, count, dst, N, Hs, Ws, max_det, K, D, pad, s);
    case 8: return roi_nv12_launch<8>(src, det, count, dst, N, Hs, Ws, max_det, K, D, pad, s);
    case 16: return roi_nv12_launch<16>(src, det, count, dst, N, Hs, Ws, max_det, K, D, pad, s);
    case 32: return roi_nv12_launch<32>(src, det, count, dst, N, Hs, Ws, max_det, K, D, pad, s);
    default: return -7;
  }
}

extern "C" int kv_roi_crop_nv12(const uint8_t* src, const float* det, const int* count,
                                uint8_t* dst, int N, int Hs, int Ws, int max_det, int K, int D,
                                int pad, hipStream_t s) {
  return kv_roi_crop_nv12_band(src, det, count, dst, N, Hs, Ws, max_det, K, D, pad, 0, s);
}
