// K15 (ROI crop + resize): the seam of the detect-then-classify cascade.  For every image n
// and slot k < K it reads box row k of det[n] (kept NMS rows are ordered by score, so these
// are the top-K detections) from device memory, cuts that window out of the uint8 frame and
// stretches it to a D x D uint8 crop for the ResNet frames-in stem -- no host in the loop, so
// the whole cascade stays inside one captured graph.
//
// ROI geometry, per ROI on the device, from the float box (x1, y1, x2, y2) in frame pixels.
// The clamp is done in float first, so NaN and inf never reach a float -> int conversion
// (fmaxf(NaN, 0) = 0):
//   fx1 = fminf(fmaxf(x1, 0), Ws), fx2 likewise;  x0 = min((int)floorf(fx1), Ws - 1);
//   xe = min(max((int)ceilf(fx2), x0 + 1), Ws);  w = xe - x0;  the same for y.
// The window is therefore always >= 1 x 1 and inside the frame whatever the box holds
// (zero-area, inverted, out of range, non-finite): no source read leaves [0, Hs) x [0, Ws).
//
// Resample: exactly frame_resize of the window with the stretch axes (h, D, 0, 0, D) and
// (w, D, 0, 0, D) -- the same rs_tap, 11-bit fixed point and rounding (resample.h), so the
// crop is bit-identical to ops.reference.roi_crop.  Slots k >= min(max(count[n], 0), max_det)
// are filled with `pad`; every destination byte is written on every launch (a replayed graph
// must not show a stale crop).
//
// Launch shape: one workgroup per (ROI, band of BAND destination rows).  The box and the count
// are wave-uniform loads; the per-column tap table is built in LDS once per workgroup, followed
// by the kernel's only barrier, which every thread reaches -- an invalid slot takes the same
// path and only then writes `pad`.  Each thread makes 4 pixels = 12 bytes = three dword stores
// (D % 4 == 0 keeps every row 4-byte aligned).
#include "common.h"
#include "kvedge_kernels.h"
#include "resample.h"  // RsAxis, rs_tap, roi_window

namespace kvedge {
namespace {

constexpr int kRoiBlock = 256;
// destination rows per workgroup, from the probe's same-process alternation at b64, 1080p, K 4,
// D 224 (tools/roi_crop_probe.py, profiles/roi_crop_b64_1080p.json): ~600 px windows 0.095 /
// 0.096 / 0.103 / 0.117 ms for 4 / 8 / 16 / 32 rows, ~64 px windows 0.058-0.060 ms for all
// four.  4 and 8 tie within the run's spread; 8 builds half as many tap tables.
constexpr int kRoiBand = 8;

template <int BAND>
__global__ __launch_bounds__(kRoiBlock) void roi_crop_kernel(
    const uint8_t* __restrict__ src, const float* __restrict__ det, const int* __restrict__ count,
    uint8_t* __restrict__ dst, int Hs, int Ws, int max_det, int K, int D, unsigned pad,
    int bands_per_roi) {
  // per destination column: x = byte offsets of the two taps in a window row (q * 3 < 2^16,
  // low / high half), y = wx
  extern __shared__ __attribute__((aligned(16))) uint2 roi_col[];
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
  for (int x = threadIdx.x; x < D; x += kRoiBlock) {
    int q0, q1, wx;
    rs_tap(ax, x, q0, q1, wx);
    roi_col[x] = make_uint2((unsigned)(q0 * 3) | ((unsigned)(q1 * 3) << 16), (unsigned)wx);
  }
  __syncthreads();
  const unsigned pad4 = pad * 0x01010101u;
  const int W4 = D >> 2;
  const int items = BAND * W4;
  // 64-bit offsets: b512 at 1080p is past 2^31 bytes
  const uint8_t* win = src + (((long long)n * Hs + y0) * Ws + x0) * 3;
  uint8_t* crop = dst + (long long)roi * D * D * 3;
  const long long pitch = (long long)Ws * 3;
  for (int it = threadIdx.x; it < items; it += kRoiBlock) {
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
    rs_tap(ay, d, q0, q1, wy);  // q0, q1 < h: rows y0 + q < Hs
    const uint8_t* r0 = win + q0 * pitch;
    const uint8_t* r1 = win + q1 * pitch;
    unsigned px[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint2 c = roi_col[x4 * 4 + j];
      const int o0 = (int)(c.x & 0xffffu), o1 = (int)(c.x >> 16);  // taps < w: x0 + q < Ws
      const int wx = (int)c.y;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int top = (int)r0[o0 + ch] * (2048 - wx) + (int)r0[o1 + ch] * wx;
        const int bot = (int)r1[o0 + ch] * (2048 - wx) + (int)r1[o1 + ch] * wx;
        px[3 * j + ch] = (unsigned)((top * (2048 - wy) + bot * wy + (1 << 21)) >> 22);
      }
    }
    out[0] = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    out[1] = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
    out[2] = px[8] | (px[9] << 8) | (px[10] << 16) | (px[11] << 24);
  }
}

template <int BAND>
int roi_launch(const uint8_t* src, const float* det, const int* count, uint8_t* dst, int N, int Hs,
               int Ws, int max_det, int K, int D, int pad, hipStream_t s) {
  const int bands_per_roi = (D + BAND - 1) / BAND;
  const long long wgs = (long long)N * K * bands_per_roi;
  if (wgs >= (1ll << 31)) return -6;
  hipLaunchKernelGGL(roi_crop_kernel<BAND>, dim3((unsigned)wgs), dim3(kRoiBlock),
                     (unsigned)(D * sizeof(uint2)), s, src, det, count, dst, Hs, Ws, max_det, K, D,
                     (unsigned)pad, bands_per_roi);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}

}  // namespace
}  // namespace kvedge

using namespace kvedge;

extern "C" int kv_roi_crop_band(const uint8_t* src, const float* det, const int* count,
                                uint8_t* dst, int N, int Hs, int Ws, int max_det, int K, int D,
                                int pad, int band, hipStream_t s) {
  if (D % 4) return -1;
  if (Hs < 1 || Hs > kRsMaxExtent || Ws < 1 || Ws > kRsMaxExtent || D < 1 || D > kRsMaxExtent)
    return -2;
  if (K < 1 || K > max_det) return -3;
  if (pad < 0 || pad > 255) return -4;
  if (reinterpret_cast<uintptr_t>(dst) & 3) return -5;  // dword stores
  if (N < 0) return -6;
  if (N == 0) return 0;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(src, (long long)N * Hs * Ws * 3)) return -20;
  if (!rs_in_alloc(det, (long long)N * max_det * 6 * 4)) return -21;
  if (!rs_in_alloc(count, (long long)N * 4)) return -22;
  if (!rs_in_alloc(dst, (long long)N * K * D * D * 3)) return -23;
#endif
  switch (band ? band : kRoiBand) {
    case 4: return roi_launch<4>(src, det, count, dst, N, Hs, Ws, max_det, K, D, pad, s);
    case 8: return roi_launch<8>(src, det, count, dst, N, Hs, Ws, max_det, K, D, pad, s);
    case 16: return roi_launch<16>(src, det, count, dst, N, Hs, Ws, max_det, K, D, pad, s);
    case 32: return roi_launch<32>(src, det, count, dst, N, Hs, Ws, max_det, K, D, pad, s);
    default: return -7;
  }
}

extern "C" int kv_roi_crop(const uint8_t* src, const float* det, const int* count, uint8_t* dst,
                           int N, int Hs, int Ws, int max_det, int K, int D, int pad,
                           hipStream_t s) {
  return kv_roi_crop_band(src, det, count, dst, N, Hs, Ws, max_det, K, D, pad, 0, s);
}
