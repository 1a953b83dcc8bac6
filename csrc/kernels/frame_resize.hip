// K13 (frame resize: letterbox / resize + centre-crop) and K14 (detections back to
// source-frame pixels): the front end between native-resolution camera frames and the
// model-size uint8 frame buffer the frames-in stems read.
//
// The resample is bilinear with half-pixel centres (align_corners = False, no antialias) in
// 11-bit fixed point, integer from end to end, so the result is bit-identical to the CPU
// reference (kvedge_amd/ops/reference.py frame_resize) and from launch to launch.  Per axis
// {S, R, off, c0, cn} and destination index d inside the content [c0, c0 + cn):
//   v = d - c0 + off, num = (2v + 1) S - R, q = floor(num / 2R), r = num - q 2R,
//   w = (r 2048 + R) / 2R; q < 0 -> (0, w = 0); q >= S - 1 -> (S - 1, w = 0);
//   second tap min(q + 1, S - 1).
// Per channel, taps a b / c d: top = a (2048 - wx) + b wx, bot = c (2048 - wx) + d wx,
// out = (top (2048 - wy) + bot wy + 2^21) >> 22.  With S, R <= 8192 everything fits int32.
//
// Memory-bound and byte-granular: one workgroup per (image, band of kRsBand destination
// rows), grid-striding the bands; the per-column (tap offsets, wx) table is built in LDS once
// per workgroup; each thread makes 4 destination pixels = 12 bytes = three dword stores
// (Wd % 4 == 0 keeps every row 4-byte aligned).  Padding is written by the same threads, so
// every destination byte is written on every launch.
#include "common.h"
#include "kvedge_kernels.h"
#include "resample.h"  // RsAxis, rs_tap, rs_axis_ok

namespace kvedge {
namespace {

constexpr int kRsBlock = 256;
constexpr int kRsBand = 8;       // destination rows per workgroup step
constexpr unsigned kRsPadCol = 0xffffffffu;

__global__ __launch_bounds__(kRsBlock) void frame_resize_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int Hs, int Ws, int Hd, int Wd,
    RsAxis ay, RsAxis ax, unsigned pad, int bands_per_img, long long n_bands) {
  // per destination column: x = byte offsets of the two taps in a source row (q * 3 < 2^16,
  // low / high half), y = wx (kRsPadCol: padding)
  extern __shared__ __attribute__((aligned(16))) uint2 rs_col[];
  for (int x = threadIdx.x; x < Wd; x += kRsBlock) {
    int q0, q1, w;
    rs_tap(ax, x, q0, q1, w);
    rs_col[x] = make_uint2((unsigned)(q0 * 3) | ((unsigned)(q1 * 3) << 16),
                           w < 0 ? kRsPadCol : (unsigned)w);
  }
  __syncthreads();
  const unsigned pad4 = pad * 0x01010101u;
  const int W4 = Wd >> 2;
  const int items = kRsBand * W4;
  for (long long band = blockIdx.x; band < n_bands; band += gridDim.x) {
    const int n = (int)(band / bands_per_img);
    const int d0 = (int)(band - (long long)n * bands_per_img) * kRsBand;
    const uint8_t* simg = src + (long long)n * Hs * Ws * 3;  // 64-bit: b512 at 1080p > 2^31 B
    uint8_t* dimg = dst + (long long)n * Hd * Wd * 3;
    for (int it = threadIdx.x; it < items; it += kRsBlock) {
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
      const uint8_t* r0 = simg + (long long)y0 * Ws * 3;
      const uint8_t* r1 = simg + (long long)y1 * Ws * 3;
      unsigned px[12];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint2 c = rs_col[x4 * 4 + j];
        if (c.y == kRsPadCol) {
          px[3 * j] = px[3 * j + 1] = px[3 * j + 2] = pad;
          continue;
        }
        const int o0 = (int)(c.x & 0xffffu), o1 = (int)(c.x >> 16);
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
}

// K14: one thread per (image, detection row)
__global__ __launch_bounds__(kRsBlock) void det_to_source_kernel(float* __restrict__ det,
                                                                 const int* __restrict__ count,
                                                                 int N, int max_det, float cy,
                                                                 float sy, float cx, float sx,
                                                                 float Hs, float Ws) {
  const int total = N * max_det;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int n = i / max_det, r = i - n * max_det;
    if (r >= count[n]) continue;
    float2* p = reinterpret_cast<float2*>(det + (long long)i * 6);  // 24-B rows: 8-B aligned
    float2 a = p[0], b = p[1];
    a.x = fminf(fmaxf((a.x - cx) * sx, 0.f), Ws);
    a.y = fminf(fmaxf((a.y - cy) * sy, 0.f), Hs);
    b.x = fminf(fmaxf((b.x - cx) * sx, 0.f), Ws);
    b.y = fminf(fmaxf((b.y - cy) * sy, 0.f), Hs);
    p[0] = a;
    p[1] = b;
  }
}

}  // namespace
}  // namespace kvedge

using namespace kvedge;

extern "C" int kv_frame_resize(const uint8_t* src, uint8_t* dst, int N, int Hs, int Ws, int Hd,
                               int Wd, const int* axis_y, const int* axis_x, int pad,
                               hipStream_t s) {
  if (Wd % 4) return -1;
  if (Hs < 1 || Hs > kRsMaxExtent || Ws < 1 || Ws > kRsMaxExtent || Hd < 1 ||
      Hd > kRsMaxExtent || Wd < 1 || Wd > kRsMaxExtent || N < 0)
    return -2;
  if (!rs_axis_ok(axis_y, Hs, Hd) || !rs_axis_ok(axis_x, Ws, Wd)) return -3;
  if (pad < 0 || pad > 255) return -4;
  if (reinterpret_cast<uintptr_t>(dst) & 3) return -5;  // dword stores
  if (N == 0) return 0;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(src, (long long)N * Hs * Ws * 3)) return -20;
  if (!rs_in_alloc(dst, (long long)N * Hd * Wd * 3)) return -23;
#endif
  const int bands_per_img = (Hd + kRsBand - 1) / kRsBand;
  const long long n_bands = (long long)N * bands_per_img;
  const unsigned grid = (unsigned)(n_bands < 2048 ? n_bands : 2048);  // 256 CUs x 8, stride the rest
  const RsAxis ay{axis_y[0], axis_y[1], axis_y[2], axis_y[3], axis_y[4]};
  const RsAxis ax{axis_x[0], axis_x[1], axis_x[2], axis_x[3], axis_x[4]};
  hipLaunchKernelGGL(frame_resize_kernel, dim3(grid), dim3(kRsBlock),
                     (unsigned)(Wd * sizeof(uint2)), s, src, dst, Hs, Ws, Hd, Wd, ay, ax,
                     (unsigned)pad, bands_per_img, n_bands);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}

extern "C" int kv_det_to_source(float* det, const int* count, int N, int max_det, float cy,
                                float sy, float cx, float sx, int Hs, int Ws, hipStream_t s) {
  if (N < 0 || max_det < 1 || Hs < 1 || Ws < 1) return -1;
  const long long total = (long long)N * max_det;
  if (total >= (1ll << 31)) return -2;
  if (reinterpret_cast<uintptr_t>(det) & 7) return -5;  // 8-B row loads
  if (total == 0) return 0;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(det, total * 6 * 4)) return -20;
  if (!rs_in_alloc(count, (long long)N * 4)) return -21;
#endif
  long long g = (total + kRsBlock - 1) / kRsBlock;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(det_to_source_kernel, dim3((unsigned)g), dim3(kRsBlock), 0, s, det, count, N,
                     max_det, cy, sy, cx, sx, (float)Hs, (float)Ws);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}
