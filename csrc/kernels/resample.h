// Fixed-point bilinear resample shared by frame_resize.hip (K13), roi_crop.hip (K15) and their
// NV12 forms in frame_nv12.hip (K16 / K17): one axis description, its tap / weight formula, the
// ROI window, the launchers' axis check and the bounds-check build's allocation probe.
// The formulas are documented at the top of frame_resize.hip; all kernels and the CPU
// reference (kvedge_amd/ops/reference.py _resize_axis) compute exactly these integers.
#pragma once
#include "common.h"

namespace kvedge {

constexpr int kRsMaxExtent = 8192;  // S, R <= 8192 keeps every product inside int32

// {source extent, extent of the virtual resized image, crop offset inside it, first
// destination index that holds content, number of content indices}
struct RsAxis {
  int S, R, off, c0, cn;
};

// taps and weight of destination index d; w = -1: d is padding
__device__ __forceinline__ void rs_tap(const RsAxis& a, int d, int& q0, int& q1, int& w) {
  if (d < a.c0 || d >= a.c0 + a.cn) {
    q0 = q1 = 0;
    w = -1;
    return;
  }
  const int v = d - a.c0 + a.off;
  const int num = (2 * v + 1) * a.S - a.R;
  const int den = 2 * a.R;
  int q = num >= 0 ? num / den : -((den - 1 - num) / den);  // floor
  const int r = num - q * den;
  w = (r * 2048 + a.R) / den;
  if (q < 0) {
    q = 0;
    w = 0;
  }
  if (q >= a.S - 1) {
    q = a.S - 1;
    w = 0;
  }
  q0 = q;
  // a zero weight never reads its second tap (b * 0): an exact integer ratio such as
  // 1080 -> 360 then touches one source line per destination line instead of two
  q1 = w ? min(q + 1, a.S - 1) : q;
}

// integer window [x0, x0 + w) of one ROI axis from the float box edges (lo, hi) in a frame of S
// (the geometry is documented at the top of roi_crop.hip)
__device__ __forceinline__ void roi_window(float lo, float hi, int S, int& x0, int& w) {
  const float fs = (float)S;
  const float flo = fminf(fmaxf(lo, 0.f), fs);
  const float fhi = fminf(fmaxf(hi, 0.f), fs);
  x0 = min((int)floorf(flo), S - 1);
  const int xe = min(max((int)ceilf(fhi), x0 + 1), S);
  w = xe - x0;
}

// launcher side: one axis tuple {S, R, off, c0, cn} against its source extent S and
// destination extent D
inline bool rs_axis_ok(const int* a, int S, int D) {
  return a[0] == S && a[0] >= 1 && a[0] <= kRsMaxExtent && a[1] >= 1 && a[1] <= kRsMaxExtent &&
         a[2] >= 0 && a[3] >= 0 && a[4] >= 0 && a[3] + a[4] <= D && a[2] + a[4] <= a[1];
}

#ifdef KVEDGE_CHECKS
// bounds-check build: operand extents against their HIP allocations (as kv_conv_check_extents)
inline bool rs_in_alloc(const void* ptr, long long bytes) {
  if (!ptr || bytes <= 0) return true;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)ptr) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  const char* b = static_cast<const char*>(base);
  const char* q = static_cast<const char*>(ptr);
  return q >= b && q + bytes <= b + size;
}
#endif

}  // namespace kvedge
