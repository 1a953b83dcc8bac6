// NV12 source taps for frame_nv12.hip (K16 / K17): where the chroma of a pixel lives and the
// integer BT.601 limited-range conversion of one (Y, U, V) tap to RGB.  The CPU reference
// (kvedge_amd/ops/reference.py nv12_to_rgb) computes exactly these integers.
//
// Layout of one Hs x Ws frame (Hs, Ws even), uint8 [Hs * 3 / 2][Ws]: rows 0 .. Hs - 1 are Y;
// row Hs + (y >> 1) holds, at bytes (x & ~1) and (x & ~1) + 1, the U and V of pixel (y, x)
// (nearest-neighbour chroma: one pair per 2 x 2 cell).
//   c = Y - 16, d = U - 128, e = V - 128
//   R = clamp((298 c         + 409 e + 128) >> 8, 0, 255)
//   G = clamp((298 c - 100 d - 208 e + 128) >> 8, 0, 255)
//   B = clamp((298 c + 516 d         + 128) >> 8, 0, 255)
// with >> the arithmetic shift of an int32; the sums lie in [-43756, 136882].
#pragma once
#include "common.h"

namespace kvedge {

// one tap: y_row / uv_row point at the tap's Y row and chroma row, q is its pixel column.
// The pair is one 16-bit load: uv_row and q & ~1 are even (even frame address, even Ws).
__device__ __forceinline__ void nv12_tap(const uint8_t* __restrict__ y_row,
                                         const uint8_t* __restrict__ uv_row, int q, int& r,
                                         int& g, int& b) {
  const int c = 298 * ((int)y_row[q] - 16) + 128;
  const unsigned uv = *reinterpret_cast<const uint16_t*>(uv_row + (q & ~1));
  const int d = (int)(uv & 0xffu) - 128, e = (int)(uv >> 8) - 128;
  r = min(max((c + 409 * e) >> 8, 0), 255);
  g = min(max((c - 100 * d - 208 * e) >> 8, 0), 255);
  b = min(max((c + 516 * d) >> 8, 0), 255);
}

}  // namespace kvedge
