// K24 (frame warp: per-camera ROI / rotation / lens dewarp / perspective) and K25 (view boxes
// back to source-frame pixels): the camera front end where one axis-aligned letterbox for the
// whole batch (K13) is not enough.  Every camera has its own view, a mesh of source positions
// in device memory (ops.CameraViews), so a view changes without recapturing the graph.
//
// Mesh int32 [streams, Hd/16 + 1, Wd/16 + 1, 2]: node (gy, gx) = the source position (x, y),
// in 1/64 pixel and pixel-corner coordinates (centre of pixel q = 64 q + 32), that destination
// corner point (16 gx, 16 gy) samples.  Destination pixel (dx, dy) of stream s, all integer:
//   cell (dx >> 4, dy >> 4), u = 2 (dx & 15) + 1, v = 2 (dy & 15) + 1 (pixel centre, 1/32 cell)
//   X = n00.x (32-u)(32-v) + n01.x u (32-v) + n10.x (32-u) v + n11.x u v   (2^-16 pixel; nodes
//       are clamped to [-2^20, 2^20), the weights sum to 1024: |X| <= 2^30), Y likewise
//   X < 0, X >= Ws << 16, Y < 0 or Y >= Hs << 16: the pixel is pad[s]
//   Xc = X - 32768, q = Xc >> 16, w = ((Xc & 0xffff) + 16) >> 5 in 0..2048;
//   q < 0 -> (0, w = 0); q >= S - 1 -> (S - 1, w = 0); second tap min(q + 1, S - 1)
// and K13's blend of the four taps.  NV12: each tap is converted first (nv12.h), so the result
// equals the RGB warp of the converted frame.  Bit-identical to ops.reference.frame_warp.
//
// Work split: one 256-thread workgroup per destination tile of 64 x 16 pixels (4 cells side
// by side), grid-striding over (camera, tile); thread t makes the 4 pixels at row t >> 4,
// columns 4 (t & 15) .. + 3 = 12 bytes = three dword stores (Wd % 16 == 0 keeps rows aligned;
// 4 pixels never straddle a cell, so the vertical half of the interpolation is done once per
// thread).  The tile's 5 x 2 nodes go to LDS once.
//
// The taps are gathered straight from global memory, as in K13.  A variant that staged each
// tile's source footprint (the bounding box of its nodes) in LDS first and gathered from there
// was measured at b64, 1080p -> 640 and was 1.4 .. 4 times slower on every mesh tried
// (profiles/frame_warp_b64_1080p_staged_ab.json, docs/kernels.md), so it was taken out.
#include "common.h"
#include "kvedge_kernels.h"
#include "nv12.h"      // nv12_rgb
#include "resample.h"  // kRsMaxExtent, rs_in_alloc

namespace kvedge {
namespace {

constexpr int kWpBlock = 256;
constexpr int kWpTileW = 64;   // destination pixels per tile row: 4 cells
constexpr int kWpCell = 16;    // destination pixels per mesh cell, and rows per tile
constexpr int kWpNodes = 10;   // 5 x 2 nodes per tile
constexpr int kWpNodeLim = 1 << 20;

// position -> taps and weight of one axis (P inside [0, S << 16))
__device__ __forceinline__ void wp_tap(int P, int S, int& q0, int& q1, int& w) {
  const int Pc = P - 32768;
  int q = Pc >> 16;
  w = ((Pc & 0xffff) + 16) >> 5;
  if (q < 0) {
    q = 0;
    w = 0;
  }
  if (q >= S - 1) {
    q = S - 1;
    w = 0;
  }
  q0 = q;
  q1 = w ? min(q + 1, S - 1) : q;  // a zero weight never reads its second tap
}

__device__ __forceinline__ unsigned wp_blend(const int (*t)[3], int ch, int wx, int wy) {
  const int top = t[0][ch] * (2048 - wx) + t[1][ch] * wx;
  const int bot = t[2][ch] * (2048 - wx) + t[3][ch] * wx;
  return (unsigned)((top * (2048 - wy) + bot * wy + (1 << 21)) >> 22);
}

__device__ __forceinline__ void wp_rgb(const uint8_t* p, int* t) {
  t[0] = p[0];
  t[1] = p[1];
  t[2] = p[2];
}

__device__ __forceinline__ unsigned wp_pair(const uint8_t* p) {
  return *reinterpret_cast<const uint16_t*>(p);
}

template <bool NV12>
__global__ __launch_bounds__(kWpBlock) void frame_warp_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int2* __restrict__ mesh,
    const int* __restrict__ pad, int Hs, int Ws, int Hd, int Wd, int slot0, int tiles_x,
    int tiles_per_img, long long n_tiles) {
  __shared__ int2 wp_node[kWpNodes];
  const int Gx = Wd / kWpCell + 1, Gy = Hd / kWpCell + 1;
  const int row = threadIdx.x >> 4, x4 = threadIdx.x & 15;
  const int pitch = NV12 ? Ws : Ws * 3;  // bytes per source row (NV12: of the Y and UV planes)
  const long long frame = NV12 ? (long long)(Hs >> 1) * 3 * Ws : (long long)Hs * Ws * 3;
  for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int n = (int)(tile / tiles_per_img);
    const int t = (int)(tile - (long long)n * tiles_per_img);
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const uint8_t* simg = src + (long long)n * frame;  // 64-bit: b512 at 1080p > 2^31 B
    __syncthreads();  // the previous tile's LDS reads are done
    if (threadIdx.x < kWpNodes) {
      // a tile past the last cell repeats the last node column
      const int r = threadIdx.x / 5;
      const int gx = min(tx * 4 + (int)threadIdx.x - r * 5, Gx - 1);
      int2 v = mesh[((long long)(slot0 + n) * Gy + ty + r) * Gx + gx];
      v.x = min(max(v.x, -kWpNodeLim), kWpNodeLim - 1);
      v.y = min(max(v.y, -kWpNodeLim), kWpNodeLim - 1);
      wp_node[threadIdx.x] = v;
    }
    __syncthreads();
    const int dx0 = tx * kWpTileW + x4 * 4;
    if (dx0 >= Wd) continue;  // the last tile of a row may hold 1 .. 3 cells
    const int dy = ty * kWpCell + row;
    const int c = x4 >> 2;
    const int2 n00 = wp_node[c], n01 = wp_node[c + 1], n10 = wp_node[5 + c], n11 = wp_node[6 + c];
    const int v = 2 * row + 1;
    const int lx = n00.x * (32 - v) + n10.x * v, ly = n00.y * (32 - v) + n10.y * v;
    const int rx = n01.x * (32 - v) + n11.x * v, ry = n01.y * (32 - v) + n11.y * v;
    const unsigned padv = (unsigned)pad[slot0 + n] & 0xffu;
    unsigned px[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int u = 2 * ((x4 & 3) * 4 + j) + 1;
      const int X = lx * (32 - u) + rx * u, Y = ly * (32 - u) + ry * u;
      if (X < 0 || X >= (Ws << 16) || Y < 0 || Y >= (Hs << 16)) {
        px[3 * j] = px[3 * j + 1] = px[3 * j + 2] = padv;
        continue;
      }
      int xa, xb, wx, ya, yb, wy;
      wp_tap(X, Ws, xa, xb, wx);
      wp_tap(Y, Hs, ya, yb, wy);
      int tp[4][3];  // taps a b / c d
      const uint8_t* p0 = simg + (long long)ya * pitch;
      const uint8_t* p1 = simg + (long long)yb * pitch;
      if (!NV12) {
        wp_rgb(p0 + xa * 3, tp[0]);
        wp_rgb(p0 + xb * 3, tp[1]);
        wp_rgb(p1 + xa * 3, tp[2]);
        wp_rgb(p1 + xb * 3, tp[3]);
      } else {
        // the pair of a tap: chroma row y >> 1, bytes x & ~1 and + 1 (one aligned 16-bit load:
        // frame address and Ws are even)
        const uint8_t* u0 = simg + (long long)(Hs + (ya >> 1)) * Ws;
        const uint8_t* u1 = simg + (long long)(Hs + (yb >> 1)) * Ws;
        const int ea = xa & ~1, eb = xb & ~1;
        nv12_rgb(p0[xa], wp_pair(u0 + ea), tp[0][0], tp[0][1], tp[0][2]);
        nv12_rgb(p0[xb], wp_pair(u0 + eb), tp[1][0], tp[1][1], tp[1][2]);
        nv12_rgb(p1[xa], wp_pair(u1 + ea), tp[2][0], tp[2][1], tp[2][2]);
        nv12_rgb(p1[xb], wp_pair(u1 + eb), tp[3][0], tp[3][1], tp[3][2]);
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) px[3 * j + ch] = wp_blend(tp, ch, wx, wy);
    }
    uint32_t* out = reinterpret_cast<uint32_t*>(dst + (long long)n * Hd * Wd * 3 +
                                                ((long long)dy * Wd + dx0) * 3);
    out[0] = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
    out[1] = px[4] | (px[5] << 8) | (px[6] << 16) | (px[7] << 24);
    out[2] = px[8] | (px[9] << 8) | (px[10] << 16) | (px[11] << 24);
  }
}

// the tracker's quantisation (track.hip): quarter pixels, fmaxf(NaN, 0) = 0
__device__ __forceinline__ int wp_quant(float x) {
  return (int)fminf(fmaxf(floorf(x * 4.f + 0.5f), 0.f), 16384.f);
}

// view point (px, py) in quarter pixels (1/64 cell) -> source position in 1/64 pixel
__device__ __forceinline__ void wp_point(const int2* __restrict__ m, int Gx, int cells_x,
                                         int cells_y, int px, int py, int& X, int& Y) {
  const int cx = min(px >> 6, cells_x - 1), cy = min(py >> 6, cells_y - 1);
  const int u = px - 64 * cx, v = py - 64 * cy;  // 0 .. 64
  const int2* p = m + (long long)cy * Gx + cx;
  const int2 nd[4] = {p[0], p[1], p[Gx], p[Gx + 1]};
  const long long w[4] = {(64 - u) * (64 - v), u * (64 - v), (64 - u) * v, u * v};  // sum 4096
  long long ax = 2048, ay = 2048;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ax += (long long)min(max(nd[i].x, -kWpNodeLim), kWpNodeLim - 1) * w[i];
    ay += (long long)min(max(nd[i].y, -kWpNodeLim), kWpNodeLim - 1) * w[i];
  }
  X = (int)(ax >> 12);  // |.| <= 2^20
  Y = (int)(ay >> 12);
}

// K25: one thread per (image, detection row)
__global__ __launch_bounds__(kWpBlock) void view_to_source_kernel(
    float* __restrict__ det, const int* __restrict__ count, const int2* __restrict__ mesh, int N,
    int max_det, int Hd, int Wd, float Hs, float Ws, int slot0) {
  const int total = N * max_det;
  const int cells_x = Wd / kWpCell, cells_y = Hd / kWpCell, Gx = cells_x + 1;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int n = i / max_det, r = i - n * max_det;
    if (r >= count[n]) continue;
    float2* p = reinterpret_cast<float2*>(det + (long long)i * 6);  // 24-B rows: 8-B aligned
    const float2 a = p[0], b = p[1];
    const int x1 = min(wp_quant(a.x), 4 * Wd), y1 = min(wp_quant(a.y), 4 * Hd);
    const int x2 = min(wp_quant(b.x), 4 * Wd), y2 = min(wp_quant(b.y), 4 * Hd);
    const int xm = (x1 + x2) >> 1, ym = (y1 + y2) >> 1;
    const int qx[8] = {x1, x2, x1, x2, xm, xm, x1, x2};
    const int qy[8] = {y1, y1, y2, y2, y1, y2, ym, ym};
    const int2* m = mesh + (long long)(slot0 + n) * (cells_y + 1) * Gx;
    int lox = INT_MAX, loy = INT_MAX, hix = INT_MIN, hiy = INT_MIN;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int X, Y;
      wp_point(m, Gx, cells_x, cells_y, qx[k], qy[k], X, Y);
      lox = min(lox, X);
      hix = max(hix, X);
      loy = min(loy, Y);
      hiy = max(hiy, Y);
    }
    // |.| <= 2^20 and a division by 64: exact in fp32
    p[0] = make_float2(fminf(fmaxf((float)lox / 64.f, 0.f), Ws),
                       fminf(fmaxf((float)loy / 64.f, 0.f), Hs));
    p[1] = make_float2(fminf(fmaxf((float)hix / 64.f, 0.f), Ws),
                       fminf(fmaxf((float)hiy / 64.f, 0.f), Hs));
  }
}

int wp_check(const void* dst, const int* mesh, const int* pad, int N, int Hs, int Ws, int Hd,
             int Wd, int streams, int gy, int gx, int slot0) {
  if (Hd % kWpCell || Wd % kWpCell) return -1;
  if (Hs < 1 || Hs > kRsMaxExtent || Ws < 1 || Ws > kRsMaxExtent || Hd < 1 ||
      Hd > kRsMaxExtent || Wd < 1 || Wd > kRsMaxExtent || N < 0)
    return -2;
  if (gy != Hd / kWpCell + 1 || gx != Wd / kWpCell + 1 || streams < 1) return -3;
  if (slot0 < 0 || (long long)slot0 + N > streams) return -4;
  if (reinterpret_cast<uintptr_t>(dst) & 3) return -5;  // dword stores
  if ((reinterpret_cast<uintptr_t>(mesh) & 7) || (reinterpret_cast<uintptr_t>(pad) & 3) ||
      !mesh || !pad)
    return -6;  // 8-B node loads
  return 0;
}

template <bool NV12>
int wp_launch(const uint8_t* src, uint8_t* dst, const int* mesh, const int* pad, int N, int Hs,
              int Ws, int Hd, int Wd, int streams, int gy, int gx, int slot0, hipStream_t s) {
  const int rc = wp_check(dst, mesh, pad, N, Hs, Ws, Hd, Wd, streams, gy, gx, slot0);
  if (rc) return rc;
  if (NV12 && ((Hs | Ws) & 1)) return -8;                       // 2 x 2 chroma cells
  if (NV12 && (reinterpret_cast<uintptr_t>(src) & 1)) return -9;  // 16-bit UV loads
  if (N == 0) return 0;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(src, (long long)N * Hs * Ws * (NV12 ? 3 : 6) / 2)) return -20;
  if (!rs_in_alloc(mesh, (long long)streams * gy * gx * 8)) return -21;
  if (!rs_in_alloc(pad, (long long)streams * 4)) return -22;
  if (!rs_in_alloc(dst, (long long)N * Hd * Wd * 3)) return -23;
#endif
  const int tiles_x = (Wd + kWpTileW - 1) / kWpTileW;
  const int tiles_per_img = tiles_x * (Hd / kWpCell);
  const long long n_tiles = (long long)N * tiles_per_img;
  const unsigned grid = (unsigned)(n_tiles < 2048 ? n_tiles : 2048);  // 256 CUs x 8, stride the rest
  hipLaunchKernelGGL(frame_warp_kernel<NV12>, dim3(grid), dim3(kWpBlock), 0, s, src, dst,
                     reinterpret_cast<const int2*>(mesh), pad, Hs, Ws, Hd, Wd, slot0, tiles_x,
                     tiles_per_img, n_tiles);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}

}  // namespace
}  // namespace kvedge

using namespace kvedge;

extern "C" int kv_frame_warp(const uint8_t* src, uint8_t* dst, const int* mesh, const int* pad,
                             int N, int Hs, int Ws, int Hd, int Wd, int streams, int gy, int gx,
                             int slot0, hipStream_t s) {
  return wp_launch<false>(src, dst, mesh, pad, N, Hs, Ws, Hd, Wd, streams, gy, gx, slot0, s);
}

extern "C" int kv_frame_warp_nv12(const uint8_t* src, uint8_t* dst, const int* mesh,
                                  const int* pad, int N, int Hs, int Ws, int Hd, int Wd,
                                  int streams, int gy, int gx, int slot0, hipStream_t s) {
  return wp_launch<true>(src, dst, mesh, pad, N, Hs, Ws, Hd, Wd, streams, gy, gx, slot0, s);
}

extern "C" int kv_view_to_source(float* det, const int* count, const int* mesh, int N, int max_det,
                                 int Hs, int Ws, int Hd, int Wd, int streams, int gy, int gx,
                                 int slot0, hipStream_t s) {
  if (max_det < 1) return -2;
  const int rc = wp_check(nullptr, mesh, count, N, Hs, Ws, Hd, Wd, streams, gy, gx, slot0);
  if (rc) return rc;
  const long long total = (long long)N * max_det;
  if (total >= (1ll << 31)) return -2;
  if (reinterpret_cast<uintptr_t>(det) & 7) return -5;  // 8-B row loads
  if (total == 0) return 0;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(det, total * 6 * 4)) return -20;
  if (!rs_in_alloc(mesh, (long long)streams * gy * gx * 8)) return -21;
  if (!rs_in_alloc(count, (long long)N * 4)) return -22;
#endif
  long long g = (total + kWpBlock - 1) / kWpBlock;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(view_to_source_kernel, dim3((unsigned)g), dim3(kWpBlock), 0, s, det, count,
                     reinterpret_cast<const int2*>(mesh), N, max_det, Hd, Wd, (float)Hs, (float)Ws,
                     slot0);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}
