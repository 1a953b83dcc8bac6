// K22 (snapshot annotation): draws what the device knows into the snapshot thumbnails, between
// frame_resize and jpeg_encode -- the outlines and cls:id labels of the boxes, and a mosaic over
// every box of a privacy class and over fixed privacy polygons -- in place, one launch, inside
// the captured step.
//
// images uint8 RGB [N,H,W,3] (W % 4 == 0: every row is whole dwords).  Image n is drawn in the
// style of camera slot0 + n, one int32 table row (kAnTab = 168 words, read only):
//   boxes @0 | labels @1 (bit 0: class, bit 1: id) | colour_by @2 (1 = track id) | thickness @3
//   | scale @4 | block @5 | max_draw @6 | n_polygons @7 | privacy class [8] @8 (-1 = unused)
//   | n_vertex [8] @16 | vertex [8][8][2] = (x, y) @24 | palette [16] @152 (R | G << 8 | B << 16)
// and one font table for all (88 words: glyph g of "0123456789:" in words 8 g .. 8 g + 6, one
// 5-bit row each, bit 4 = the left column).  Every word is clamped here whatever the table
// holds -- thickness 1..4, scale 1..2, block to 16 / 8 / 4 (>= 16, >= 8, else), max_draw 0..300,
// n_polygons and n_vertex 0..8 (fewer than 3 vertices = no polygon), palette index & 15, glyph
// <= 10 -- so no table content can index out of range; ops.AnnotateStyle range-checks where the
// table is built.  Vertices are the tracker's quarter pixels and MUST lie in 0..16384 (as in
// zones.hip: differences in int32, products in int64).
//
// The rules are written out in ops.reference.annotate, which this equals byte for byte.  Every
// output pixel is a function of the INPUT picture and the tables (a gather: no order between
// boxes to race on).  From the top: labels, the lowest row index first; outlines, the lowest row
// index first; the mosaic; the picture.
//   row r < count -> rectangle: q = the tracker's quantisation clamped to 4 Ws / 4 Hs,
//     x0 = min(q1 W / (4 Ws), W - 1), x1 = min(max(ceil(q2 W / (4 Ws)), x0 + 1), W), y alike:
//     every thumbnail pixel the box touches, never empty; products < 2^28.
//   privacy: the B x B block at (y / B, x / B), clipped at the image edge, is pixelated when it
//     meets the rectangle of any row r < count of a privacy class, or when the centre of one
//     of its pixels, ((2 x + 1) 2 Ws / W, (2 y + 1) 2 Hs / H) in quarter pixels, lies in a
//     polygon (the zones' crossing-number rule).  Every pixel of it becomes
//     (sum + cnt / 2) / cnt per channel over the block's cnt pixels of the input.
//   outline of r < min(count, max_draw), with `boxes`: the rectangle minus its inside
//     [x0 + t, x1 - t) x [y0 + t, y1 - t), in palette[(colour_by && id >= 0 ? id : cls) & 15].
//   label of the same rows: digits of cls, ':' when both parts show, digits of id % 100000 (id
//     and colon dropped while id < 0; nothing left = no label); [x0, x0 + s (6 chars + 1)) x
//     [y0, y0 + 9 s) clipped to the image, filled with the box colour; glyph k sits at
//     (s (1 + 6 k), s) and is black when (77 R + 150 G + 29 B) >> 8 >= 128, else white.
//
// Launch shape: ONE WORKGROUP OF 256 PER 64 x 16 TILE, one lane per 4 pixels of a row (12 bytes
// = 3 dwords).  Blocks are 4, 8 or 16 wide and tiles start on multiples of 64 / 16, so a block
// never straddles tiles and a workgroup reads and writes only its own tile: in place is safe
// without a halo.  (1) the table and the font go to LDS; a camera with nothing switched on
// leaves here.  (2) The lanes walk the count rows once and compact the rows that meet the tile
// into an LDS list (ballot + prefix popcount per wave, one LDS add per wave for the base): the
// rectangle, the label's end, colour, flags, text as 4-bit glyph numbers, and r -- the list is
// unordered, the compose step takes minima over r.  Room for all 300.  A tile no row and no
// polygon (by its bounding box) meets leaves here, having written nothing.  (3) Lanes mark the
// blocks under the privacy rectangles (one LDS flag per block) and test their own four pixel
// centres against the polygons.  (4) Lanes of flagged blocks add their 4-pixel channel sums
// into the block's three LDS counters.  (5) Each lane composes its four pixels against the list
// and stores its three dwords if anything touched them.  No atomics on global memory, no
// dependence between workgroups.
#include "common.h"
#include "kvedge_kernels.h"
#include "resample.h"  // rs_in_alloc

namespace kvedge {
namespace {

constexpr int kAnTileW = 64, kAnTileH = 16, kAnThreads = 256;
constexpr int kAnMaxDet = 300, kAnMax = 8, kAnTab = 168, kAnFont = 88;
constexpr int kAnMaxExtent = 8192, kAnMaxSrc = 4096;
constexpr int kAnBoxes = 0, kAnLabels = 1, kAnColourBy = 2, kAnThick = 3, kAnScale = 4,
              kAnBlock = 5, kAnMaxDraw = 6, kAnNPoly = 7, kAnPrivCls = 8, kAnNVert = 16,
              kAnVert = 24, kAnPalette = 152;
constexpr int kAnBlocks = (kAnTileW / 4) * (kAnTileH / 4);  // at B = 4
constexpr int kAnPriv = 1, kAnOutline = 2, kAnInkBlack = 4, kAnLabel = 8;  // entry flags << 24
constexpr int kAnNone = 0x7fffffff;

// the tracker's quantisation and class clamp (track.hip trk_q / trk_cls)
__device__ __forceinline__ int an_q(float x) {
  return (int)fminf(fmaxf(floorf(x * 4.f + 0.5f), 0.f), 16384.f);
}

__device__ __forceinline__ int an_cls(float c) {
  return (int)fminf(fmaxf(c, 0.f), 65535.f);
}

__device__ __forceinline__ int an_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// decimal digits of v <= 99999 as 4-bit glyph numbers, first digit at position nch
__device__ __forceinline__ int an_digits(unsigned v, unsigned long long& txt, int nch) {
  const int nd = v >= 10000 ? 5 : v >= 1000 ? 4 : v >= 100 ? 3 : v >= 10 ? 2 : 1;
  for (int i = nd - 1; i >= 0; --i) {
    txt |= (unsigned long long)(v % 10u) << (4 * (nch + i));
    v /= 10u;
  }
  return nch + nd;
}

__device__ __forceinline__ int an_byte(unsigned d0, unsigned d1, unsigned d2, int k) {
  const unsigned d = k < 4 ? d0 : k < 8 ? d1 : d2;
  return (int)((d >> (8 * (k & 3))) & 255u);
}

__global__ __launch_bounds__(kAnThreads) void annotate_kernel(
    uint8_t* __restrict__ images, const int* __restrict__ table, const int* __restrict__ font,
    const float* __restrict__ det, const int* __restrict__ count,
    const int* __restrict__ track_id, int H, int W, int Hs, int Ws, int slot0, int max_det) {
  __shared__ int s_tab[kAnTab];
  __shared__ int s_font[kAnFont];
  __shared__ int s_xy0[kAnMaxDet], s_xy1[kAnMaxDet], s_lab[kAnMaxDet], s_col[kAnMaxDet];
  __shared__ int s_t0[kAnMaxDet], s_t1[kAnMaxDet], s_r[kAnMaxDet];
  __shared__ int s_flag[kAnBlocks];
  __shared__ int s_sum[kAnBlocks * 3];
  __shared__ int s_n;

  const int tid = (int)threadIdx.x;
  const int lane = tid & (kWave - 1);
  const int n = (int)blockIdx.z;
  const int tx0 = (int)blockIdx.x * kAnTileW, ty0 = (int)blockIdx.y * kAnTileH;
  const int tx1 = min(tx0 + kAnTileW, W), ty1 = min(ty0 + kAnTileH, H);

  // (1) tables to LDS
  const int* tab = table + (long long)(slot0 + n) * kAnTab;
  if (tid < kAnTab) s_tab[tid] = tab[tid];
  if (tid < kAnFont) s_font[tid] = font[tid];
  if (tid < kAnBlocks) s_flag[tid] = 0;
  if (tid < kAnBlocks * 3) s_sum[tid] = 0;
  if (tid == 0) s_n = 0;
  __syncthreads();

  const bool boxes = s_tab[kAnBoxes] != 0;
  const int labels = s_tab[kAnLabels] & 3;
  const bool by_track = s_tab[kAnColourBy] == 1;
  const int t = an_clamp(s_tab[kAnThick], 1, 4);
  const int ssh = an_clamp(s_tab[kAnScale], 1, 2) - 1;  // glyph scale as a shift
  const int lb = s_tab[kAnBlock] >= 16 ? 4 : s_tab[kAnBlock] >= 8 ? 3 : 2;  // log2 B
  const int cnt = det ? min(max(count[n], 0), max_det) : 0;
  const int ndraw = (boxes || labels) ? min(cnt, an_clamp(s_tab[kAnMaxDraw], 0, kAnMaxDet)) : 0;
  bool any_priv = false;
#pragma unroll
  for (int k = 0; k < kAnMax; ++k) any_priv |= s_tab[kAnPrivCls + k] >= 0;
  const int n_poly = an_clamp(s_tab[kAnNPoly], 0, kAnMax);

  // polygons whose bounding box holds one of the tile's pixel centres (quarter pixels)
  unsigned poly_mask = 0;
  if (n_poly > 0) {
    const int cx_lo = (int)(((2u * tx0 + 1u) * 2u * Ws) / (unsigned)W);
    const int cx_hi = (int)(((2u * (tx1 - 1) + 1u) * 2u * Ws) / (unsigned)W);
    const int cy_lo = (int)(((2u * ty0 + 1u) * 2u * Hs) / (unsigned)H);
    const int cy_hi = (int)(((2u * (ty1 - 1) + 1u) * 2u * Hs) / (unsigned)H);
    for (int z = 0; z < n_poly; ++z) {
      const int nv = an_clamp(s_tab[kAnNVert + z], 0, kAnMax);
      if (nv < 3) continue;
      const int* v = s_tab + kAnVert + z * (2 * kAnMax);
      int x_lo = v[0], x_hi = v[0], y_lo = v[1], y_hi = v[1];
      for (int i = 1; i < nv; ++i) {
        x_lo = min(x_lo, v[2 * i]);
        x_hi = max(x_hi, v[2 * i]);
        y_lo = min(y_lo, v[2 * i + 1]);
        y_hi = max(y_hi, v[2 * i + 1]);
      }
      if (x_lo <= cx_hi && x_hi >= cx_lo && y_lo <= cy_hi && y_hi >= cy_lo) poly_mask |= 1u << z;
    }
  }
  if (!(cnt > 0 && any_priv) && ndraw == 0 && poly_mask == 0) return;  // uniform

  // (2) the rows that meet this tile
  const unsigned den_x = 4u * (unsigned)Ws, den_y = 4u * (unsigned)Hs;
  for (int base = 0; base < cnt; base += kAnThreads) {
    const int r = base + tid;
    bool push = false;
    int xy0 = 0, xy1 = 0, lab = 0, col = 0, t0 = 0, t1 = 0;
    if (r < cnt) {  // r < max_det: inside det[n]
      const float* p = det + ((long long)n * max_det + r) * 6;
      const unsigned qx0 = min((unsigned)an_q(p[0]), den_x), qy0 = min((unsigned)an_q(p[1]), den_y);
      const unsigned qx1 = min((unsigned)an_q(p[2]), den_x), qy1 = min((unsigned)an_q(p[3]), den_y);
      const int x0 = min((int)(qx0 * (unsigned)W / den_x), W - 1);
      const int y0 = min((int)(qy0 * (unsigned)H / den_y), H - 1);
      const int x1 = min(max((int)((qx1 * (unsigned)W + den_x - 1u) / den_x), x0 + 1), W);
      const int y1 = min(max((int)((qy1 * (unsigned)H + den_y - 1u) / den_y), y0 + 1), H);
      const int cls = an_cls(p[5]);
      const int id = track_id ? track_id[(long long)n * max_det + r] : -1;
      bool priv = false;
#pragma unroll
      for (int k = 0; k < kAnMax; ++k) priv |= s_tab[kAnPrivCls + k] == cls;  // cls >= 0
      const bool drawn = r < ndraw;
      const bool outline = drawn && boxes;
      unsigned long long txt = 0;
      int nch = 0;
      if (drawn) {
        if (labels & 1) nch = an_digits((unsigned)cls, txt, nch);
        if ((labels & 2) && id >= 0) {
          if (nch) txt |= 10ull << (4 * nch++);
          nch = an_digits((unsigned)id % 100000u, txt, nch);
        }
      }
      const int lx1 = nch ? min(x0 + ((6 * nch + 1) << ssh), W) : x0;
      const int ly1 = nch ? min(y0 + (9 << ssh), H) : y0;
      const int rgb = s_tab[kAnPalette + (((by_track && id >= 0) ? id : cls) & 15)] & 0xffffff;
      const int luma = (77 * (rgb & 255) + 150 * ((rgb >> 8) & 255) + 29 * ((rgb >> 16) & 255)) >> 8;
      const bool in_rect = x0 < tx1 && x1 > tx0 && y0 < ty1 && y1 > ty0;
      const bool in_lab = nch && x0 < tx1 && lx1 > tx0 && y0 < ty1 && ly1 > ty0;
      push = ((priv || outline) && in_rect) || in_lab;
      xy0 = x0 | (y0 << 16);
      xy1 = x1 | (y1 << 16);
      lab = lx1 | (ly1 << 16);
      col = rgb | ((priv ? kAnPriv : 0) | (outline ? kAnOutline : 0) |
                   (luma >= 128 ? kAnInkBlack : 0) | (nch ? kAnLabel : 0)) << 24;
      t0 = (int)(unsigned)txt;
      t1 = (int)(unsigned)(txt >> 32);
    }
    const unsigned long long m = __ballot(push);
    int at = 0;
    if (lane == 0 && m) at = atomicAdd(&s_n, __popcll(m));  // LDS; at most cnt <= 300 in all
    at = __shfl(at, 0, kWave) + __popcll(m & ((1ull << lane) - 1ull));
    if (push) {
      s_xy0[at] = xy0;
      s_xy1[at] = xy1;
      s_lab[at] = lab;
      s_col[at] = col;
      s_t0[at] = t0;
      s_t1[at] = t1;
      s_r[at] = r;
    }
  }
  __syncthreads();
  const int total = min(s_n, kAnMaxDet);
  if (total == 0 && poly_mask == 0) return;  // uniform: this tile stays as it is

  // this lane's four pixels
  const int lx = (tid & 15) * 4, ly = tid >> 4;
  const int x = tx0 + lx, y = ty0 + ly;
  const bool in_img = x < W && y < H;  // W % 4 == 0: all four or none
  unsigned* pix = reinterpret_cast<unsigned*>(images + (((long long)n * H + y) * W + x) * 3);
  unsigned d0 = 0, d1 = 0, d2 = 0;
  if (in_img) {
    d0 = pix[0];
    d1 = pix[1];
    d2 = pix[2];
  }
  const int bpr = kAnTileW >> lb;  // blocks per tile row
  const int blk = (ly >> lb) * bpr + (lx >> lb);

  // (3) blocks under privacy rectangles, and this lane's pixel centres against the polygons
  for (int e = tid; e < total; e += kAnThreads) {
    if (!((s_col[e] >> 24) & kAnPriv)) continue;
    const int ax0 = max(s_xy0[e] & 0xffff, tx0), ay0 = max(s_xy0[e] >> 16, ty0);
    const int ax1 = min(s_xy1[e] & 0xffff, tx1), ay1 = min(s_xy1[e] >> 16, ty1);
    if (ax0 >= ax1 || ay0 >= ay1) continue;  // only its label is here
    for (int by = (ay0 - ty0) >> lb; by <= (ay1 - 1 - ty0) >> lb; ++by)
      for (int bx = (ax0 - tx0) >> lb; bx <= (ax1 - 1 - tx0) >> lb; ++bx) s_flag[by * bpr + bx] = 1;
  }
  if (poly_mask && in_img) {
    const int py = (int)(((2u * y + 1u) * 2u * Hs) / (unsigned)H);
    int px[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) px[i] = (int)(((2u * (x + i) + 1u) * 2u * Ws) / (unsigned)W);
    bool hit = false;
    for (int z = 0; z < kAnMax; ++z) {
      if (!((poly_mask >> z) & 1u)) continue;
      const int nv = an_clamp(s_tab[kAnNVert + z], 0, kAnMax);
      const int* v = s_tab + kAnVert + z * (2 * kAnMax);
      bool in[4] = {false, false, false, false};
      int xj = v[2 * (nv - 1)], yj = v[2 * (nv - 1) + 1];
      for (int i = 0; i < nv; ++i) {
        const int xi = v[2 * i], yi = v[2 * i + 1];
        const int dx = xj - xi, dy = yj - yi;
        if ((yi > py) != (yj > py)) {  // dy != 0 here
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const long long c = (long long)dx * (py - yi) - (long long)(px[k] - xi) * dy;
            if (dy > 0 ? c > 0 : c < 0) in[k] = !in[k];
          }
        }
        xj = xi;
        yj = yi;
      }
      hit |= in[0] || in[1] || in[2] || in[3];
    }
    if (hit) s_flag[blk] = 1;
  }
  __syncthreads();

  // (4) channel sums of the flagged blocks
  const bool mosaic = in_img && s_flag[blk] != 0;
  if (mosaic) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      atomicAdd(&s_sum[blk * 3 + c], an_byte(d0, d1, d2, c) + an_byte(d0, d1, d2, 3 + c) +
                                         an_byte(d0, d1, d2, 6 + c) + an_byte(d0, d1, d2, 9 + c));
  }
  __syncthreads();
  if (!in_img) return;

  // (5) compose: the lowest row whose label / outline covers each pixel
  int best_l[4], best_o[4], e_l[4], e_o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    best_l[i] = best_o[i] = kAnNone;
    e_l[i] = e_o[i] = 0;
  }
  for (int e = 0; e < total; ++e) {
    const int xy0 = s_xy0[e], xy1 = s_xy1[e], lab = s_lab[e];
    const int fl = s_col[e] >> 24, r = s_r[e];
    const int x0 = xy0 & 0xffff, y0 = xy0 >> 16, x1 = xy1 & 0xffff, y1 = xy1 >> 16;
    const int lx1 = lab & 0xffff, ly1 = lab >> 16;
    if (y < y0 || (y >= y1 && y >= ly1)) continue;
    const bool row_l = (fl & kAnLabel) && y < ly1;
    const bool row_o = (fl & kAnOutline) && y < y1;
    const bool y_in = y >= y0 + t && y < y1 - t;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int xx = x + i;
      if (row_l && xx >= x0 && xx < lx1 && r < best_l[i]) {
        best_l[i] = r;
        e_l[i] = e;
      }
      if (row_o && xx >= x0 && xx < x1 && !(y_in && xx >= x0 + t && xx < x1 - t) &&
          r < best_o[i]) {
        best_o[i] = r;
        e_o[i] = e;
      }
    }
  }
  int mean[3] = {0, 0, 0};
  if (mosaic) {
    const int B = 1 << lb;
    const int bx0 = x & ~(B - 1), by0 = y & ~(B - 1);
    const unsigned area = (unsigned)((min(bx0 + B, W) - bx0) * (min(by0 + B, H) - by0));
#pragma unroll
    for (int c = 0; c < 3; ++c) mean[c] = (int)(((unsigned)s_sum[blk * 3 + c] + area / 2u) / area);
  }
  bool touched = mosaic;
  int o[12];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int rgb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = mosaic ? mean[c] : an_byte(d0, d1, d2, 3 * i + c);
    if (best_l[i] != kAnNone) {
      const int e = e_l[i];
      const int col = s_col[e];
      const int u = (x + i - (s_xy0[e] & 0xffff)) >> ssh, v = (y - (s_xy0[e] >> 16)) >> ssh;
      bool ink = false;
      if (u >= 1 && v >= 1 && v <= 7) {
        const int k = (u - 1) / 6, gx = (u - 1) - 6 * k;
        if (gx < 5 && k < 16) {
          const int g = min(((k < 8 ? s_t0[e] >> (4 * k) : s_t1[e] >> (4 * (k - 8))) & 15), 10);
          ink = (s_font[g * 8 + v - 1] >> (4 - gx)) & 1;
        }
      }
      const int inkv = ((col >> 24) & kAnInkBlack) ? 0 : 255;
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c] = ink ? inkv : (col >> (8 * c)) & 255;
      touched = true;
    } else if (best_o[i] != kAnNone) {
      const int col = s_col[e_o[i]];
#pragma unroll
      for (int c = 0; c < 3; ++c) rgb[c] = (col >> (8 * c)) & 255;
      touched = true;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[3 * i + c] = rgb[c];
  }
  if (touched) {
    pix[0] = (unsigned)(o[0] | o[1] << 8 | o[2] << 16) | (unsigned)o[3] << 24;
    pix[1] = (unsigned)(o[4] | o[5] << 8 | o[6] << 16) | (unsigned)o[7] << 24;
    pix[2] = (unsigned)(o[8] | o[9] << 8 | o[10] << 16) | (unsigned)o[11] << 24;
  }
}

}  // namespace
}  // namespace kvedge

using namespace kvedge;

extern "C" int kv_annotate_table_stride(void) { return kAnTab; }
extern "C" int kv_annotate_font_words(void) { return kAnFont; }

extern "C" int kv_annotate(unsigned char* images, const int* table, const int* font,
                           const float* det, const int* count, const int* track_id, int N, int S,
                           int slot0, int H, int W, int Hs, int Ws, int max_det, hipStream_t s) {
  if (H < 1 || H > kAnMaxExtent || W < 4 || W > kAnMaxExtent || W % 4) return -1;
  if (N < 0 || N > 65535 || S < 0 || slot0 < 0 || (long long)slot0 + N > S) return -2;
  if (det && (max_det < 1 || max_det > kAnMaxDet)) return -3;
  if (Hs < 1 || Hs > kAnMaxSrc || Ws < 1 || Ws > kAnMaxSrc) return -4;
  if (det ? !count : (count || track_id)) return -5;
  if ((reinterpret_cast<uintptr_t>(images) | reinterpret_cast<uintptr_t>(table) |
       reinterpret_cast<uintptr_t>(font) | reinterpret_cast<uintptr_t>(det) |
       reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(track_id)) & 3)
    return -7;  // dword accesses
  if (N == 0) return 0;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(images, (long long)N * H * W * 3)) return -20;
  if (!rs_in_alloc(table + (long long)slot0 * kAnTab, (long long)N * kAnTab * 4)) return -21;
  if (!rs_in_alloc(font, kAnFont * 4)) return -22;
  if (!rs_in_alloc(det, (long long)N * max_det * 6 * 4)) return -23;
  if (!rs_in_alloc(count, (long long)N * 4)) return -24;
  if (!rs_in_alloc(track_id, (long long)N * max_det * 4)) return -25;
#endif
  const dim3 grid((unsigned)((W + kAnTileW - 1) / kAnTileW), (unsigned)((H + kAnTileH - 1) / kAnTileH),
                  (unsigned)N);
  hipLaunchKernelGGL(annotate_kernel, grid, dim3(kAnThreads), 0, s, images, table, font, det, count,
                     track_id, H, W, Hs, Ws, slot0, det ? max_det : 0);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}
