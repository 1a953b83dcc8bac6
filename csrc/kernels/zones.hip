// K19 (lines and zones): turns the tracker's stable ids into counts -- how many tracks crossed
// a virtual line, in which direction, and how many are inside a polygon zone, for how long.
// It runs right after K18 (track.hip) on the tracker state in device memory, inside the
// captured step, no host sync.
//
// One batch row = one camera ("stream").  Per stream, in ints:
//   zone state (kZnStride(T) = 4 T + 48 of them), T = 64 * TJ the tracker's slots:
//     entry [T][4] = (seen_id, ax, ay, zmask): the confirmed track id this entry describes
//       (-1 = none), its anchor at the last sighting (quarter pixels), bit z set when that
//       anchor was inside zone z
//     | line_fwd [8] | line_back [8] | zone_enter [8] | zone_exit [8] | zone_occ [8]
//     | zone_dwell [8]     cumulative int32, wrapping modulo 2^32 (zone_occ: current value)
//   region table (kZnTab = 188 of them, read only):
//     line [8][4] = (ax, ay, bx, by)  @0   | line_cls [8] @32 (-1 = any class)
//     | vertex [8][8][2] = (x, y)     @40  | n_vertex [8] @168 | zone_cls [8] @176
//     | n_lines  n_zones  anchor  0   @184
//   Coordinates are quarter pixels and MUST lie in 0..16384 (ops.ZoneSet quantises and clamps
//   them): differences are taken in int32 before the int64 products, so a hand-written table
//   with larger words is outside the contract (no out-of-range access, but not the reference).
//   n_lines / n_zones / n_vertex are clamped to 0..8 here whatever the table holds (fewer than
//   3 vertices = an empty zone; anchor 1 = centre, anything else = bottom-centre), so no table
//   content can index out of range; ops.ZoneSet range-checks them where the table is built.
//
// Everything after the tracker's quantisation q(x) = (int) min(max(floor(x * 4 + 0.5), 0), 16384)
// is integer arithmetic, every product int64, no divide, no float compare, so the result is
// bit-identical to ops.reference.zone_update, where the rules are written out:
//   anchor of a box: ((x1 + x2) >> 1, y2) (bottom-centre, mode 0) or ((x1 + x2) >> 1,
//     (y1 + y2) >> 1) (centre, mode 1);
//   point in polygon: crossing number; the edge (xi, yi) -> (xj, yj) toggles when
//     (yi > py) != (yj > py) and t = (xj - xi) (py - yi) - (px - xi) (yj - yi) has the sign of
//     yj - yi (px strictly left of the edge);
//   the move P0 -> P1 crosses A -> B when side(P0) != side(P1), side(P) = cross(B - A, P - A) >= 0,
//     and sp(A) != sp(B), sp(X) = cross(P1 - P0, X - P0) >= 0: both tests half-open, so a path
//     through the shared end point of two chained segments counts on exactly one of them;
//     side(P0) && !side(P1) is "forward"; A == B has side() true everywhere and never counts.
//
// One update per slot, cur = (hits > 0 && id >= 0) ? id : -1 read from the tracker:
//   seen_id != cur, seen_id >= 0: the track is gone or the slot was reused -> zone_exit for
//     every bit of zmask, entry cleared to (-1, 0, 0, 0);
//   cur >= 0, age == 0 (seen this frame): P1 = anchor(box), m1 = zones holding P1 whose class
//     passes;  seen_id == cur: every class-passing line is tested with P0 = (ax, ay),
//     zone_enter gets m1 & ~zmask, zone_exit gets zmask & ~m1;  otherwise (first sighting)
//     zone_enter gets m1 and no line is tested;  entry = (cur, P1, m1);
//   coasting tracks (age > 0) keep their entry: they still occupy their zones;
//   zone_occ[z] = entries with seen_id >= 0 and bit z;  zone_dwell[z] += zone_occ[z].
// zone_mask [N, max_det]: for the rows r < count the zones holding the anchor of the row's own
// quantised box under the row's class, 0 for the others; zone_counts [N, 48]: the 48 counters
// after this step.  Every element of both is written.
//
// Launch shape: ONE WAVEFRONT PER STREAM, the tracker's mapping: slot t in lane t & 63, register
// set t >> 6; row r in lane r & 63, set r >> 6.  A lane tests its TJ slot anchors and its row
// anchors (up to 5; a set past count is skipped, a scalar branch) against each edge as the wave
// walks the (wave-uniform) region table once: at most 8 lines + 64 edges.  Counter deltas are
// wave-reduced with popcount(ballot) and lane 0 adds them to the state.  No LDS, no barrier, no
// atomics; the tracker state is only read, and streams outside [slot0, slot0 + N) are not
// touched.
#include "common.h"
#include "kvedge_kernels.h"
#include "resample.h"  // rs_in_alloc

namespace kvedge {
namespace {

constexpr int kZnWave = 64;
constexpr int kZnMaxDet = 300;
constexpr int kZnDJ = (kZnMaxDet + kZnWave - 1) / kZnWave;  // row sets per lane
constexpr int kZnMax = 8;                                   // lines, zones, vertices
constexpr int kZnCounters = 6 * kZnMax;
constexpr int kZnTab = 188;
constexpr int kZnLine = 0, kZnLineCls = 32, kZnVert = 40, kZnNVert = 168, kZnZoneCls = 176,
              kZnMeta = 184;

__host__ __device__ constexpr int zn_stride(int T) { return 4 * T + kZnCounters; }
__host__ __device__ constexpr int zn_trk_stride(int T) { return 12 * T + 4; }  // track.hip

// the tracker's quantisation and class clamp (track.hip trk_q / trk_cls)
__device__ __forceinline__ int zn_q(float x) {
  return (int)fminf(fmaxf(floorf(x * 4.f + 0.5f), 0.f), 16384.f);
}

__device__ __forceinline__ int zn_cls(float c) {
  return (int)fminf(fmaxf(c, 0.f), 65535.f);
}

__device__ __forceinline__ int zn_clamp8(int v) { return min(max(v, 0), kZnMax); }

__device__ __forceinline__ long long zn_cross(int ux, int uy, int vx, int vy) {
  return (long long)ux * vy - (long long)uy * vx;
}

template <int TJ>
__global__ __launch_bounds__(kZnWave) void zone_update_kernel(
    const float* __restrict__ det, const int* __restrict__ count,
    const int* __restrict__ track_state, int* __restrict__ zone_state,
    const int* __restrict__ table, int* __restrict__ zone_mask, int* __restrict__ zone_counts,
    int slot0, int max_det) {
  constexpr int T = TJ * kZnWave;
  constexpr int NP = TJ + kZnDJ;  // points per lane: slot anchors, then row anchors
  const int n = (int)blockIdx.x;
  const int lane = (int)threadIdx.x;
  const int* ts = track_state + (long long)(slot0 + n) * zn_trk_stride(T);
  const int4* t_box = reinterpret_cast<const int4*>(ts);
  const int* t_cls = ts + 8 * T;
  const int* t_id = ts + 9 * T;
  const int* t_age = ts + 10 * T;
  const int* t_hits = ts + 11 * T;
  int* zs = zone_state + (long long)(slot0 + n) * zn_stride(T);
  int4* z_ent = reinterpret_cast<int4*>(zs);
  int* z_cnt = zs + 4 * T;
  const int* tab = table + (long long)(slot0 + n) * kZnTab;
  const int n_lines = zn_clamp8(tab[kZnMeta + 0]);
  const int n_zones = zn_clamp8(tab[kZnMeta + 1]);
  const bool centre = tab[kZnMeta + 2] == 1;
  const int cnt = __builtin_amdgcn_readfirstlane(min(max(count[n], 0), max_det));

  // the points to place: this lane's slot anchors and row anchors, with their classes
  int px[NP], py[NP], pc[NP], pm[NP];
  int cur[TJ], age[TJ];
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int t = j * kZnWave + lane;
    const int4 b = t_box[t];
    px[j] = (b.x + b.z) >> 1;
    py[j] = centre ? (b.y + b.w) >> 1 : b.w;
    pc[j] = t_cls[t];
    pm[j] = 0;
    const int id = t_id[t];
    cur[j] = (t_hits[t] > 0 && id >= 0) ? id : -1;
    age[j] = t_age[t];
  }
#pragma unroll
  for (int jr = 0; jr < kZnDJ; ++jr) {
    const int r = jr * kZnWave + lane;
    const int k = TJ + jr;
    px[k] = py[k] = pc[k] = pm[k] = 0;
    if (r < cnt) {  // r < max_det: inside det[n]
      const float* p = det + ((long long)n * max_det + r) * 6;
      const int x1 = zn_q(p[0]), y1 = zn_q(p[1]), x2 = zn_q(p[2]), y2 = zn_q(p[3]);
      px[k] = (x1 + x2) >> 1;
      py[k] = centre ? (y1 + y2) >> 1 : y2;
      pc[k] = zn_cls(p[5]);
    }
  }

  // zones: the wave walks the edges, every lane toggles its points
  for (int z = 0; z < n_zones; ++z) {
    const int nv = zn_clamp8(tab[kZnNVert + z]);
    if (nv < 3) continue;
    const int zc = tab[kZnZoneCls + z];
    const int* v = tab + kZnVert + z * (2 * kZnMax);
    bool in[NP];
#pragma unroll
    for (int k = 0; k < NP; ++k) in[k] = false;
    int xj = v[2 * (nv - 1)], yj = v[2 * (nv - 1) + 1];
    for (int i = 0; i < nv; ++i) {
      const int xi = v[2 * i], yi = v[2 * i + 1];
      const int dx = xj - xi, dy = yj - yi;
#pragma unroll
      for (int k = 0; k < NP; ++k) {
        if (k >= TJ && (k - TJ) * kZnWave >= cnt) continue;  // a row set past count (uniform)
        if ((yi > py[k]) != (yj > py[k])) {  // dy != 0 here
          const long long t = (long long)dx * (py[k] - yi) - (long long)(px[k] - xi) * dy;
          if (dy > 0 ? t > 0 : t < 0) in[k] = !in[k];
        }
      }
      xj = xi;
      yj = yi;
    }
#pragma unroll
    for (int k = 0; k < NP; ++k)
      if (in[k] && (zc == -1 || zc == pc[k])) pm[k] |= 1 << z;
  }

  // slots: gone tracks leave, sighted tracks move
  int4 ent[TJ];
  int enter[TJ], leave[TJ], fwd[TJ], back[TJ];
  bool sighted[TJ], moved[TJ];
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    ent[j] = z_ent[j * kZnWave + lane];
    enter[j] = leave[j] = fwd[j] = back[j] = 0;
    if (ent[j].x != cur[j] && ent[j].x >= 0) {
      leave[j] = ent[j].w;
      ent[j] = make_int4(-1, 0, 0, 0);
    }
    sighted[j] = cur[j] >= 0 && age[j] == 0;
    moved[j] = sighted[j] && ent[j].x == cur[j];
  }
  for (int l = 0; l < n_lines; ++l) {
    const int ax = tab[kZnLine + 4 * l], ay = tab[kZnLine + 4 * l + 1];
    const int bx = tab[kZnLine + 4 * l + 2], by = tab[kZnLine + 4 * l + 3];
    const int lc = tab[kZnLineCls + l];
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      if (moved[j] && (lc == -1 || lc == pc[j])) {
        const int x0 = ent[j].y, y0 = ent[j].z, x1 = px[j], y1 = py[j];
        const bool s0 = zn_cross(bx - ax, by - ay, x0 - ax, y0 - ay) >= 0;
        const bool s1 = zn_cross(bx - ax, by - ay, x1 - ax, y1 - ay) >= 0;
        const bool pa = zn_cross(x1 - x0, y1 - y0, ax - x0, ay - y0) >= 0;
        const bool pb = zn_cross(x1 - x0, y1 - y0, bx - x0, by - y0) >= 0;
        if (s0 != s1 && pa != pb) {
          if (s0) fwd[j] |= 1 << l;
          else back[j] |= 1 << l;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    if (sighted[j]) {
      const int m1 = pm[j];
      if (moved[j]) {
        enter[j] = m1 & ~ent[j].w;
        leave[j] |= ent[j].w & ~m1;
      } else {
        enter[j] = m1;
      }
      ent[j] = make_int4(cur[j], px[j], py[j], m1);
    }
    z_ent[j * kZnWave + lane] = ent[j];
  }

  // counter deltas over the wave; lane 0 adds them to the state (unsigned: wraps modulo 2^32)
  unsigned d[kZnCounters];
#pragma unroll
  for (int i = 0; i < kZnMax; ++i) {
    unsigned f = 0, b = 0, e = 0, x = 0, o = 0;
#pragma unroll
    for (int j = 0; j < TJ; ++j) {
      f += __popcll(__ballot((fwd[j] >> i) & 1));
      b += __popcll(__ballot((back[j] >> i) & 1));
      e += __popcll(__ballot((enter[j] >> i) & 1));
      x += __popcll(__ballot((leave[j] >> i) & 1));
      o += __popcll(__ballot(ent[j].x >= 0 && ((ent[j].w >> i) & 1)));
    }
    d[i] = f;
    d[kZnMax + i] = b;
    d[2 * kZnMax + i] = e;
    d[3 * kZnMax + i] = x;
    d[4 * kZnMax + i] = o;
    d[5 * kZnMax + i] = o;
  }
  if (lane == 0) {
    int* out = zone_counts + (long long)n * kZnCounters;
#pragma unroll
    for (int i = 0; i < kZnCounters; ++i) {
      const bool occ = i >= 4 * kZnMax && i < 5 * kZnMax;  // current value, not a sum
      const int v = (int)((occ ? 0u : (unsigned)z_cnt[i]) + d[i]);
      z_cnt[i] = v;
      out[i] = v;
    }
  }
  // rows >= cnt get 0 (in a partly filled set their padding anchor (0, 0) was tested too, and
  // may lie in a zone): every element of zone_mask[n] is written
  int* zm = zone_mask + (long long)n * max_det;
#pragma unroll
  for (int jr = 0; jr < kZnDJ; ++jr) {
    const int r = jr * kZnWave + lane;
    if (r < max_det) zm[r] = r < cnt ? pm[TJ + jr] : 0;
  }
}

template <int TJ>
int zn_launch(const float* det, const int* count, const int* track_state, int* zone_state,
              const int* table, int* zone_mask, int* zone_counts, int N, int slot0, int max_det,
              hipStream_t s) {
  hipLaunchKernelGGL(zone_update_kernel<TJ>, dim3((unsigned)N), dim3(kZnWave), 0, s, det, count,
                     track_state, zone_state, table, zone_mask, zone_counts, slot0, max_det);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}

}  // namespace
}  // namespace kvedge

using namespace kvedge;

extern "C" int kv_zone_state_stride(int T) { return zn_stride(T); }

extern "C" int kv_zone_table_stride(void) { return kZnTab; }

extern "C" int kv_zone_update(const float* det, const int* count, const int* track_state,
                              int* zone_state, const int* table, int* zone_mask,
                              int* zone_counts, int N, int S, int slot0, int T, int max_det,
                              hipStream_t s) {
  if (T != 64 && T != 128 && T != 192 && T != 256) return -1;
  if (N < 0 || S < 0 || slot0 < 0 || (long long)slot0 + N > S) return -2;
  if (max_det < 1 || max_det > kZnMaxDet) return -3;
  if ((reinterpret_cast<uintptr_t>(track_state) | reinterpret_cast<uintptr_t>(zone_state)) & 15)
    return -7;  // 16-byte box / entry accesses
  if (reinterpret_cast<uintptr_t>(table) & 3) return -8;
  if (N == 0) return 0;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(det, (long long)N * max_det * 6 * 4)) return -20;
  if (!rs_in_alloc(count, (long long)N * 4)) return -21;
  if (!rs_in_alloc(track_state + (long long)slot0 * zn_trk_stride(T),
                   (long long)N * zn_trk_stride(T) * 4))
    return -22;
  if (!rs_in_alloc(zone_state + (long long)slot0 * zn_stride(T), (long long)N * zn_stride(T) * 4))
    return -23;
  if (!rs_in_alloc(table + (long long)slot0 * kZnTab, (long long)N * kZnTab * 4)) return -24;
  if (!rs_in_alloc(zone_mask, (long long)N * max_det * 4)) return -25;
  if (!rs_in_alloc(zone_counts, (long long)N * kZnCounters * 4)) return -26;
#endif
  switch (T / kZnWave) {
    case 1: return zn_launch<1>(det, count, track_state, zone_state, table, zone_mask, zone_counts, N, slot0, max_det, s);
    case 2: return zn_launch<2>(det, count, track_state, zone_state, table, zone_mask, zone_counts, N, slot0, max_det, s);
    case 3: return zn_launch<3>(det, count, track_state, zone_state, table, zone_mask, zone_counts, N, slot0, max_det, s);
    default: return zn_launch<4>(det, count, track_state, zone_state, table, zone_mask, zone_counts, N, slot0, max_det, s);
  }
}
