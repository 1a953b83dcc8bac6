// K18 (multi-object tracker): ties every detection row of this step to the track it continues,
// so the same object keeps the same id from frame to frame.  It runs where the detections
// already are -- on the NMS output in device memory, inside the captured step, no host sync.
//
// One batch row = one camera ("stream").  Stream s keeps T = 64 * TJ track slots as int32:
//   box[4] vel[4] (quarter pixels, per frame)  cls  id (-1 = not confirmed)  age (frames since
//   the last match)  hits (0 = free slot);  per stream also next_id (ids handed out so far)
//   and dropped (detections that found no free slot).
// Memory layout of one stream, in ints (kTrkStride(T) = 12 T + 4 of them):
//   box [T][4] | vel [T][4] | cls [T] | id [T] | age [T] | hits [T] | next_id dropped 0 0
//
// Everything after the quantisation q(x) = (int) min(max(floor(x * 4 + 0.5), 0), 16384)
// (fmaxf(NaN, 0) = 0; x * 4 is exact, so an FMA contraction cannot change it) is integer
// arithmetic, so the result is bit-identical to ops.reference.track_update:
//   inter = max(0, min(x2) - max(x1)) * max(0, min(y2) - max(y1)),  union = a + b - inter;
//   extents <= 2^14, so inter <= 2^28 and union <= 2^29 fit int32; the threshold test
//   inter * 1024 >= thr_q * union and the ratio compare inter_a * union_b > inter_b * union_a
//   (<= 2^57) are int64.  No divide, no float compare: GPU and CPU cannot disagree on a tie.
//
// One update, in this order: predict (box + vel * (age + 1), clamped) -> associate the rows
// r = 0 .. count - 1 in order (NMS orders them by score), each claiming the best candidate
// among the slots live at entry and not yet claimed (lower slot wins a tie) -> age the
// unclaimed slots (freed past max_age, or at once while unconfirmed) -> unmatched rows, in
// row order, take the lowest free slot -> track_id, every element written.
//
// Launch shape: ONE WAVEFRONT PER STREAM.  Association is sequential over the rows and parallel
// over the slots: slot t lives in lane t & 63, register set t >> 6, for the whole kernel; the
// quantised rows are loaded once (row r in lane r & 63, set r >> 6) and broadcast with
// v_readlane as the loop reaches them.  One row = TJ integer IoUs per lane and a six-step
// __shfl_xor butterfly over (inter, union, slot); the ratio order with the slot tie-break is a
// total order, so every lane ends with the same winner.  No LDS, no barrier, no atomics; the
// state is read once and written once, and streams outside [slot0, slot0 + N) are not touched.
#include "common.h"
#include "kvedge_kernels.h"
#include "resample.h"  // rs_in_alloc

namespace kvedge {
namespace {

constexpr int kTrkWave = 64;
constexpr int kTrkMaxDet = 300;
constexpr int kTrkDJ = (kTrkMaxDet + kTrkWave - 1) / kTrkWave;  // row sets per lane
constexpr int kTrkUnmatched = -2;  // track_id of a row waiting for the birth pass (never stored)

__host__ __device__ constexpr int trk_stride(int T) { return 12 * T + 4; }

__device__ __forceinline__ int trk_q(float x) {
  return (int)fminf(fmaxf(floorf(x * 4.f + 0.5f), 0.f), 16384.f);
}

__device__ __forceinline__ int trk_cls(float c) {
  return (int)fminf(fmaxf(c, 0.f), 65535.f);
}

__device__ __forceinline__ int trk_clamp(int v) { return min(max(v, 0), 16384); }

__device__ __forceinline__ int4 trk_bcast(const int4& v, int src_lane) {
  return make_int4(__builtin_amdgcn_readlane(v.x, src_lane), __builtin_amdgcn_readlane(v.y, src_lane),
                   __builtin_amdgcn_readlane(v.z, src_lane), __builtin_amdgcn_readlane(v.w, src_lane));
}

template <int TJ>
__global__ __launch_bounds__(kTrkWave) void track_update_kernel(
    const float* __restrict__ det, const int* __restrict__ count, int* __restrict__ state,
    int* __restrict__ track_id, int slot0, int max_det, int thr_q, int max_age, int min_hits,
    int class_aware) {
  constexpr int T = TJ * kTrkWave;
  const int n = (int)blockIdx.x;
  const int lane = (int)threadIdx.x;
  int* st = state + (long long)(slot0 + n) * trk_stride(T);
  int4* s_box = reinterpret_cast<int4*>(st);
  int4* s_vel = reinterpret_cast<int4*>(st + 4 * T);
  int* s_cls = st + 8 * T;
  int* s_id = st + 9 * T;
  int* s_age = st + 10 * T;
  int* s_hits = st + 11 * T;
  int* s_meta = st + 12 * T;

  int4 box[TJ], vel[TJ], pred[TJ];
  int cls[TJ], id[TJ], age[TJ], hits[TJ], parea[TJ];
  bool live[TJ], claimed[TJ];
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int t = j * kTrkWave + lane;
    box[j] = s_box[t];
    vel[j] = s_vel[t];
    cls[j] = s_cls[t];
    id[j] = s_id[t];
    age[j] = s_age[t];
    hits[j] = s_hits[t];
    live[j] = hits[j] > 0;
    claimed[j] = false;
    const int dt = age[j] + 1;
    pred[j] = make_int4(trk_clamp(box[j].x + vel[j].x * dt), trk_clamp(box[j].y + vel[j].y * dt),
                        trk_clamp(box[j].z + vel[j].z * dt), trk_clamp(box[j].w + vel[j].w * dt));
    parea[j] = max(pred[j].z - pred[j].x, 0) * max(pred[j].w - pred[j].y, 0);
  }
  int next_id = s_meta[0];
  int dropped = s_meta[1];
  const int cnt = __builtin_amdgcn_readfirstlane(min(max(count[n], 0), max_det));

  // the step's rows, quantised once: row r in lane r & 63, set r >> 6
  int4 dq[kTrkDJ];
  int dc[kTrkDJ], tid[kTrkDJ];
#pragma unroll
  for (int jr = 0; jr < kTrkDJ; ++jr) {
    const int r = jr * kTrkWave + lane;
    dq[jr] = make_int4(0, 0, 0, 0);
    dc[jr] = 0;
    tid[jr] = -1;
    if (r < cnt) {  // r < max_det: inside det[n]
      const float* p = det + ((long long)n * max_det + r) * 6;
      dq[jr] = make_int4(trk_q(p[0]), trk_q(p[1]), trk_q(p[2]), trk_q(p[3]));
      dc[jr] = trk_cls(p[5]);
    }
  }

  // associate: rows in order, each a wave-wide argmax over the slots
#pragma unroll
  for (int jr = 0; jr < kTrkDJ; ++jr) {
    const int rows = min(cnt - jr * kTrkWave, kTrkWave);  // wave-uniform
    for (int rl = 0; rl < rows; ++rl) {
      const int4 d = trk_bcast(dq[jr], rl);
      const int dcl = __builtin_amdgcn_readlane(dc[jr], rl);
      const int darea = max(d.z - d.x, 0) * max(d.w - d.y, 0);
      int bi = 0, bu = 1, bs = 0x7fffffff;  // no candidate: inter 0
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const int iw = max(min(pred[j].z, d.z) - max(pred[j].x, d.x), 0);
        const int ih = max(min(pred[j].w, d.w) - max(pred[j].y, d.y), 0);
        const int inter = iw * ih;
        const int uni = parea[j] + darea - inter;
        const bool cand = live[j] && !claimed[j] && inter > 0 &&
                          (long long)inter * 1024 >= (long long)thr_q * uni &&
                          (!class_aware || cls[j] == dcl);
        // strictly better only: within a lane the lower set is the lower slot
        if (cand && (long long)inter * bu > (long long)bi * uni) {
          bi = inter;
          bu = uni;
          bs = j * kTrkWave + lane;
        }
      }
#pragma unroll
      for (int off = kTrkWave / 2; off; off >>= 1) {
        const int oi = __shfl_xor(bi, off);
        const int ou = __shfl_xor(bu, off);
        const int os = __shfl_xor(bs, off);
        const long long theirs = (long long)oi * bu, mine = (long long)bi * ou;
        if (theirs > mine || (theirs == mine && os < bs)) {
          bi = oi;
          bu = ou;
          bs = os;
        }
      }
      // every lane holds the same winner
      const int m = __builtin_amdgcn_readfirstlane(bs);
      int rid = kTrkUnmatched;
      if (__builtin_amdgcn_readfirstlane(bi) > 0) {
        const int ml = m & (kTrkWave - 1), mj = m >> 6;
        int pid = 0, ph = 0;
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          if (j == mj) {
            pid = id[j];
            ph = hits[j];
          }
        }
        pid = __builtin_amdgcn_readlane(pid, ml);
        ph = __builtin_amdgcn_readlane(ph, ml);
        const int nh = ph + 1;
        rid = pid;
        if (pid < 0 && nh >= min_hits) rid = next_id++;
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          if (j == mj && lane == ml) {
            const int dt = age[j] + 1;
            vel[j] = make_int4((d.x - box[j].x) / dt, (d.y - box[j].y) / dt,
                               (d.z - box[j].z) / dt, (d.w - box[j].w) / dt);
            box[j] = d;
            age[j] = 0;
            hits[j] = nh;
            cls[j] = dcl;
            id[j] = rid;
            claimed[j] = true;
          }
        }
      }
      if (lane == rl) tid[jr] = rid;
    }
  }

  // age the slots that were live at entry and found no detection
#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    if (live[j] && !claimed[j]) {
      age[j] += 1;
      if (age[j] > max_age || id[j] < 0) {
        box[j] = make_int4(0, 0, 0, 0);
        vel[j] = make_int4(0, 0, 0, 0);
        cls[j] = 0;
        id[j] = -1;
        age[j] = 0;
        hits[j] = 0;
      }
    }
  }

  // birth: unmatched rows in order take the lowest free slot
#pragma unroll
  for (int jr = 0; jr < kTrkDJ; ++jr) {
    unsigned long long um = __ballot(tid[jr] == kTrkUnmatched);
    while (um) {
      const int rl = __builtin_ctzll(um);
      um &= um - 1;
      int slot = -1;
#pragma unroll
      for (int j = 0; j < TJ; ++j) {
        const unsigned long long fm = __ballot(hits[j] == 0);
        if (slot < 0 && fm) slot = j * kTrkWave + __builtin_ctzll(fm);
      }
      int rid = -1;
      if (slot >= 0) {
        const int4 d = trk_bcast(dq[jr], rl);
        const int dcl = __builtin_amdgcn_readlane(dc[jr], rl);
        if (min_hits <= 1) rid = next_id++;
        const int sl = slot & (kTrkWave - 1), sj = slot >> 6;
#pragma unroll
        for (int j = 0; j < TJ; ++j) {
          if (j == sj && lane == sl) {
            box[j] = d;
            vel[j] = make_int4(0, 0, 0, 0);
            cls[j] = dcl;
            id[j] = rid;
            age[j] = 0;
            hits[j] = 1;
          }
        }
      } else {
        dropped += 1;
      }
      if (lane == rl) tid[jr] = rid;
    }
  }

#pragma unroll
  for (int j = 0; j < TJ; ++j) {
    const int t = j * kTrkWave + lane;
    s_box[t] = box[j];
    s_vel[t] = vel[j];
    s_cls[t] = cls[j];
    s_id[t] = id[j];
    s_age[t] = age[j];
    s_hits[t] = hits[j];
  }
  if (lane == 0) {
    s_meta[0] = next_id;
    s_meta[1] = dropped;
  }
  // rows >= cnt kept their initial -1: every element of track_id[n] is written
  int* out = track_id + (long long)n * max_det;
#pragma unroll
  for (int jr = 0; jr < kTrkDJ; ++jr) {
    const int r = jr * kTrkWave + lane;
    if (r < max_det) out[r] = tid[jr];
  }
}

template <int TJ>
int trk_launch(const float* det, const int* count, int* state, int* track_id, int N, int slot0,
               int max_det, int thr_q, int max_age, int min_hits, int class_aware, hipStream_t s) {
  hipLaunchKernelGGL(track_update_kernel<TJ>, dim3((unsigned)N), dim3(kTrkWave), 0, s, det, count,
                     state, track_id, slot0, max_det, thr_q, max_age, min_hits, class_aware);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}

}  // namespace
}  // namespace kvedge

using namespace kvedge;

extern "C" int kv_track_state_stride(int T) { return trk_stride(T); }

extern "C" int kv_track_update(const float* det, const int* count, int* state, int* track_id,
                               int N, int S, int slot0, int T, int max_det, int thr_q, int max_age,
                               int min_hits, int class_aware, hipStream_t s) {
  if (T != 64 && T != 128 && T != 192 && T != 256) return -1;
  if (N < 0 || S < 0 || slot0 < 0 || (long long)slot0 + N > S) return -2;
  if (max_det < 1 || max_det > kTrkMaxDet) return -3;
  if (max_age < 0 || max_age > 255) return -4;
  if (min_hits < 1 || min_hits > 255) return -5;
  if (thr_q < 1 || thr_q > 1024) return -6;
  if (reinterpret_cast<uintptr_t>(state) & 15) return -7;  // 16-byte box / vel accesses
  if (N == 0) return 0;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(det, (long long)N * max_det * 6 * 4)) return -20;
  if (!rs_in_alloc(count, (long long)N * 4)) return -21;
  if (!rs_in_alloc(state + (long long)slot0 * trk_stride(T), (long long)N * trk_stride(T) * 4))
    return -22;
  if (!rs_in_alloc(track_id, (long long)N * max_det * 4)) return -23;
#endif
  const int ca = class_aware ? 1 : 0;
  switch (T / kTrkWave) {
    case 1: return trk_launch<1>(det, count, state, track_id, N, slot0, max_det, thr_q, max_age, min_hits, ca, s);
    case 2: return trk_launch<2>(det, count, state, track_id, N, slot0, max_det, thr_q, max_age, min_hits, ca, s);
    case 3: return trk_launch<3>(det, count, state, track_id, N, slot0, max_det, thr_q, max_age, min_hits, ca, s);
    default: return trk_launch<4>(det, count, state, track_id, N, slot0, max_det, thr_q, max_age, min_hits, ca, s);
  }
}
