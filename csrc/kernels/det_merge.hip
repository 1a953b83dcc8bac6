// K28 (cross-group detection merge): the NMS outputs of `groups` passes over one camera -- the
// tiles of a sliced frame plus the full frame -- become one detection list, on the device and
// inside the captured step.  Greedy suppression (mode nms) or greedy merge (mode nmm: the kept
// box grows to the hull of what it absorbed), by IoU or by IoS = inter / min(area), the
// measure that lets the whole box one tile saw absorb the half a tile border cut off.
//
// The rule is ops.reference.det_merge, and this kernel equals it bit for bit:
//   candidates  rows r < clamp(count[g * N + n], 0, R) of every group g of camera n; edges
//               quantised to quarter pixels q(x) = (int) min(max(floor(x * 4 + 0.5), 0), 16384)
//               (the tracker's), class (int) min(max(c, 0), 65535), score s = score > 0 ? score
//               : +0 (NaN and negatives are 0);
//   order       s descending, then group, then row ascending;
//   match(a, b) same class (class_aware), inter > 0 and inter * 1024 >= thr_q * denom in int64,
//               denom = union (iou) or min(area_a, area_b) (ios); always on the ORIGINAL
//               quantised boxes.  Extents <= 2^14: inter, the areas and the union fit int32;
//   sweep       in order: a candidate that matches an earlier KEPT one is absorbed by the
//               earliest such one, else it is kept; the sweep ends when max_det are kept;
//   output      row k: the kept candidate's own six floats with the score as s (nms) or the
//               hull of it and what it absorbed as q / 4 (nmm); rows >= the count are zero.
//
// ONE WORKGROUP OF 8 WAVEFRONTS PER CAMERA, everything between the first load and the last
// store in LDS (32 bytes per candidate slot + 8.5 KiB; 4096 candidates = 136 KiB of the 160):
//   load    wave 0 scans the clamped counts into per-group offsets, so the candidates sit
//           densely at pos = offset[g] + r -- the sort is sized by the boxes that exist, not by
//           groups * R.  Every thread then reads whole rows (neighbouring lanes, neighbouring
//           24-byte rows) and leaves a 64-bit key  score_bits << 32 | ~pos  (pos grows with
//           (g, r), so the key orders exactly as the rule does and no two are equal), the four
//           edges as 16-bit words and class << 16 | g * R + r;
//   sort    bitonic, descending, over the next power of two of the total; pad keys are 0 and
//           every real key is larger;
//   gather  boxes and class words once into sorted order, so the sweep reads LDS linearly;
//   sweep   chunks of 64 sorted candidates, lane = candidate.  Every wave tests the chunk
//           against its interleaved share of the kept list (kept box = one broadcast LDS read)
//           and leaves the EARLIEST matching kept index per candidate with an LDS atomicMin.
//           Wave 0 then walks the chunk's survivors in order: the first one is kept, its box
//           is broadcast with v_readlane, the lanes it matches are struck from the 64-bit
//           survivor mask with one ballot, and so on -- at most max_det such steps in total;
//   hull    (nmm) one parallel pass: LDS atomicMin / atomicMax of each absorbed candidate's
//           edges into its absorber's hull;
//   write   one thread per output row, three 8-byte stores; the tail is zeroed.
// Matching is integer only; the one float compare is score > 0 when the key is built.
#include <atomic>

#include "common.h"
#include "kvedge_kernels.h"
#include "resample.h"  // rs_in_alloc

namespace kvedge {
namespace {

constexpr int kDmThreads = 512;
constexpr int kDmWaves = kDmThreads / 64;
constexpr int kDmMaxCand = 4096;
constexpr int kDmMaxDet = 300;
constexpr int kDmInf = 0x7fffffff;
constexpr unsigned kDmNone = 0xffffu;  // absorber word: not absorbed
// after the 32 bytes per slot: hull int4, kept box uint2 and kept word per kept row, the
// chunk's 64 earliest-absorber words and the kept count
constexpr int kDmFixedLds = kDmMaxDet * (16 + 8 + 4) + 64 * 4 + 16;

typedef unsigned long long dm_u64;

__device__ __forceinline__ int dm_q(float x) {
  return (int)fminf(fmaxf(floorf(x * 4.f + 0.5f), 0.f), 16384.f);
}

__device__ __forceinline__ int dm_cls(float c) {
  return (int)fminf(fmaxf(c, 0.f), 65535.f);
}

struct DmBox {
  int x1, y1, x2, y2, area, cls;
};

__device__ __forceinline__ DmBox dm_unpack(uint2 b, int cls) {
  DmBox o;
  o.x1 = (int)(b.x & 0xffffu);
  o.y1 = (int)(b.x >> 16);
  o.x2 = (int)(b.y & 0xffffu);
  o.y2 = (int)(b.y >> 16);
  o.area = max(o.x2 - o.x1, 0) * max(o.y2 - o.y1, 0);
  o.cls = cls;
  return o;
}

__device__ __forceinline__ bool dm_match(const DmBox& a, const DmBox& b, int thr_q, int use_iou,
                                         int class_aware) {
  const int iw = max(min(a.x2, b.x2) - max(a.x1, b.x1), 0);
  const int ih = max(min(a.y2, b.y2) - max(a.y1, b.y1), 0);
  const int inter = iw * ih;
  const int denom = use_iou ? a.area + b.area - inter : min(a.area, b.area);
  return inter > 0 && (long long)inter * 1024 >= (long long)thr_q * denom &&
         (!class_aware || a.cls == b.cls);
}

__global__ __launch_bounds__(kDmThreads) void det_merge_kernel(
    const float* __restrict__ det, const int* __restrict__ count, float* __restrict__ out,
    int* __restrict__ out_count, int N, int groups, int R, int P, int max_det, int thr_q,
    int use_iou, int class_aware, int nmm) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dm_lds[];
  dm_u64* key = reinterpret_cast<dm_u64*>(dm_lds);                 // [P]
  uint2* ubox = reinterpret_cast<uint2*>(dm_lds + 8 * P);          // [P] as loaded
  unsigned short* absorber = reinterpret_cast<unsigned short*>(ubox);  // [P] once gathered
  uint2* sbox = reinterpret_cast<uint2*>(dm_lds + 16 * P);         // [P] sorted
  int* off = reinterpret_cast<int*>(sbox);                         // [groups + 1] until the gather
  unsigned* umeta = reinterpret_cast<unsigned*>(dm_lds + 24 * P);  // cls << 16 | g * R + r
  unsigned* smeta = reinterpret_cast<unsigned*>(dm_lds + 28 * P);
  int4* hull = reinterpret_cast<int4*>(dm_lds + 32 * P);           // [kDmMaxDet]
  uint2* kbox = reinterpret_cast<uint2*>(hull + kDmMaxDet);        // [kDmMaxDet]
  unsigned* kmeta = reinterpret_cast<unsigned*>(kbox + kDmMaxDet);  // cls << 16 | sorted index
  int* early = reinterpret_cast<int*>(kmeta + kDmMaxDet);          // [64]
  int* ctl = early + 64;

  const int n = (int)blockIdx.x;
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // offsets of the groups' clamped counts: off[g] .. off[g + 1] are group g's candidates
  if (wave == 0) {
    int carry = 0;
    for (int base = 0; base < groups; base += 64) {
      const int g = base + lane;
      const int c = g < groups ? min(max(count[(long long)g * N + n], 0), R) : 0;
      int incl = c;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
      }
      if (g < groups) off[g] = carry + incl - c;
      carry += __shfl(incl, 63);
    }
    if (lane == 0) off[groups] = carry;
    early[lane] = kDmInf;
  }
  __syncthreads();
  const int tot = off[groups];  // <= groups * R <= P
  int Ps = 64;
  while (Ps < tot) Ps <<= 1;

  // load: u = g * R + r over all rows; neighbouring lanes read neighbouring rows
  const int GR = groups * R;
  for (int u = tid; u < GR; u += kDmThreads) {
    const int g = u / R, r = u - g * R;
    const int pos0 = off[g];
    if (r < off[g + 1] - pos0) {  // r < R: inside det[g * N + n]
      const float* p = det + (((long long)g * N + n) * R + r) * 6;
      const float2 a = *reinterpret_cast<const float2*>(p);
      const float2 b = *reinterpret_cast<const float2*>(p + 2);
      const float2 c = *reinterpret_cast<const float2*>(p + 4);
      const float s = c.x > 0.f ? c.x : 0.f;
      const int pos = pos0 + r;
      key[pos] = ((dm_u64)__float_as_uint(s) << 32) | (unsigned)~pos;
      ubox[pos] = make_uint2((unsigned)dm_q(a.x) | ((unsigned)dm_q(a.y) << 16),
                             (unsigned)dm_q(b.x) | ((unsigned)dm_q(b.y) << 16));
      umeta[pos] = ((unsigned)dm_cls(c.y) << 16) | (unsigned)u;
    }
  }
  for (int i = tot + tid; i < Ps; i += kDmThreads) key[i] = 0;
  __syncthreads();

  // bitonic sort, descending
  for (int k = 2; k <= Ps; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (Ps >> 1); t += kDmThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i | j;
        const bool desc = (i & k) == 0;
        const dm_u64 a = key[i], b = key[l];
        if ((a < b) == desc) {
          key[i] = b;
          key[l] = a;
        }
      }
      __syncthreads();
    }
  }

  // gather into sorted order (off is dead from here: sbox takes its place)
  uint2 gb[kDmMaxCand / kDmThreads];
  unsigned gm[kDmMaxCand / kDmThreads];
#pragma unroll
  for (int j = 0; j < kDmMaxCand / kDmThreads; ++j) {
    const int i = j * kDmThreads + tid;
    if (i < tot) {
      const unsigned pos = ~(unsigned)key[i];  // < tot: the first tot keys are the real ones
      gb[j] = ubox[pos];
      gm[j] = umeta[pos];
    }
  }
  __syncthreads();  // every ubox / off read is done: absorber and sbox may overwrite them
#pragma unroll
  for (int j = 0; j < kDmMaxCand / kDmThreads; ++j) {
    const int i = j * kDmThreads + tid;
    if (i < tot) {
      sbox[i] = gb[j];
      smeta[i] = gm[j];
      absorber[i] = (unsigned short)kDmNone;
    }
  }
  __syncthreads();

  // sweep
  int nk = 0;
  for (int c0 = 0; c0 < tot && nk < max_det; c0 += 64) {
    const int i = c0 + lane;
    const bool valid = i < tot;
    const uint2 bb = valid ? sbox[i] : make_uint2(0u, 0u);
    const unsigned mm = valid ? smeta[i] : 0u;
    const DmBox cb = dm_unpack(bb, (int)(mm >> 16));
    int m = kDmInf;
    for (int k = wave; k < nk; k += kDmWaves) {
      const DmBox kb = dm_unpack(kbox[k], (int)(kmeta[k] >> 16));
      if (m == kDmInf && dm_match(kb, cb, thr_q, use_iou, class_aware)) m = k;
    }
    if (valid && m != kDmInf) atomicMin(&early[lane], m);
    __syncthreads();
    if (wave == 0) {
      const int e = early[lane];
      early[lane] = kDmInf;
      unsigned ab = (valid && e != kDmInf) ? (unsigned)e : kDmNone;
      dm_u64 mask = __ballot(valid && e == kDmInf);  // survivors of the kept list so far
      int stop = 64;
      while (mask) {
        const int j = __builtin_ctzll(mask);
        mask &= mask - 1;
        DmBox jb;
        jb.x1 = __builtin_amdgcn_readlane(cb.x1, j);
        jb.y1 = __builtin_amdgcn_readlane(cb.y1, j);
        jb.x2 = __builtin_amdgcn_readlane(cb.x2, j);
        jb.y2 = __builtin_amdgcn_readlane(cb.y2, j);
        jb.area = __builtin_amdgcn_readlane(cb.area, j);
        jb.cls = __builtin_amdgcn_readlane(cb.cls, j);
        if (lane == j) {  // nk < max_det <= kDmMaxDet
          kbox[nk] = bb;
          kmeta[nk] = (mm & 0xffff0000u) | (unsigned)i;
          hull[nk] = make_int4(cb.x1, cb.y1, cb.x2, cb.y2);
        }
        const int kept = nk++;
        if (nk == max_det) {  // the sweep ends here: what follows is dropped, not absorbed
          stop = j;
          break;
        }
        const bool hit = ((mask >> lane) & 1ull) && dm_match(jb, cb, thr_q, use_iou, class_aware);
        if (hit) ab = (unsigned)kept;
        mask &= ~__ballot(hit);
      }
      if (lane > stop) ab = kDmNone;
      if (valid) absorber[i] = (unsigned short)ab;
      if (lane == 0) ctl[0] = nk;
    }
    __syncthreads();
    nk = ctl[0];
  }
  __syncthreads();

  if (nmm) {
    for (int i = tid; i < tot; i += kDmThreads) {
      const unsigned ab = absorber[i];
      if (ab != kDmNone) {  // ab < nk
        const uint2 b = sbox[i];
        atomicMin(&hull[ab].x, (int)(b.x & 0xffffu));
        atomicMin(&hull[ab].y, (int)(b.x >> 16));
        atomicMax(&hull[ab].z, (int)(b.y & 0xffffu));
        atomicMax(&hull[ab].w, (int)(b.y >> 16));
      }
    }
    __syncthreads();
  }

  for (int k = tid; k < max_det; k += kDmThreads) {
    float2 o0 = make_float2(0.f, 0.f), o1 = o0, o2 = o0;
    if (k < nk) {
      const int i = (int)(kmeta[k] & 0xffffu);
      const int u = (int)(smeta[i] & 0xffffu);  // < groups * R
      const int g = u / R, r = u - g * R;
      const float* p = det + (((long long)g * N + n) * R + r) * 6;
      if (nmm) {
        const int4 h = hull[k];
        o0 = make_float2((float)h.x * 0.25f, (float)h.y * 0.25f);
        o1 = make_float2((float)h.z * 0.25f, (float)h.w * 0.25f);
      } else {
        o0 = *reinterpret_cast<const float2*>(p);
        o1 = *reinterpret_cast<const float2*>(p + 2);
      }
      o2 = make_float2(__uint_as_float((unsigned)(key[i] >> 32)), p[5]);
    }
    float2* o = reinterpret_cast<float2*>(out + ((long long)n * max_det + k) * 6);
    o[0] = o0;
    o[1] = o1;
    o[2] = o2;
  }
  if (tid == 0) out_count[n] = nk;
}

// The kernel's dynamic-LDS limit is raised once per device, to what the largest launch needs
// (4096 candidates), not at every launch: dm_lds_ready[d] is set once device d has it.
constexpr int kDmMaxLds = 32 * kDmMaxCand + kDmFixedLds;
constexpr int kDmDevices = 64;
std::atomic<bool> dm_lds_ready[kDmDevices];

bool dm_allow_lds() {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  const bool cached = dev >= 0 && dev < kDmDevices;
  if (cached && dm_lds_ready[dev].load(std::memory_order_acquire)) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(det_merge_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, kDmMaxLds) != hipSuccess)
    return false;
  if (cached) dm_lds_ready[dev].store(true, std::memory_order_release);
  return true;
}

}  // namespace
}  // namespace kvedge

using namespace kvedge;

extern "C" int kv_det_merge(const float* det, const int* count, float* out, int* out_count, int N,
                            int groups, int R, int max_det, int thr_q, int use_iou,
                            int class_aware, int nmm, hipStream_t s) {
  if (groups < 1 || R < 1 || R > kDmMaxDet || (long long)groups * R > kDmMaxCand) return -1;
  if (max_det < 1 || max_det > R) return -2;
  if (thr_q < 1 || thr_q > 1024) return -3;
  if (N < 0 || N > 65535) return -4;
  if ((reinterpret_cast<uintptr_t>(det) | reinterpret_cast<uintptr_t>(out)) & 7) return -7;
  if ((reinterpret_cast<uintptr_t>(count) | reinterpret_cast<uintptr_t>(out_count)) & 3) return -7;
  if (N == 0) return 0;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(det, (long long)groups * N * R * 24)) return -20;
  if (!rs_in_alloc(count, (long long)groups * N * 4)) return -21;
  if (!rs_in_alloc(out, (long long)N * max_det * 24)) return -22;
  if (!rs_in_alloc(out_count, (long long)N * 4)) return -23;
#endif
  int P = 64;
  while (P < groups * R) P <<= 1;
  const int lds = 32 * P + kDmFixedLds;
  if (!dm_allow_lds()) return -100;
  hipLaunchKernelGGL(det_merge_kernel, dim3((unsigned)N), dim3(kDmThreads), (unsigned)lds, s, det,
                     count, out, out_count, N, groups, R, P, max_det, thr_q, use_iou ? 1 : 0,
                     class_aware ? 1 : 0, nmm ? 1 : 0);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}
