// K29 (MJPEG camera sources): baseline JPEG files in device memory -> uint8 RGB frames in
// device memory, no host in the loop, capturable.  Three launches on one stream; every table
// comes from the file's own DQT / DHT segments and lives in the decoder's device scratch.
//
// ops.reference.jpeg_decode is THE definition (all integer, byte-identical, status words and
// malformed files included); the arithmetic and the parsing rules are in jpeg_decode_core.h,
// which the host self-test runs under sanitizers.
//
// Launches:
//   scan     one workgroup per file.  Thread 0 walks the marker segments up to SOS
//            (jd_parse_header) and writes the file's quantisation tables, its Huffman tables
//            (9-bit look-ahead + maxcode / valoff / symbols) and the scan geometry into the
//            image's JdTables in device scratch.  Then the 256 threads stream the entropy
//            bytes, 16 bytes per thread and 4 KiB per step: a thread marks the FF D0..D7 and
//            FF D9 pairs that start in its 16 bytes (the pair's second byte may be the next
//            thread's or the next step's first), a workgroup minimum finds the first EOI, a
//            wave scan (shuffles) plus the waves' totals in LDS number the markers in file
//            order, and their offsets are appended to mpos.  No atomics, no sort.
//   decode   one lane per restart interval, L = 16 / 32 / 64 lanes of one wave per workgroup
//            (a launch parameter).  The image's tables are copied into LDS.  A lane owns a
//            64-bit bit reservoir refilled from a 16-byte register window over its interval
//            (aligned 16-byte loads, FF 00 -> FF on the way), decodes one MCU's blocks into
//            its own LDS coefficients -- laid out [block][coefficient][lane], so the zeroing
//            and the IDCT's reads are conflict free -- runs the dequantising IDCT of its own
//            blocks in registers and stores 8-byte sample rows into the image's Y / Cb / Cr
//            planes in device scratch.  No barrier: a lane never reads another lane's data.
//            An entropy error zeroes the rest of the interval; a missing interval is all zero.
//   colour   one thread per 4 pixels of a row: Y from the plane, chroma by libjpeg's fancy
//            triangle upsampling with clamped (= replicated) edges, JFIF YCbCr -> RGB, three
//            dword stores where W % 4 == 0.  A header error zero-fills the image.  The
//            image's first thread writes status = -(error bits).
//
// Long restart intervals (a file without restart markers is one) get four more launches
// between scan and decode -- plan, speculate + synchronise, stitch, write: one lane per
// kJdSplitBytes subsequence, described at the kernels below and in docs/kernels.md, K29.  What
// they cannot prove equal to the one-lane walk they hand back to the decode launch, which skips
// the intervals they completed.
//
// Scratch per image: JdTables (6256 bytes), mpos int32 [ceil(H / 8) * ceil(W / 8)] (the
// worst case: 4:4:4 with a restart interval of one MCU), planes uint8 [3][H16][W16] with
// H16 / W16 = H / W rounded up to 16.
#include "common.h"
#include "kvedge_kernels.h"
#include "jpeg_decode_core.h"
#include "resample.h"  // rs_in_alloc

namespace kvedge {
namespace {

constexpr int kJdMaxExtent = 8192;
constexpr int kJdScanThreads = 256;
constexpr int kJdScanStep = kJdScanThreads * 16;
constexpr int kJdColourThreads = 256;

__global__ __launch_bounds__(kJdScanThreads) void jpeg_scan_kernel(
    const uint8_t* __restrict__ files, uint8_t* __restrict__ tables, int* __restrict__ mpos,
    long long row_bytes, int H, int W, int max_int) {
  __shared__ int s_info[4];  // e0, cap, header error
  __shared__ int s_min[kJdScanThreads / kWave];
  __shared__ int s_cnt[kJdScanThreads / kWave];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
  const int n = (int)row_bytes;
  const uint8_t* row = files + (long long)blockIdx.x * row_bytes;
  JdTables* T = reinterpret_cast<JdTables*>(tables + (long long)blockIdx.x * sizeof(JdTables));
  int* mp = mpos + (long long)blockIdx.x * max_int;
  if (tid == 0) {
    const int rc = jd_parse_header(row, n, H, W, T);
    T->info.err = rc;
    s_info[0] = T->info.e0;
    s_info[1] = min(T->info.expected, max_int);
    s_info[2] = rc;
  }
  __syncthreads();
  if (s_info[2]) return;
  const int e0 = s_info[0], cap = s_info[1];
  const int base0 = e0 & ~15;
  const int steps = (n - base0 + kJdScanStep - 1) / kJdScanStep;
  int nmark = 0;  // markers so far, RSTn and the EOI (uniform)
  bool eoi = false;
  for (int st = 0; st < steps; ++st) {
    const long long o = (long long)base0 + (long long)st * kJdScanStep + tid * 16;
    unsigned rst = 0, end = 0;  // bit j: a marker starts at byte o + j
    if (o < n) {                // rows are whole 16-byte words: o + 16 <= n
      const uint4 v = *reinterpret_cast<const uint4*>(row + o);
      const unsigned w[5] = {v.x, v.y, v.z, v.w, o + 16 < n ? (unsigned)row[o + 16] : 0u};
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const unsigned b0 = (w[j >> 2] >> (8 * (j & 3))) & 255u;
        const unsigned b1 = (w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 255u;
        const bool in = o + j >= e0;
        if (in && b0 == 0xffu && b1 >= 0xd0u && b1 <= 0xd7u) rst |= 1u << j;
        if (in && b0 == 0xffu && b1 == 0xd9u) end |= 1u << j;
      }
    }
    // the first EOI of the step
    int first = end ? (int)o + __ffs(end) - 1 : 0x7fffffff;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) first = min(first, __shfl_xor(first, d, kWave));
    if (lane == 0) s_min[wv] = first;
    __syncthreads();
    first = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
    // this thread's markers up to and including it, in file order
    unsigned mk = rst | end;
    if (first != 0x7fffffff) {
      const long long rel = (long long)first - o;  // keep bits 0..rel
      mk = rel < 0 ? 0u : rel >= 15 ? mk : mk & ((2u << rel) - 1u);
    }
    const int cnt = __popc(mk);
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int t = __shfl_up(incl, d, kWave);
      if (lane >= d) incl += t;
    }
    if (lane == kWave - 1) s_cnt[wv] = incl;
    __syncthreads();
    int at = nmark + incl - cnt;
    for (int w2 = 0; w2 < wv; ++w2) at += s_cnt[w2];
    const int total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
#pragma unroll 1
    for (int j = 0; j < 16; ++j) {
      if ((mk >> j) & 1u) {
        if (at < cap) mp[at] = (int)o + j;
        ++at;
      }
    }
    nmark += total;
    __syncthreads();  // s_min / s_cnt are rewritten by the next step
    if (first != 0x7fffffff) {
      eoi = true;
      break;
    }
  }
  if (tid == 0) {
    const int present = eoi ? nmark : nmark + 1;
    T->info.nmark = nmark;
    T->info.present = present;
    T->info.err = (eoi ? 0 : JD_E_NOEOI) | (present != T->info.expected ? JD_E_INTERVALS : 0);
  }
}

__global__ __launch_bounds__(kWave) void jpeg_decode_kernel(
    const uint8_t* __restrict__ files, uint8_t* __restrict__ tables,
    const int* __restrict__ mpos, uint8_t* __restrict__ planes, long long row_bytes, int H,
    int W, int max_int, int L, long long pitch, long long plane_bytes,
    const int* __restrict__ done, int* __restrict__ paths) {
  __shared__ __attribute__((aligned(16))) JdTables s_t;
  extern __shared__ __attribute__((aligned(16))) int16_t s_coef[];  // [6][64][L]
  const int lane = (int)threadIdx.x;
  const int n = (int)row_bytes;
  const long long img = blockIdx.y;
  JdTables* T = reinterpret_cast<JdTables*>(tables + img * sizeof(JdTables));
  const int k0 = (int)blockIdx.x * L;
  // (err is rewritten by other waves' entropy errors: only its header bits are read here)
  if ((T->info.err & JD_HDR_ERRORS) || k0 >= T->info.expected) return;
  {
    const uint4* src = reinterpret_cast<const uint4*>(T);
    uint4* dst = reinterpret_cast<uint4*>(&s_t);
    for (int i = lane; i < (int)(sizeof(JdTables) / 16); i += kWave) dst[i] = src[i];
  }
  __syncthreads();
  const JdInfo& I = s_t.info;
  const int hs = I.hs & 3, vs = I.vs & 3, ny = hs * vs, bpm = ny + 2;  // 3, 4 or 6 blocks
  const int mw = I.mw, mcus = I.mw * I.mh, ri = I.ri;
  const int iters = ri ? ri : mcus;
  const int k = k0 + lane;
  bool mine = lane < L && k < I.expected;
  if (done) {  // the split launches ran first: 0 not theirs, 1 completed, else handed back
    const int d = mine && k < max_int ? done[img * max_int + k] : 0;
    if (d) atomicAdd(&paths[2 * img + (d == 1 ? 0 : 1)], 1);
    if (d == 1) mine = false;
    if (!__syncthreads_or(mine)) return;
  }
  bool failed = !mine || k >= I.present;
  const uint8_t* row = files + img * row_bytes;
  const int* mp = mpos + img * max_int;
  int start = 0, stop = 0;
  if (!failed) jd_interval(I, mp, k, n, max_int, start, stop);
  JdReader rd(row, start, stop);
  int pred[3] = {0, 0, 0};
  bool bad = false;  // this lane met an entropy error
  uint8_t* pl = planes + img * 3 * plane_bytes;
  const JdHuff* dcs[3] = {&s_t.h[I.td[0] & 1], &s_t.h[I.td[1] & 1], &s_t.h[I.td[2] & 1]};
  const JdHuff* acs[3] = {&s_t.h[2 + (I.ta[0] & 1)], &s_t.h[2 + (I.ta[1] & 1)],
                          &s_t.h[2 + (I.ta[2] & 1)]};
  int16_t* my = s_coef + lane;  // element (b, c) at (b * 64 + c) * L

#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
    // zero the wave's coefficients: each lane its own column, so no barrier is needed
    if (lane < L)
      for (int i = 0; i < bpm * 64; ++i) my[i * L] = 0;
    const long long m = ri ? (long long)k * ri + it : it;
    if (!mine || m >= mcus) continue;
    const int mx = (int)(m % mw), myr = (int)(m / mw);
    if (!failed) {
#pragma unroll 1
      for (int b = 0; b < bpm; ++b) {
        const int c = b < ny ? 0 : b - ny + 1;
        int16_t* blk = my + b * 64 * L;
        if (jd_decode_block(rd, *dcs[c], *acs[c], pred[c], blk, L)) {
          failed = bad = true;
          // the block the error is in and every block before it in this MCU stay as decoded
          // only if complete: the failing block is zeroed, the later ones still are
          for (int i = 0; i < 64; ++i) blk[i * L] = 0;
          break;
        }
      }
    }
#pragma unroll 1
    for (int b = 0; b < bpm; ++b) {
      const int c = b < ny ? 0 : b - ny + 1;
      const int by = c == 0 ? myr * vs + b / hs : myr;
      const int bx = c == 0 ? mx * hs + b % hs : mx;
      uint8_t* dst = pl + c * plane_bytes + (long long)by * 8 * pitch + bx * 8;
      jd_idct_block(my + b * 64 * L, L, s_t.q[I.tq[c] & 3], dst, pitch);
    }
  }
  if (bad) atomicOr(&T->info.err, (int)JD_E_ENTROPY);
}

// ---- long restart intervals: one lane per kJdSplitBytes subsequence (jpeg_decode_core.h) ----
// Per-file scratch `split`: a header (lanes in use, most sync rounds of a workgroup, seam
// rounds, seam passes, then kJdRoundBins counts of spec workgroups by their sync rounds, the
// last bin open-ended) and ten int32 arrays of maxl lanes.
constexpr int kJdRoundBins = 12;
constexpr int kJdSplitHdr = 4 + kJdRoundBins;
constexpr int kJdSplitArrays = 10;
enum { SP_K, SP_BEG, SP_SB, SP_SS, SP_EB, SP_ES, SP_NB, SP_D0, SP_D1, SP_D2 };
constexpr int kJdSplitLanes = kWave;  // lanes of a spec / write workgroup
constexpr int kJdSeamRounds = 8;
constexpr int kJdPlanThreads = 256;
enum { JD_DONE_SERIAL = 0, JD_DONE_PARALLEL = 1, JD_DONE_BACK = 2, JD_DONE_PENDING = 3 };

struct JdSplit {  // one file's view of the scratch
  int* hdr;
  int* a[kJdSplitArrays];
  __device__ JdSplit(int* split, long long img, int maxl) {
    hdr = split + img * (kJdSplitHdr + (long long)kJdSplitArrays * maxl);
#pragma unroll
    for (int i = 0; i < kJdSplitArrays; ++i) a[i] = hdr + kJdSplitHdr + (long long)i * maxl;
  }
  __device__ JdState start(int l) const { return JdState{a[SP_SB][l], a[SP_SS][l]}; }
  __device__ JdState end(int l) const { return JdState{a[SP_EB][l], a[SP_ES][l]}; }
  __device__ void put(int l, const JdState& from, const JdLaneSums& o) const {
    a[SP_SB][l] = from.byte; a[SP_SS][l] = from.sub;
    a[SP_EB][l] = o.end.byte; a[SP_ES][l] = o.end.sub;
    a[SP_NB][l] = o.nblk;
    a[SP_D0][l] = (int)o.dc[0]; a[SP_D1][l] = (int)o.dc[1]; a[SP_D2][l] = (int)o.dc[2];
  }
};
__device__ __forceinline__ void jd_copy_tables(const JdTables* T, JdTables* s_t, int tid, int nt) {
  const uint4* src = reinterpret_cast<const uint4*>(T);
  uint4* dst = reinterpret_cast<uint4*>(s_t);
  for (int i = tid; i < (int)(sizeof(JdTables) / 16); i += nt) dst[i] = src[i];
}
__device__ __forceinline__ int jd_lane_bound(int beg, int istop) {
  return min((beg / kJdSplitBytes + 1) * kJdSplitBytes, istop);
}

// plan: one workgroup per file.  Every interval longer than thresh bytes gets one lane per
// subsequence it touches (a workgroup prefix sum of the counts places them) and is marked
// pending in done; every other interval stays the serial walk's.  Clears paths.
__global__ __launch_bounds__(kJdPlanThreads) void jpeg_plan_kernel(
    const uint8_t* __restrict__ tables, const int* __restrict__ mpos, int* __restrict__ split,
    int* __restrict__ done, int* __restrict__ paths, long long row_bytes, int max_int, int maxl,
    int thresh) {
  __shared__ int s_cnt[kJdPlanThreads / kWave];
  __shared__ int s_b[kJdPlanThreads], s_n[kJdPlanThreads], s_st[kJdPlanThreads];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
  const long long img = blockIdx.x;
  const JdInfo& I = reinterpret_cast<const JdTables*>(tables + img * sizeof(JdTables))->info;
  const JdSplit sp(split, img, maxl);
  const int* mp = mpos + img * max_int;
  int* dn = done + img * max_int;
  if (tid < 2) paths[2 * img + tid] = 0;
  if (tid < kJdSplitHdr) sp.hdr[tid] = 0;
  if (I.err & JD_HDR_ERRORS) return;
  const int all = min(I.expected, max_int), live = min(all, I.present);
  int carry = 0;  // lanes placed so far (uniform)
  for (int k0 = 0; k0 < all; k0 += kJdPlanThreads) {
    const int k = k0 + tid;
    int start = 0, stop = 0, nsub = 0;
    if (k < live) {
      jd_interval(I, mp, k, (int)row_bytes, max_int, start, stop);
      if (stop - start > thresh) nsub = (stop - 1) / kJdSplitBytes - start / kJdSplitBytes + 1;
    }
    int incl = nsub;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
      const int t = __shfl_up(incl, d, kWave);
      if (lane >= d) incl += t;
    }
    if (lane == kWave - 1) s_cnt[wv] = incl;
    __syncthreads();
    int base = carry + incl - nsub;
    for (int w2 = 0; w2 < wv; ++w2) base += s_cnt[w2];
    const int total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (base + nsub > maxl) nsub = 0;  // cannot happen: maxl holds every interval longer than S
    if (k < all) dn[k] = nsub ? JD_DONE_PENDING : JD_DONE_SERIAL;
    s_b[tid] = base; s_n[tid] = nsub; s_st[tid] = start;
    __syncthreads();
    if (total) {
      for (int q = 0; q < kJdPlanThreads; ++q) {
        const int nq = s_n[q], st = s_st[q];
        for (int j = tid; j < nq; j += kJdPlanThreads) {
          sp.a[SP_K][s_b[q] + j] = k0 + q;
          sp.a[SP_BEG][s_b[q] + j] = j ? (st / kJdSplitBytes + j) * kJdSplitBytes : st;
        }
      }
    }
    carry = min(carry + total, maxl);
    __syncthreads();
  }
  if (tid == 0) sp.hdr[0] = carry;
}

// What a lane is: its interval and the row bytes [beg, bound) of its subsequence.
struct JdLane {
  int k, beg, istart, istop, bound;
  __device__ JdLane(const JdSplit& sp, const JdInfo& I, const int* mp, int l, int n, int max_int) {
    k = min(max(sp.a[SP_K][l], 0), max_int - 1);
    jd_interval(I, mp, k, n, max_int, istart, istop);
    beg = min(max(sp.a[SP_BEG][l], istart), max(istop - 1, istart));
    bound = jd_lane_bound(beg, istop);
  }
  __device__ bool first() const { return beg == istart; }
};

// speculate + synchronise: kJdSplitLanes lanes of one file per workgroup, its tables in LDS.
// Every lane walks its subsequence from the cold state (the interval's first lane from the
// true one), then the lanes pass end states down through LDS, a lane decoding again whenever
// the lane before it ended somewhere else, until none changed: at most one round per lane,
// after which the workgroup is consistent with its first lane.  No pixels are written.
__global__ __launch_bounds__(kJdSplitLanes) void jpeg_spec_kernel(
    const uint8_t* __restrict__ files, const uint8_t* __restrict__ tables,
    const int* __restrict__ mpos, int* __restrict__ split, long long row_bytes, int max_int,
    int maxl) {
  __shared__ __attribute__((aligned(16))) JdTables s_t;
  __shared__ JdState s_end[kJdSplitLanes];
  const int lane = (int)threadIdx.x;
  const long long img = blockIdx.y;
  const JdSplit sp(split, img, maxl);
  const int nl = min(sp.hdr[0], maxl), l = (int)blockIdx.x * kJdSplitLanes + lane;
  if ((int)blockIdx.x * kJdSplitLanes >= nl) return;
  jd_copy_tables(reinterpret_cast<const JdTables*>(tables + img * sizeof(JdTables)), &s_t, lane,
                 kJdSplitLanes);
  s_end[lane] = JdState{-1, 0};
  __syncthreads();
  const uint8_t* row = files + img * row_bytes;
  const bool active = l < nl;
  const JdLane ln(sp, s_t.info, mpos + img * max_int, active ? l : 0, (int)row_bytes, max_int);
  JdState from = jd_lane_cold(row, ln.istart, ln.beg);
  JdLaneSums o;
  bool need = active;
  int rounds = 0;
  for (int r = 0; r < kJdSplitLanes; ++r) {
    if (need) {
      jd_lane_count(row, s_t, ln.istart, ln.istop, from, ln.bound, o);
      s_end[lane] = o.end;
    }
    __syncthreads();
    need = false;
    if (active && lane > 0 && !ln.first()) {
      const JdState prev = s_end[lane - 1];
      if (prev.byte >= 0 && !jd_same(prev, from)) {
        from = prev;
        need = true;
      }
    }
    if (!__syncthreads_or(need)) break;
    ++rounds;
  }
  if (need) o.end.byte = -1;  // (the cap is one round per lane: not reached with a change left)
  if (active) sp.put(l, from, o);
  if (lane == 0) {
    atomicMax(&sp.hdr[1], rounds);
    atomicAdd(&sp.hdr[4 + min(rounds, kJdRoundBins - 1)], 1);
  }
}

// stitch: one workgroup per file.  First the seams between the spec workgroups: where a
// workgroup's first lane did not start at the end state of the lane before it, one thread
// decodes that workgroup's lanes again, one after the other, until an end state meets the start
// the next lane already has.  Even and odd seams take turns, so nobody reads a lane that is
// being rewritten; the rounds repeat until no seam moved, kJdSeamRounds at most.  Then the
// chain check (every lane starts exactly where the one before it ended, the interval's first
// at the true state) and, per interval, the exclusive prefix sums of the block counts and the
// DC sums, which give every lane its first block and its predictors.  An interval whose chain
// holds and whose blocks add up to the expected count is marked completed in done, any other
// handed back.  Nothing here waits for another workgroup.
__global__ __launch_bounds__(kJdPlanThreads) void jpeg_stitch_kernel(
    const uint8_t* __restrict__ files, const uint8_t* __restrict__ tables,
    const int* __restrict__ mpos, int* split, int* __restrict__ done, long long row_bytes,
    int max_int, int maxl) {
  __shared__ __attribute__((aligned(16))) JdTables s_t;
  __shared__ int s_v[5][kJdPlanThreads], s_f[kJdPlanThreads], s_passes;
  const int tid = (int)threadIdx.x, n = (int)row_bytes;
  const long long img = blockIdx.x;
  const JdSplit sp(split, img, maxl);
  const int nl = min(sp.hdr[0], maxl);
  if (nl == 0) return;
  jd_copy_tables(reinterpret_cast<const JdTables*>(tables + img * sizeof(JdTables)), &s_t, tid,
                 kJdPlanThreads);
  if (tid == 0) s_passes = 0;
  __syncthreads();
  const JdInfo& I = s_t.info;
  const uint8_t* row = files + img * row_bytes;
  const int* mp = mpos + img * max_int;
  const int nwg = (nl + kJdSplitLanes - 1) / kJdSplitLanes;
  int rounds = 0;
  for (int r = 0; r < kJdSeamRounds; ++r) {
    int moved = 0;
    for (int half = 0; half < 2; ++half) {
      for (int s = 1 + half + 2 * tid; s < nwg; s += 2 * kJdPlanThreads) {
        const int f = s * kJdSplitLanes, stop = min(f + kJdSplitLanes, nl);
        const JdLane l0(sp, I, mp, f, n, max_int);
        if (l0.first()) continue;
        JdState e = sp.end(f - 1);
        for (int l = f; l < stop && e.byte >= 0; ++l) {
          const JdLane ln(sp, I, mp, l, n, max_int);
          if (ln.k != l0.k || jd_same(sp.start(l), e)) break;
          JdLaneSums o;
          jd_lane_count(row, s_t, ln.istart, ln.istop, e, ln.bound, o);
          sp.put(l, e, o);
          e = o.end;
          ++moved;
        }
      }
      __syncthreads();
    }
    if (moved) atomicAdd(&s_passes, moved);
    if (!__syncthreads_or(moved)) break;
    ++rounds;
  }
  if (tid == 0) {
    sp.hdr[2] = rounds;
    sp.hdr[3] = s_passes;
  }
  int carry[5] = {0, 0, 0, 0, 0};  // the running interval's sums before this tile (uniform)
  for (int l0 = 0; l0 < nl; l0 += kJdPlanThreads) {
    const int l = l0 + tid;
    int v[5] = {0, 0, 0, 0, 0}, head = 1, tail = 0, k = 0;
    if (l < nl) {
      const JdLane ln(sp, I, mp, l, n, max_int);
      k = ln.k;
      head = ln.first();
      tail = ln.bound == ln.istop;
      const JdState from = sp.start(l);
      const JdState want = head ? JdState{ln.istart, 0} : sp.end(l - 1);
      v[0] = sp.a[SP_NB][l]; v[1] = sp.a[SP_D0][l]; v[2] = sp.a[SP_D1][l]; v[3] = sp.a[SP_D2][l];
      v[4] = (want.byte < 0 || !jd_same(from, want)) ? 1 : 0;
    }
    const int own[4] = {v[0], v[1], v[2], v[3]};
    if (tid == 0 && !head)
      for (int i = 0; i < 5; ++i) v[i] = (int)((unsigned)v[i] + (unsigned)carry[i]);
    for (int i = 0; i < 5; ++i) s_v[i][tid] = v[i];
    s_f[tid] = head;
    __syncthreads();
    for (int d = 1; d < kJdPlanThreads; d <<= 1) {  // segmented inclusive scan
      int t[5] = {0, 0, 0, 0, 0}, tf = 1;
      const bool take = tid >= d && !s_f[tid];
      if (take) {
        for (int i = 0; i < 5; ++i) t[i] = s_v[i][tid - d];
        tf = s_f[tid - d];
      }
      __syncthreads();
      if (take) {
        for (int i = 0; i < 5; ++i) s_v[i][tid] = (int)((unsigned)s_v[i][tid] + (unsigned)t[i]);
        s_f[tid] = tf;
      }
      __syncthreads();
    }
    if (l < nl) {
      sp.a[SP_NB][l] = s_v[0][tid] - own[0];
      sp.a[SP_D0][l] = (int)((unsigned)s_v[1][tid] - (unsigned)own[1]);
      sp.a[SP_D1][l] = (int)((unsigned)s_v[2][tid] - (unsigned)own[2]);
      sp.a[SP_D2][l] = (int)((unsigned)s_v[3][tid] - (unsigned)own[3]);
      if (tail)
        done[img * max_int + k] = s_v[4][tid] == 0 && s_v[0][tid] == jd_interval_blocks(I, k)
                                      ? JD_DONE_PARALLEL : JD_DONE_BACK;
    }
    for (int i = 0; i < 5; ++i) carry[i] = s_v[i][kJdPlanThreads - 1];
    __syncthreads();
  }
}

// write: the spec launch's lanes again, each from its verified state with its first block
// index and predictors.  A lane decodes the blocks whose DC symbol it read into its own LDS
// column [coefficient][lane], runs the IDCT and stores the block's samples.  Anything the serial
// walk would call an error hands the whole interval back.
__global__ __launch_bounds__(kJdSplitLanes) void jpeg_write_kernel(
    const uint8_t* __restrict__ files, const uint8_t* __restrict__ tables,
    const int* __restrict__ mpos, const int* __restrict__ split, int* done,
    uint8_t* __restrict__ planes, long long row_bytes, int max_int, int maxl, long long pitch,
    long long plane_bytes) {
  __shared__ __attribute__((aligned(16))) JdTables s_t;
  __shared__ int16_t s_coef[64 * kJdSplitLanes];
  const int lane = (int)threadIdx.x;
  const long long img = blockIdx.y;
  const JdSplit sp(const_cast<int*>(split), img, maxl);
  const int nl = min(sp.hdr[0], maxl), l = (int)blockIdx.x * kJdSplitLanes + lane;
  if ((int)blockIdx.x * kJdSplitLanes >= nl) return;
  jd_copy_tables(reinterpret_cast<const JdTables*>(tables + img * sizeof(JdTables)), &s_t, lane,
                 kJdSplitLanes);
  __syncthreads();
  if (l >= nl) return;
  const JdLane ln(sp, s_t.info, mpos + img * max_int, l, (int)row_bytes, max_int);
  int* dn = done + img * max_int + ln.k;
  if (*dn != JD_DONE_PARALLEL) return;
  const uint32_t pred[3] = {(uint32_t)sp.a[SP_D0][l], (uint32_t)sp.a[SP_D1][l],
                            (uint32_t)sp.a[SP_D2][l]};
  const int ri = s_t.info.ri;
  if (jd_lane_write(files + img * row_bytes, s_t, ln.istart, ln.istop, sp.start(l), ln.bound,
                    sp.a[SP_NB][l], jd_interval_blocks(s_t.info, ln.k), (long long)ln.k * ri, pred,
                    s_coef + lane, kJdSplitLanes, planes + img * 3 * plane_bytes, pitch,
                    plane_bytes))
    *dn = JD_DONE_BACK;
}

__global__ __launch_bounds__(kJdColourThreads) void jpeg_colour_kernel(
    const uint8_t* __restrict__ tables, const uint8_t* __restrict__ planes,
    uint8_t* __restrict__ out, int* __restrict__ status, int H, int W, long long pitch,
    long long plane_bytes, int vec_ok) {
  const long long img = blockIdx.y;
  const JdInfo& I = reinterpret_cast<const JdTables*>(tables + img * sizeof(JdTables))->info;
  const int err = I.err;
  const int w4 = (W + 3) >> 2;
  const long long t = (long long)blockIdx.x * kJdColourThreads + threadIdx.x;
  if (t == 0) status[img] = -err;
  if (t >= (long long)w4 * H) return;
  const int y = (int)(t / w4), x0 = (int)(t - (long long)y * w4) * 4;
  uint8_t* dst = out + (img * H + y) * (long long)W * 3 + (long long)x0 * 3;
  unsigned char px[12];
  if (err & JD_HDR_ERRORS) {
#pragma unroll
    for (int i = 0; i < 12; ++i) px[i] = 0;
  } else {
    const int hs = I.hs & 3, vs = I.vs & 3;
    const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
    const uint8_t* p0 = planes + img * 3 * plane_bytes;
    const unsigned yy = *reinterpret_cast<const unsigned*>(p0 + y * pitch + x0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int x = min(x0 + i, W - 1);
      const int cb = jd_chroma(p0 + plane_bytes, pitch, cw, ch, hs, vs, x, y);
      const int cr = jd_chroma(p0 + 2 * plane_bytes, pitch, cw, ch, hs, vs, x, y);
      int r, g, b;
      jd_rgb((int)((yy >> (8 * i)) & 255u), cb, cr, r, g, b);
      px[3 * i] = (unsigned char)r;
      px[3 * i + 1] = (unsigned char)g;
      px[3 * i + 2] = (unsigned char)b;
    }
  }
  if (vec_ok) {  // W % 4 == 0 and out is dword aligned: x0 + 3 < W
    unsigned* d = reinterpret_cast<unsigned*>(dst);
    d[0] = px[0] | px[1] << 8 | px[2] << 16 | (unsigned)px[3] << 24;
    d[1] = px[4] | px[5] << 8 | px[6] << 16 | (unsigned)px[7] << 24;
    d[2] = px[8] | px[9] << 8 | px[10] << 16 | (unsigned)px[11] << 24;
  } else {
    const int nb = min(4, W - x0) * 3;
    for (int i = 0; i < nb; ++i) dst[i] = px[i];
  }
}

}  // namespace
}  // namespace kvedge

using namespace kvedge;

extern "C" int kv_jpeg_decode_table_bytes(void) { return (int)sizeof(JdTables); }
extern "C" int kv_jpeg_decode_split_bytes(void) { return kJdSplitBytes; }
extern "C" long long kv_jpeg_decode_split_ints(long long row_bytes) {
  return kJdSplitHdr + (long long)kJdSplitArrays * jd_lanes_per_row(row_bytes);
}

namespace {
// mode 0: scan, decode, colour.  Else the split launches go between scan and decode, for
// intervals longer than kJdSplitBytes (mode 2) or kJdAutoSplitBytes (mode 1).  launches < 7
// stops after that many of scan, plan, spec, stitch, write, decode, colour: the probe times the
// prefixes to tell the launches apart; the output is then incomplete.
int jd_launch(const unsigned char* files, unsigned char* tables, int* mpos, unsigned char* planes,
              unsigned char* out, int* status, int* split, int* done, int* paths, int N,
              long long row_bytes, int H, int W, int lanes, int mode, int launches,
              hipStream_t s) {
  if (H < 1 || H > kJdMaxExtent || W < 1 || W > kJdMaxExtent) return -1;
  if (N < 0 || N > 65535) return -2;
  if (row_bytes < 16 || row_bytes > 0x7ffffff0ll || (row_bytes & 15)) return -3;
  if (lanes != 16 && lanes != 32 && lanes != 64) return -5;
  if (mode < 0 || mode > 2 || launches < 1 || launches > 7) return -6;
  if ((reinterpret_cast<uintptr_t>(files) & 15) || (reinterpret_cast<uintptr_t>(tables) & 15) ||
      (reinterpret_cast<uintptr_t>(planes) & 15) || (reinterpret_cast<uintptr_t>(mpos) & 3) ||
      (reinterpret_cast<uintptr_t>(status) & 3) || (reinterpret_cast<uintptr_t>(split) & 3) ||
      (reinterpret_cast<uintptr_t>(done) & 3) || (reinterpret_cast<uintptr_t>(paths) & 3))
    return -7;
  if (N == 0) return 0;
  const int max_int = ((H + 7) / 8) * ((W + 7) / 8);
  const int maxl = jd_lanes_per_row(row_bytes);
  const long long pitch = (W + 15) / 16 * 16, plane_bytes = pitch * ((H + 15) / 16 * 16);
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(files, (long long)N * row_bytes)) return -20;
  if (!rs_in_alloc(tables, (long long)N * (long long)sizeof(JdTables))) return -21;
  if (!rs_in_alloc(mpos, (long long)N * max_int * 4)) return -22;
  if (!rs_in_alloc(planes, (long long)N * 3 * plane_bytes)) return -23;
  if (!rs_in_alloc(out, (long long)N * H * W * 3)) return -24;
  if (!rs_in_alloc(status, (long long)N * 4)) return -25;
  if (mode) {
    if (!rs_in_alloc(split, (long long)N * kv_jpeg_decode_split_ints(row_bytes) * 4)) return -26;
    if (!rs_in_alloc(done, (long long)N * max_int * 4)) return -27;
    if (!rs_in_alloc(paths, (long long)N * 2 * 4)) return -28;
  }
#endif
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)N), dim3(kJdScanThreads), 0, s, files,
                     tables, mpos, row_bytes, H, W, max_int);
  if (hipGetLastError() != hipSuccess) return -100;
  if (--launches == 0) return 0;
  if (mode) {
    const int thresh = mode == 2 ? kJdSplitBytes : kJdAutoSplitBytes;
    const dim3 gl((unsigned)((maxl + kJdSplitLanes - 1) / kJdSplitLanes), (unsigned)N);
    hipLaunchKernelGGL(jpeg_plan_kernel, dim3((unsigned)N), dim3(kJdPlanThreads), 0, s, tables,
                       mpos, split, done, paths, row_bytes, max_int, maxl, thresh);
    if (hipGetLastError() != hipSuccess) return -100;
    if (--launches == 0) return 0;
    hipLaunchKernelGGL(jpeg_spec_kernel, gl, dim3(kJdSplitLanes), 0, s, files, tables, mpos,
                       split, row_bytes, max_int, maxl);
    if (hipGetLastError() != hipSuccess) return -100;
    if (--launches == 0) return 0;
    hipLaunchKernelGGL(jpeg_stitch_kernel, dim3((unsigned)N), dim3(kJdPlanThreads), 0, s, files,
                       tables, mpos, split, done, row_bytes, max_int, maxl);
    if (hipGetLastError() != hipSuccess) return -100;
    if (--launches == 0) return 0;
    hipLaunchKernelGGL(jpeg_write_kernel, gl, dim3(kJdSplitLanes), 0, s, files, tables, mpos,
                       split, done, planes, row_bytes, max_int, maxl, pitch, plane_bytes);
    if (hipGetLastError() != hipSuccess) return -100;
    if (--launches == 0) return 0;
  }
  const dim3 g2((unsigned)((max_int + lanes - 1) / lanes), (unsigned)N);
  hipLaunchKernelGGL(jpeg_decode_kernel, g2, dim3(kWave), (size_t)lanes * 6 * 64 * 2, s, files,
                     tables, mpos, planes, row_bytes, H, W, max_int, lanes, pitch, plane_bytes,
                     mode ? done : nullptr, mode ? paths : nullptr);
  if (hipGetLastError() != hipSuccess) return -100;
  if (--launches == 0) return 0;
  const int vec_ok = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(out) % 4 == 0);
  const long long threads = (long long)((W + 3) / 4) * H;
  const dim3 g3((unsigned)((threads + kJdColourThreads - 1) / kJdColourThreads), (unsigned)N);
  hipLaunchKernelGGL(jpeg_colour_kernel, g3, dim3(kJdColourThreads), 0, s, tables, planes, out,
                     status, H, W, pitch, plane_bytes, vec_ok);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}
}  // namespace

extern "C" int kv_jpeg_decode(const unsigned char* files, unsigned char* tables, int* mpos,
                              unsigned char* planes, unsigned char* out, int* status, int N,
                              long long row_bytes, int H, int W, int lanes, hipStream_t s) {
  return jd_launch(files, tables, mpos, planes, out, status, nullptr, nullptr, nullptr, N,
                   row_bytes, H, W, lanes, 0, 7, s);
}

extern "C" int kv_jpeg_decode_split(const unsigned char* files, unsigned char* tables, int* mpos,
                                    unsigned char* planes, unsigned char* out, int* status,
                                    int* split, int* done, int* paths, int N, long long row_bytes,
                                    int H, int W, int lanes, int mode, int launches,
                                    hipStream_t s) {
  if (mode && (!split || !done || !paths)) return -7;
  return jd_launch(files, tables, mpos, planes, out, status, split, done, paths, N, row_bytes, H,
                   W, lanes, mode, launches, s);
}
