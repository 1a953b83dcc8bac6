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
    int W, int max_int, int L, long long pitch, long long plane_bytes) {
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
  const bool mine = lane < L && k < I.expected;
  bool failed = !mine || k >= I.present;
  const uint8_t* row = files + img * row_bytes;
  const int* mp = mpos + img * max_int;
  int start = 0, stop = 0;
  if (!failed) {
    const int cap = min(I.expected, max_int);
    // offsets read from scratch the scan wrote from the file: clamped to the row
    start = k == 0 ? I.e0 : min(max(mp[min(k - 1, cap - 1)] + 2, 0), n);
    stop = k < I.nmark ? min(max(mp[min(k, cap - 1)], 0), n) : n;
    stop = max(stop, start);
  }
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

extern "C" int kv_jpeg_decode(const unsigned char* files, unsigned char* tables, int* mpos,
                              unsigned char* planes, unsigned char* out, int* status, int N,
                              long long row_bytes, int H, int W, int lanes, hipStream_t s) {
  if (H < 1 || H > kJdMaxExtent || W < 1 || W > kJdMaxExtent) return -1;
  if (N < 0 || N > 65535) return -2;
  if (row_bytes < 16 || row_bytes > 0x7ffffff0ll || (row_bytes & 15)) return -3;
  if (lanes != 16 && lanes != 32 && lanes != 64) return -5;
  if ((reinterpret_cast<uintptr_t>(files) & 15) || (reinterpret_cast<uintptr_t>(tables) & 15) ||
      (reinterpret_cast<uintptr_t>(planes) & 15) || (reinterpret_cast<uintptr_t>(mpos) & 3) ||
      (reinterpret_cast<uintptr_t>(status) & 3))
    return -7;
  if (N == 0) return 0;
  const int max_int = ((H + 7) / 8) * ((W + 7) / 8);
  const long long pitch = (W + 15) / 16 * 16, plane_bytes = pitch * ((H + 15) / 16 * 16);
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(files, (long long)N * row_bytes)) return -20;
  if (!rs_in_alloc(tables, (long long)N * (long long)sizeof(JdTables))) return -21;
  if (!rs_in_alloc(mpos, (long long)N * max_int * 4)) return -22;
  if (!rs_in_alloc(planes, (long long)N * 3 * plane_bytes)) return -23;
  if (!rs_in_alloc(out, (long long)N * H * W * 3)) return -24;
  if (!rs_in_alloc(status, (long long)N * 4)) return -25;
#endif
  hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)N), dim3(kJdScanThreads), 0, s, files,
                     tables, mpos, row_bytes, H, W, max_int);
  if (hipGetLastError() != hipSuccess) return -100;
  const dim3 g2((unsigned)((max_int + lanes - 1) / lanes), (unsigned)N);
  hipLaunchKernelGGL(jpeg_decode_kernel, g2, dim3(kWave), (size_t)lanes * 6 * 64 * 2, s, files,
                     tables, mpos, planes, row_bytes, H, W, max_int, lanes, pitch, plane_bytes);
  if (hipGetLastError() != hipSuccess) return -100;
  const int vec_ok = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(out) % 4 == 0);
  const long long threads = (long long)((W + 3) / 4) * H;
  const dim3 g3((unsigned)((threads + kJdColourThreads - 1) / kJdColourThreads), (unsigned)N);
  hipLaunchKernelGGL(jpeg_colour_kernel, g3, dim3(kJdColourThreads), 0, s, tables, planes, out,
                     status, H, W, pitch, plane_bytes, vec_ok);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}
