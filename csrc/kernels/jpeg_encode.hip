// K21 (JPEG snapshots): uint8 RGB images already in device memory -> baseline JPEG files in
// device memory, no host in the loop, capturable.  Three launches on one stream; every table
// (quantisation, Huffman, the file header) lives in device memory and is read at run time, so
// a new quality takes effect on the next replay of a captured step.
//
// The format (ops.reference.jpeg_encode is THE definition; all integer, byte-identical):
//   colour   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
//            Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
//            Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
//   padding  to whole MCUs (8 x 8 for 4:4:4, 16 x 16 for 4:2:0) by replicating the last column
//            and row; 4:2:0 chroma = (a + b + c + d + 2) >> 2 over each 2 x 2
//   DCT      level shift by 128, Loeffler-Ligtenberg-Moschytz 8-point passes in 13-bit fixed
//            point: rows first (2 extra bits kept), then columns; outputs scaled by 8
//   quantise q = sign(c) * ((|c| + 4 Q) / (8 Q)), DC clamped to +-1024, AC to +-1023
//   scan     one interleaved scan (Y00 Y01 Y10 Y11 Cb Cr per MCU for 4:2:0, Y Cb Cr for 4:4:4),
//            restart interval = one MCU row, DC prediction from 0 in every interval, the four
//            Annex K Huffman tables, ZRL for zero runs above 15, EOB unless coefficient 63 is
//            nonzero, intervals padded with 1-bits to a byte, FF stuffed as FF 00
//   file     header (611 bytes: SOI DQT DQT SOF0 DHT x4 DRI SOS) | interval 0 | RST0 |
//            interval 1 | RST1 | ... (RSTn cycling 0..7) | EOI
//
// Launches:
//   blocks   one workgroup = a strip of 128 padded pixel columns of one MCU row of one image
//            (8 MCUs of 4:2:0, 16 of 4:4:4: 48 blocks either way).  A thread converts a 4 x 2
//            (4:2:0) or 4 x 1 (4:4:4) pixel patch, read as three dwords per row where the
//            image allows, into level-shifted int16 Y / Cb / Cr planes in LDS; then one thread
//            per (block, row) runs the row pass into an int32 LDS tile, one thread per
//            (block, column) the column pass and the quantiser into a zigzag int16 LDS image,
//            and the strip's blocks -- contiguous in scan order -- leave as 16-byte stores.
//   entropy  one wavefront per restart interval, 64 blocks at a time, one block per lane.  A
//            lane counts its bits, a wave prefix sum gives it its bit offset, and it writes
//            its codes MSB first into an LDS chunk buffer of big-endian dwords: plain stores
//            for the dwords wholly its own, atomicOr for its first and last.  The wave then
//            walks the chunk's whole bytes, 64 at a time, and writes them with FF 00 stuffing
//            (ballot / popcount prefix) to the interval's scratch segment.  The chunk's
//            partial last byte and the segment offset carry into the next chunk.
//   pack     one workgroup per image: prefix sum of the interval lengths, then header,
//            segments, RSTn markers and EOI are copied into the image's output row, or only
//            length = -needed is written when the file does not fit the row.
#include "common.h"
#include "kvedge_kernels.h"
#include "resample.h"  // rs_in_alloc

namespace kvedge {
namespace {

constexpr int kJpMaxExtent = 8192;
constexpr int kJpHeader = 611;
constexpr int kJpBlockBits = 22 + 63 * 26;                    // DC 11 + 11, AC 63 x (16 + 10)
constexpr int kJpBlockBytes = 2 * ((kJpBlockBits + 7) / 8);   // every byte stuffed: 416
constexpr int kJpStripPx = 128, kJpStripBlocks = 48, kJpThreads = 256;
// the chunk buffer holds 64 blocks whatever the Huffman tables in device memory say: a code
// length is clamped to 16, so a block is at most (16 + 11) + 63 x 26 bits; + 7 carried bits
constexpr int kJpChunkDwords = (kWave * (kJpBlockBits + 5) + 7 + 31) / 32 + 1;
constexpr int kJpPackThreads = 256;
constexpr int kJpMaxIntervals = kJpMaxExtent / 8;             // 1024 = 4 per pack thread

__device__ const unsigned char kJpNatToZig[64] = {
    0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
    41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
    46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

__device__ __forceinline__ int jp_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 8-point pass; FIRST: the row pass (2 extra bits), else the column pass
template <bool FIRST>
__device__ __forceinline__ void jp_dct8(const int (&d)[8], int (&o)[8]) {
  constexpr int SH = FIRST ? 11 : 15;
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  if constexpr (FIRST) {
    o[0] = (t10 + t11) * 4;  // (<< 2 of a possibly negative value)
    o[4] = (t10 - t11) * 4;
  } else {
    o[0] = jp_descale(t10 + t11, 2);
    o[4] = jp_descale(t10 - t11, 2);
  }
  int z1 = (t12 + t13) * 4433;
  o[2] = jp_descale(z1 + t13 * 6270, SH);
  o[6] = jp_descale(z1 - t12 * 15137, SH);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
  z1 *= -7373;
  z2 *= -20995;
  z3 = z3 * -16069 + z5;
  z4 = z4 * -3196 + z5;
  o[7] = jp_descale(u4 + z1 + z3, SH);
  o[5] = jp_descale(u5 + z2 + z4, SH);
  o[3] = jp_descale(u6 + z2 + z3, SH);
  o[1] = jp_descale(u7 + z1 + z4, SH);
}

__device__ __forceinline__ void jp_ycc(int r, int g, int b, int& y, int& cb, int& cr) {
  y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// S420: planes Y [16][128], Cb / Cr [8][64] (pitch 128 all); else Y / Cb / Cr [8][128]
template <bool S420>
__global__ __launch_bounds__(kJpThreads) void jpeg_blocks_kernel(
    const uint8_t* __restrict__ img, const int* __restrict__ qtab, short* __restrict__ coef,
    int H, int W, int mw, int mh, int vec_ok) {
  constexpr int MCU = S420 ? 16 : 8, BPM = S420 ? 6 : 3;
  constexpr int MCUS = kJpStripPx / MCU;  // MCUs per strip
  __shared__ short s_pl[3][16][kJpStripPx];
  __shared__ int s_row[kJpStripBlocks][64];
  __shared__ __attribute__((aligned(16))) short s_zz[kJpStripBlocks][64];
  __shared__ int s_q[2][64];
  const int tid = (int)threadIdx.x;
  const int strip = (int)blockIdx.x, my = (int)blockIdx.y, m = (int)blockIdx.z;
  const uint8_t* src = img + (long long)m * H * W * 3;
  if (tid < 128) s_q[tid >> 6][tid & 63] = min(max(qtab[tid], 1), 255);

  // colour conversion: thread = 4 columns x (2 | 1) rows; every coordinate is clamped into
  // the image, which both replicates the edges and keeps every read inside it
  {
    constexpr int PR = S420 ? 2 : 1;
    const int px = (tid & 31) * 4, py = (tid >> 5) * PR;  // 32 x 8 patches
    const int gx = strip * kJpStripPx + px, gy = my * MCU + py;
    int cbs[2] = {0, 0}, crs[2] = {0, 0};
#pragma unroll
    for (int r = 0; r < PR; ++r) {
      const int sy = min(gy + r, H - 1);
      const uint8_t* row = src + (long long)sy * W * 3;
      unsigned w0, w1, w2;
      if (vec_ok && gx + 3 < W) {
        const unsigned* p = reinterpret_cast<const unsigned*>(row + gx * 3);
        w0 = p[0]; w1 = p[1]; w2 = p[2];
      } else {
        unsigned char b[12];
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const uint8_t* q = row + min(gx + x, W - 1) * 3;
          b[3 * x] = q[0]; b[3 * x + 1] = q[1]; b[3 * x + 2] = q[2];
        }
        w0 = b[0] | b[1] << 8 | b[2] << 16 | (unsigned)b[3] << 24;
        w1 = b[4] | b[5] << 8 | b[6] << 16 | (unsigned)b[7] << 24;
        w2 = b[8] | b[9] << 8 | b[10] << 16 | (unsigned)b[11] << 24;
      }
      const int R[4] = {(int)(w0 & 255), (int)(w0 >> 24), (int)((w1 >> 16) & 255),
                        (int)((w2 >> 8) & 255)};
      const int G[4] = {(int)((w0 >> 8) & 255), (int)(w1 & 255), (int)(w1 >> 24),
                        (int)((w2 >> 16) & 255)};
      const int B[4] = {(int)((w0 >> 16) & 255), (int)((w1 >> 8) & 255), (int)(w2 & 255),
                        (int)(w2 >> 24)};
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        int y, cb, cr;
        jp_ycc(R[x], G[x], B[x], y, cb, cr);
        s_pl[0][py + r][px + x] = (short)(y - 128);
        if constexpr (S420) {
          cbs[x >> 1] += cb;
          crs[x >> 1] += cr;
        } else {
          s_pl[1][py][px + x] = (short)(cb - 128);
          s_pl[2][py][px + x] = (short)(cr - 128);
        }
      }
    }
    if constexpr (S420) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        s_pl[1][py >> 1][(px >> 1) + h] = (short)(((cbs[h] + 2) >> 2) - 128);
        s_pl[2][py >> 1][(px >> 1) + h] = (short)(((crs[h] + 2) >> 2) - 128);
      }
    }
  }
  __syncthreads();

  const int mcu0 = strip * MCUS;
  const int nblk = min(MCUS, mw - mcu0) * BPM;  // >= BPM: the grid has no empty strip
  // block b of the strip: its plane and the top-left sample in it
  auto origin = [](int b, int& pl, int& r0, int& c0) {
    const int mc = b / BPM, k = b - mc * BPM;
    if constexpr (S420) {
      pl = k < 4 ? 0 : k - 3;
      r0 = k < 4 ? (k >> 1) * 8 : 0;
      c0 = k < 4 ? mc * 16 + (k & 1) * 8 : mc * 8;
    } else {
      pl = k;
      r0 = 0;
      c0 = mc * 8;
    }
  };
  for (int t = tid; t < nblk * 8; t += kJpThreads) {
    const int b = t >> 3, r = t & 7;
    int pl, r0, c0;
    origin(b, pl, r0, c0);
    int d[8], o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = s_pl[pl][r0 + r][c0 + i];
    jp_dct8<true>(d, o);
#pragma unroll
    for (int i = 0; i < 8; ++i) s_row[b][r * 8 + i] = o[i];
  }
  __syncthreads();
  for (int t = tid; t < nblk * 8; t += kJpThreads) {
    const int b = t >> 3, c = t & 7;
    const int k = b % BPM;
    const int* q = s_q[(S420 ? k >= 4 : k >= 1) ? 1 : 0];
    int d[8], o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) d[i] = s_row[b][i * 8 + c];
    jp_dct8<false>(d, o);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int n = i * 8 + c;
      const unsigned Q = (unsigned)q[n];
      const int a = (int)(((unsigned)abs(o[i]) + 4u * Q) / (8u * Q));
      const int lim = n == 0 ? 1024 : 1023;
      const int v = min(a, lim);
      s_zz[b][kJpNatToZig[n]] = (short)(o[i] < 0 ? -v : v);
    }
  }
  __syncthreads();
  // the strip's blocks are contiguous in scan order: nblk * 128 bytes from a 128-byte boundary
  const long long blk0 = ((long long)(m * mh + my) * mw + mcu0) * BPM;
  uint4* dst = reinterpret_cast<uint4*>(coef + blk0 * 64);
  const uint4* s4 = reinterpret_cast<const uint4*>(&s_zz[0][0]);
  for (int t = tid; t < nblk * 8; t += kJpThreads) dst[t] = s4[t];
}

// ---------------------------------------------------------------------------------------------
// entropy coder
// ---------------------------------------------------------------------------------------------
struct JpCount {
  int bits = 0;
  __device__ __forceinline__ void put(unsigned, int n) { bits += n; }
};

// MSB-first writer into big-endian dwords of an LDS buffer that was zeroed
struct JpWriter {
  unsigned* buf;
  int di, first, fill;
  unsigned cur;
  __device__ __forceinline__ JpWriter(unsigned* b, int bitpos)
      : buf(b), di(bitpos >> 5), first(bitpos >> 5), fill(bitpos & 31), cur(0) {}
  __device__ __forceinline__ void flush_full() {
    if (di == first) atomicOr(&buf[di], cur);  // shared with the lane before
    else buf[di] = cur;
    ++di;
  }
  __device__ __forceinline__ void put(unsigned v, int n) {  // n <= 27, v < 2^n
    if (n == 0) return;  // (a symbol the table does not have)
    const int room = 32 - fill;
    if (n < room) {
      cur |= v << (room - n);
      fill += n;
    } else {
      const int over = n - room;  // 0..26
      cur |= v >> over;
      flush_full();
      cur = over ? v << (32 - over) : 0u;
      fill = over;
    }
  }
  __device__ __forceinline__ void finish() {
    if (fill) atomicOr(&buf[di], cur);  // shared with the lane after
  }
};

__device__ __forceinline__ int jp_cat(int v) { return 32 - __clz(abs(v)); }  // 0 for 0
__device__ __forceinline__ unsigned jp_mag(int v, int s) {
  return (unsigned)(v < 0 ? v - 1 : v) & ((1u << s) - 1u);
}

// one block: DC difference against pred, then the AC run-length walk.  dc / ac: code |
// length << 16 by symbol (LDS).  A symbol and its magnitude bits leave as one put().
template <class Sink>
__device__ __forceinline__ void jp_code_block(const short* __restrict__ c, int pred,
                                              const unsigned* dc, const unsigned* ac,
                                              Sink& sink) {
  int run = 0;
#pragma unroll 1
  for (int g = 0; g < 8; ++g) {
    const uint4 w = reinterpret_cast<const uint4*>(c)[g];
    const unsigned u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int v = (int)(short)(u[j >> 1] >> ((j & 1) * 16));
      if (g == 0 && j == 0) {
        const int diff = v - pred;
        const int s = min(jp_cat(diff), 11);
        const unsigned e = dc[s];
        sink.put(((e & 0xffffu) << s) | jp_mag(diff, s), (int)(e >> 16) + s);
        continue;
      }
      if (v == 0) {
        ++run;
        continue;
      }
      while (run > 15) {
        const unsigned e = ac[0xf0];
        sink.put(e & 0xffffu, (int)(e >> 16));
        run -= 16;
      }
      const int s = min(jp_cat(v), 10);
      const unsigned e = ac[(run << 4) | s];
      sink.put(((e & 0xffffu) << s) | jp_mag(v, s), (int)(e >> 16) + s);
      run = 0;
    }
  }
  if (run) {
    const unsigned e = ac[0];
    sink.put(e & 0xffffu, (int)(e >> 16));
  }
}

template <bool S420>
__global__ __launch_bounds__(kWave) void jpeg_entropy_kernel(
    const short* __restrict__ coef, const int* __restrict__ huff, uint8_t* __restrict__ scratch,
    int* __restrict__ seglen, int nb, int mh, int seg_cap) {
  constexpr int BPM = S420 ? 6 : 3;
  __shared__ unsigned s_buf[kJpChunkDwords];
  __shared__ unsigned s_huff[4][256];
  const int lane = (int)threadIdx.x;
  const int iv = (int)blockIdx.x, m = (int)blockIdx.y;
  for (int i = lane; i < 4 * 256; i += kWave) {
    // a code of at most 16 bits and a length of 1..16 (0: no such symbol), whatever is stored
    const unsigned e = (unsigned)huff[i];
    s_huff[i >> 8][i & 255] = (e & 0xffffu) | (min(e >> 16, 16u) << 16);
  }
  const long long seg = (long long)m * mh + iv;
  const short* blocks = coef + seg * nb * 64;
  uint8_t* out = scratch + seg * seg_cap;
  int out_off = 0;       // stuffed bytes written so far
  unsigned carry = 0;    // the chunk's partial last byte (its bits from the MSB down) ...
  int carry_bits = 0;    // ... and how many of them
  __syncthreads();

  for (int base = 0; base < nb; base += kWave) {
    const int i = base + lane;
    const bool live = i < nb;
    const int k = live ? i % BPM : 0;
    const int comp = S420 ? (k < 4 ? 0 : k - 3) : k;
    // the previous block of the component in scan order; none in the interval's first MCU
    const int back = S420 ? (k == 0 ? 3 : k < 4 ? 1 : 6) : 3;
    const bool has_prev = S420 ? (k >= 1 && k < 4) || i >= 6 : i >= 3;
    const short* c = blocks + (long long)i * 64;
    const int pred = live && has_prev ? c[-back * 64] : 0;
    const unsigned* dc = s_huff[comp ? 1 : 0];
    const unsigned* ac = s_huff[comp ? 3 : 2];

    JpCount cnt;
    if (live) jp_code_block(c, pred, dc, ac, cnt);
    int incl = cnt.bits;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int t = __shfl_up(incl, o, kWave);
      if (lane >= o) incl += t;
    }
    const int total = carry_bits + __shfl(incl, kWave - 1, kWave);  // bits in the buffer
    const int start = carry_bits + incl - cnt.bits;

    for (int d = lane; d <= (total >> 5); d += kWave) s_buf[d] = d == 0 ? carry << 24 : 0u;
    __syncthreads();
    if (live) {
      JpWriter wr(s_buf, start);
      jp_code_block(c, pred, dc, ac, wr);
      wr.finish();
    }
    __syncthreads();

    const bool last = base + kWave >= nb;
    int nbytes = total >> 3;
    const int rem = total & 7;
    if (last && rem) {  // pad the interval's last byte with 1-bits
      if (lane == 0) atomicOr(&s_buf[nbytes >> 2], (0xffu >> rem) << (24 - 8 * (nbytes & 3)));
      ++nbytes;
      __syncthreads();
    }
    for (int j0 = 0; j0 < nbytes; j0 += kWave) {
      const int j = j0 + lane;
      const bool on = j < nbytes;
      const unsigned b = on ? (s_buf[j >> 2] >> (24 - 8 * (j & 3))) & 0xffu : 0u;
      const unsigned long long ff = __ballot(on && b == 0xffu);
      const int before = __popcll(ff & ((1ull << lane) - 1ull));
      const int at = out_off + lane + before;
      if (on && at < seg_cap) out[at] = (uint8_t)b;
      if (on && b == 0xffu && at + 1 < seg_cap) out[at + 1] = 0;
      out_off += min(kWave, nbytes - j0) + __popcll(ff);
    }
    if (!last) {
      carry_bits = rem;
      carry = rem ? (s_buf[nbytes >> 2] >> (24 - 8 * (nbytes & 3))) & 0xffu : 0u;
    }
    __syncthreads();  // the buffer is cleared next
  }
  if (lane == 0) seglen[seg] = out_off;
}

// ---------------------------------------------------------------------------------------------
// pack
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kJpPackThreads) void jpeg_pack_kernel(
    const uint8_t* __restrict__ scratch, const int* __restrict__ seglen,
    const uint8_t* __restrict__ header, uint8_t* __restrict__ out, int* __restrict__ length,
    int mh, int seg_cap, long long cap) {
  __shared__ long long s_off[kJpMaxIntervals + 1];
  __shared__ long long s_wave[kJpPackThreads / kWave];
  const int tid = (int)threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
  const int m = (int)blockIdx.x;
  const int* len = seglen + (long long)m * mh;
  // exclusive prefix sum of the segment lengths (each clamped to what a segment holds): 4
  // consecutive intervals per thread, a wave scan, then the waves' totals
  int v[4];
  long long sum = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = tid * 4 + q;
    v[q] = i < mh ? min(max(len[i], 0), seg_cap) : 0;
    sum += v[q];
  }
  long long incl = sum;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const long long t = __shfl_up(incl, o, kWave);
    if (lane >= o) incl += t;
  }
  if (lane == kWave - 1) s_wave[wv] = incl;
  __syncthreads();
  long long off = incl - sum;
  for (int w = 0; w < wv; ++w) off += s_wave[w];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = tid * 4 + q;
    if (i < mh) {
      s_off[i] = off;
      off += v[q];
      if (i == mh - 1) s_off[mh] = off;  // the total
    }
  }
  __syncthreads();
  // header | seg 0 | RST0 | seg 1 | ... | EOI
  const long long total = kJpHeader + s_off[mh] + 2ll * (mh - 1) + 2;
  if (total > cap) {
    if (tid == 0) length[m] = (int)-total;
    return;
  }
  uint8_t* dst = out + (long long)m * cap;
  for (int i = tid; i < kJpHeader; i += kJpPackThreads) dst[i] = header[i];
  for (int iv = 0; iv < mh; ++iv) {
    const long long at = kJpHeader + s_off[iv] + 2ll * iv;
    const int n = (int)(s_off[iv + 1] - s_off[iv]);
    const uint8_t* sp = scratch + ((long long)m * mh + iv) * seg_cap;
    if (iv && tid < 2) dst[at - 2 + tid] = tid ? (uint8_t)(0xd0 + ((iv - 1) & 7)) : 0xff;
    for (int i = tid; i < n; i += kJpPackThreads) dst[at + i] = sp[i];
  }
  if (tid < 2) dst[total - 2 + tid] = tid ? 0xd9 : 0xff;
  if (tid == 0) length[m] = (int)total;
}

}  // namespace
}  // namespace kvedge

using namespace kvedge;

extern "C" int kv_jpeg_header_bytes(void) { return kJpHeader; }
extern "C" int kv_jpeg_block_bytes(void) { return kJpBlockBytes; }

extern "C" int kv_jpeg_encode(const unsigned char* images, const int* qtab, const int* huff,
                              const unsigned char* header, short* coef, unsigned char* scratch,
                              int* seglen, unsigned char* out, int* length, int M, int H, int W,
                              int sub420, long long cap, hipStream_t s) {
  if (H < 1 || H > kJpMaxExtent || W < 1 || W > kJpMaxExtent) return -1;
  if (M < 0 || M > 65535) return -2;
  if (cap < 1 || cap > 0x7fffffffll) return -3;
  if ((reinterpret_cast<uintptr_t>(coef) & 15) || (reinterpret_cast<uintptr_t>(qtab) & 3) ||
      (reinterpret_cast<uintptr_t>(huff) & 3) || (reinterpret_cast<uintptr_t>(seglen) & 3) ||
      (reinterpret_cast<uintptr_t>(length) & 3))
    return -7;
  if (M == 0) return 0;
  const int mcu = sub420 ? 16 : 8, bpm = sub420 ? 6 : 3;
  const int mh = (H + mcu - 1) / mcu, mw = (W + mcu - 1) / mcu;
  const int nb = mw * bpm;
  const long long seg_cap_ll = (long long)nb * kJpBlockBytes + 16;
  const int seg_cap = (int)seg_cap_ll;  // <= 3072 * 416 + 16
  // the worst-case file must fit the int32 length
  if (kJpHeader + (long long)mh * (seg_cap_ll + 2) + 2 > 0x7fffffffll) return -4;
#ifdef KVEDGE_CHECKS
  if (!rs_in_alloc(images, (long long)M * H * W * 3)) return -20;
  if (!rs_in_alloc(coef, (long long)M * mh * nb * 128)) return -21;
  if (!rs_in_alloc(scratch, (long long)M * mh * seg_cap)) return -22;
  if (!rs_in_alloc(seglen, (long long)M * mh * 4)) return -23;
  if (!rs_in_alloc(out, (long long)M * cap)) return -24;
  if (!rs_in_alloc(length, (long long)M * 4)) return -25;
  if (!rs_in_alloc(header, kJpHeader) || !rs_in_alloc(qtab, 128 * 4) ||
      !rs_in_alloc(huff, 1024 * 4))
    return -26;
#endif
  const int vec_ok = (reinterpret_cast<uintptr_t>(images) % 4 == 0) && (W % 4 == 0);
  const int mcus = kJpStripPx / mcu;
  const dim3 g1((unsigned)((mw + mcus - 1) / mcus), (unsigned)mh, (unsigned)M);
  const dim3 g2((unsigned)mh, (unsigned)M);
  if (sub420) {
    hipLaunchKernelGGL(jpeg_blocks_kernel<true>, g1, dim3(kJpThreads), 0, s, images, qtab, coef,
                       H, W, mw, mh, vec_ok);
    hipLaunchKernelGGL(jpeg_entropy_kernel<true>, g2, dim3(kWave), 0, s, coef, huff, scratch,
                       seglen, nb, mh, seg_cap);
  } else {
    hipLaunchKernelGGL(jpeg_blocks_kernel<false>, g1, dim3(kJpThreads), 0, s, images, qtab, coef,
                       H, W, mw, mh, vec_ok);
    hipLaunchKernelGGL(jpeg_entropy_kernel<false>, g2, dim3(kWave), 0, s, coef, huff, scratch,
                       seglen, nb, mh, seg_cap);
  }
  if (hipGetLastError() != hipSuccess) return -100;
  hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)M), dim3(kJpPackThreads), 0, s, scratch,
                     seglen, header, out, length, mh, seg_cap, cap);
  return hipGetLastError() == hipSuccess ? 0 : -100;
}
