// Baseline JPEG decoder core shared by the device kernels (jpeg_decode.hip) and the host
// self-test (csrc/runtime/jpeg_decode_selftest_main.cpp, built with host sanitizers): the
// header parser, the Huffman table builder, the bit reader, the per-block Huffman walk, the
// IDCT and the upsample / colour formulas.  ops.reference.jpeg_decode is THE definition; this
// file computes exactly its integers.
//
// Files are untrusted.  Every loop below is bounded by a count fixed before it starts, every
// offset taken from the file is checked against the row before it is used, and every table
// index is masked or bounded by construction.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JD_HD __host__ __device__ __forceinline__
#else
#define JD_HD inline
#endif

namespace kvedge {

// error bits; status = -(mask).  The first six are header errors: the image is zero-filled.
enum : int {
  JD_E_MARKER = 1,      // no SOI, a stray marker, a segment of the wrong length
  JD_E_TRUNC = 2,       // a header segment runs past the row
  JD_E_UNSUP = 4,       // progressive, 12 bit, not 3 components, sampling, 16-bit tables ...
  JD_E_SIZE = 8,        // SOF size != (H, W)
  JD_E_MISSING = 16,    // SOS before SOF, or a table the scan names was never defined
  JD_E_DHT = 32,        // a Huffman table that is no prefix code
  JD_E_ENTROPY = 64,    // invalid code, coefficient index past 63, interval ran out of bits
  JD_E_INTERVALS = 128, // restart intervals found != expected
  JD_E_NOEOI = 256,     // no EOI inside the row
  JD_HDR_ERRORS = 63,
};
constexpr int kJdMaxSegments = 256;
constexpr int kJdLook = 9;

struct JdHuff {
  uint16_t look[1 << kJdLook];  // symbol | length << 8 for codes of <= 9 bits, else 0
  int32_t maxcode[17];          // [l]: largest code of length l, -1 if none
  int32_t valoff[17];           // [l]: index of the first symbol of length l - its code
  uint8_t val[256];
};
struct JdInfo {
  int32_t err, e0, ri, hs, vs, mw, mh, expected, present, nmark;
  int32_t tq[3], td[3], ta[3];
  int32_t pad_[1];
};
struct JdTables {
  JdInfo info;
  uint16_t q[4][64];  // natural order
  JdHuff h[4];        // [class * 2 + id]
};
static_assert(sizeof(JdTables) % 16 == 0, "copied to LDS as 16-byte words");

// zigzag position -> natural index
#if defined(__HIP_DEVICE_COMPILE__)
__device__
#endif
    static const uint8_t kJdZigzag[64] = {
        0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

JD_HD int jd_be16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// bits[16] codes per length, total = their sum <= 256 symbols at vals
JD_HD int jd_build_huff(const uint8_t* bits, const uint8_t* vals, int total, JdHuff* h) {
  for (int i = 0; i < (1 << kJdLook); ++i) h->look[i] = 0;
  for (int i = 0; i < 256; ++i) h->val[i] = i < total ? vals[i] : 0;
  h->maxcode[0] = -1;
  h->valoff[0] = 0;
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    const int n = bits[l - 1];
    if (code + n > (1 << l)) return JD_E_DHT;
    h->valoff[l] = k - code;
    h->maxcode[l] = n ? code + n - 1 : -1;
    if (l <= kJdLook) {
      const int rep = 1 << (kJdLook - l);  // (code + n) * rep <= 512
      for (int c = 0; c < n; ++c)
        for (int s = 0; s < rep; ++s)
          h->look[((code + c) * rep + s) & 511] = (uint16_t)(vals[k + c] | (l << 8));
    }
    k += n;
    code = (code + n) << 1;
  }
  return 0;
}

// Walks SOI .. SOS of the n-byte row p, fills t->q, t->h and t->info; returns 0 or one error
// bit.  (H, W) is the size the caller expects.
JD_HD int jd_parse_header(const uint8_t* p, int n, int H, int W, JdTables* t) {
  JdInfo& I = t->info;
  I.err = I.e0 = I.ri = I.mw = I.mh = I.expected = I.present = I.nmark = 0;
  I.hs = I.vs = 1;
  for (int c = 0; c < 3; ++c) I.tq[c] = I.td[c] = I.ta[c] = 0;
  I.pad_[0] = 0;
  if (n < 4 || p[0] != 0xff || p[1] != 0xd8) return JD_E_MARKER;
  int pos = 2, have_q = 0, have_h = 0, cid[3] = {0, 0, 0};
  bool sof = false;
  for (int seg = 0; seg < kJdMaxSegments; ++seg) {
    if (pos + 4 > n) return JD_E_TRUNC;
    if (p[pos] != 0xff) return JD_E_MARKER;
    const int m = p[pos + 1];
    if (m == 0 || m == 1 || m == 0xff || (m >= 0xd0 && m <= 0xd9)) return JD_E_MARKER;
    const int len = jd_be16(p + pos + 2);
    if (len < 2 || pos + 2 + len > n) return JD_E_TRUNC;
    const uint8_t* s = p + pos + 4;
    const int sl = len - 2;
    if (m == 0xdb) {
      int q = 0;
      for (int it = 0; it < 4 && q < sl; ++it) {
        const int pq = s[q];
        if ((pq >> 4) != 0 || (pq & 15) > 3) return JD_E_UNSUP;
        if (q + 65 > sl) return JD_E_TRUNC;
        for (int i = 0; i < 64; ++i) t->q[pq & 3][kJdZigzag[i]] = s[q + 1 + i];
        have_q |= 1 << (pq & 3);
        q += 65;
      }
      if (q != sl) return JD_E_MARKER;
    } else if (m == 0xc4) {
      int q = 0;
      for (int it = 0; it < 4 && q < sl; ++it) {
        if (q + 17 > sl) return JD_E_TRUNC;
        const int tc = s[q] >> 4, th = s[q] & 15;
        if (tc > 1 || th > 1) return JD_E_UNSUP;
        int total = 0;
        for (int i = 0; i < 16; ++i) total += s[q + 1 + i];
        if (total > 256) return JD_E_DHT;
        if (q + 17 + total > sl) return JD_E_TRUNC;
        const int rc = jd_build_huff(s + q + 1, s + q + 17, total, &t->h[tc * 2 + th]);
        if (rc) return rc;
        have_h |= 1 << (tc * 2 + th);
        q += 17 + total;
      }
      if (q != sl) return JD_E_MARKER;
    } else if (m == 0xc0) {
      if (sof) return JD_E_MARKER;
      if (sl < 6) return JD_E_TRUNC;
      if (s[0] != 8 || s[5] != 3) return JD_E_UNSUP;
      if (sl != 15) return JD_E_MARKER;
      if (jd_be16(s + 1) != H || jd_be16(s + 3) != W) return JD_E_SIZE;
      for (int c = 0; c < 3; ++c) {
        cid[c] = s[6 + 3 * c];
        const int hv = s[7 + 3 * c];
        I.tq[c] = s[8 + 3 * c];
        if (I.tq[c] > 3) return JD_E_UNSUP;
        if (c == 0 ? (hv != 0x11 && hv != 0x21 && hv != 0x22) : hv != 0x11) return JD_E_UNSUP;
        if (c == 0) {
          I.hs = hv >> 4;
          I.vs = hv & 15;
        }
      }
      sof = true;
    } else if (m >= 0xc1 && m <= 0xcf) {
      return JD_E_UNSUP;  // every other frame type, and arithmetic conditioning
    } else if (m == 0xdd) {
      if (sl != 2) return JD_E_MARKER;
      I.ri = jd_be16(s);
    } else if (m == 0xda) {
      if (!sof) return JD_E_MISSING;
      if (sl != 10 || s[0] != 3) return JD_E_UNSUP;
      for (int c = 0; c < 3; ++c) {
        if (s[1 + 2 * c] != cid[c]) return JD_E_UNSUP;
        I.td[c] = s[2 + 2 * c] >> 4;
        I.ta[c] = s[2 + 2 * c] & 15;
        if (I.td[c] > 1 || I.ta[c] > 1) return JD_E_UNSUP;
      }
      if (s[7] != 0 || s[8] != 63 || s[9] != 0) return JD_E_UNSUP;
      for (int c = 0; c < 3; ++c)
        if (!((have_q >> I.tq[c]) & 1) || !((have_h >> I.td[c]) & 1) ||
            !((have_h >> (2 + I.ta[c])) & 1))
          return JD_E_MISSING;
      I.e0 = pos + 2 + len;
      I.mw = (W + 8 * I.hs - 1) / (8 * I.hs);
      I.mh = (H + 8 * I.vs - 1) / (8 * I.vs);
      const int mcus = I.mw * I.mh;
      I.expected = I.ri ? (mcus + I.ri - 1) / I.ri : 1;
      return 0;
    } else if (!((m >= 0xe0 && m <= 0xef) || m == 0xfe)) {
      return JD_E_UNSUP;
    }
    pos += 2 + len;
  }
  return JD_E_UNSUP;
}

// 16 bytes of the row at a 16-byte boundary (rows are whole 16-byte words, 16-byte aligned)
JD_HD void jd_load16(const uint8_t* p, uint32_t (&w)[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
#else
  memcpy(w, p, 16);
#endif
}

// MSB-first bit reader over the bytes [bp, end) of one restart interval: FF 00 reads as FF,
// bytes past the end read as 0 and are counted in pad.
struct JdReader {
  const uint8_t* row;
  int bp, end, nbits, pad, chunk;
  uint64_t acc;  // the next nbits bits, left-aligned
  uint32_t w[4];
  JD_HD JdReader(const uint8_t* r, int start, int stop)
      : row(r), bp(start), end(stop), nbits(0), pad(0), chunk(-1), acc(0) {
    w[0] = w[1] = w[2] = w[3] = 0;
  }
  JD_HD uint32_t byte_at(int i) {  // i < end
    if ((i >> 4) != chunk) {
      chunk = i >> 4;
      jd_load16(row + ((long long)chunk << 4), w);
    }
    const uint32_t x = (i & 8) ? ((i & 4) ? w[3] : w[2]) : ((i & 4) ? w[1] : w[0]);
    return (x >> (8 * (i & 3))) & 255u;
  }
  JD_HD void refill() {  // afterwards nbits >= 57
    for (int i = 0; i < 8; ++i) {
      if (nbits > 56) break;
      uint32_t b = 0;
      if (bp >= end) {
        ++pad;
      } else {
        b = byte_at(bp++);
        if (b == 0xffu && bp < end && byte_at(bp) == 0u) ++bp;
      }
      acc |= (uint64_t)b << (56 - nbits);
      nbits += 8;
    }
  }
  JD_HD uint32_t peek(int l) const { return (uint32_t)(acc >> (64 - l)); }  // 1 <= l <= 32
  JD_HD void skip(int l) {
    acc <<= l;
    nbits -= l;
  }
  JD_HD bool overrun() const { return nbits < 8 * pad; }
};

// one symbol (at most 16 bits; the caller may take 15 more before the next refill), or -1
JD_HD int jd_symbol(JdReader& r, const JdHuff& h) {
  r.refill();
  const uint32_t e = h.look[r.peek(kJdLook)];
  if (e) {
    r.skip((int)(e >> 8));
    return (int)(e & 255u);
  }
  for (int l = kJdLook + 1; l <= 16; ++l) {
    const int code = (int)r.peek(l);
    if (code <= h.maxcode[l]) {
      r.skip(l);
      return h.val[(code + h.valoff[l]) & 255];
    }
  }
  return -1;
}

JD_HD int jd_receive_extend(JdReader& r, int s) {  // 1 <= s <= 15
  const int v = (int)r.peek(s);
  r.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// One block into out[natural * stride] (all 64 zero on entry); pred is the component's DC
// predictor.  Returns 0, or 1 on an invalid code, a DC category above 15, a coefficient index
// past 63 or an interval that ran out of bits -- the caller zeroes the block again.
JD_HD int jd_decode_block(JdReader& r, const JdHuff& dc, const JdHuff& ac, int& pred,
                          int16_t* out, int stride) {
  int s = jd_symbol(r, dc);
  if (s < 0 || s > 15) return 1;
  if (s) pred += jd_receive_extend(r, s);
  out[0] = (int16_t)pred;
  int k = 1;
  for (int it = 0; it < 63 && k < 64; ++it) {
    const int sym = jd_symbol(r, ac);
    if (sym < 0) return 1;
    const int run = sym >> 4;
    s = sym & 15;
    if (s == 0) {
      if (run != 15) break;
      k += 16;
      continue;
    }
    k += run;
    if (k > 63) return 1;
    out[kJdZigzag[k] * stride] = (int16_t)jd_receive_extend(r, s);
    ++k;
  }
  return r.overrun() ? 1 : 0;
}

// Bounds of restart interval k in the n-byte row: mp holds the marker offsets the scan found
// (read back from scratch, so clamped to the row), max_int entries at most.
JD_HD void jd_interval(const JdInfo& I, const int* mp, int k, int n, int max_int, int& start,
                       int& stop) {
  const int cap = I.expected < max_int ? I.expected : max_int;
  const int a = k == 0 ? I.e0 : mp[k - 1 < cap - 1 ? k - 1 : cap - 1] + 2;
  start = a < 0 ? 0 : a > n ? n : a;
  stop = n;
  if (k < I.nmark) {
    const int b = mp[k < cap - 1 ? k : cap - 1];
    stop = b < 0 ? 0 : b > n ? n : b;
  }
  if (stop < start) stop = start;
}

// libjpeg's slow integer IDCT (jidctint.c): 13-bit constants, one 8-point pass.  Arithmetic
// wraps modulo 2^32 (as int32 arrays do in the reference), shifts are arithmetic.
JD_HD uint32_t jd_sra(uint32_t x, int n) { return (uint32_t)((int32_t)x >> n); }
JD_HD void jd_idct8(const uint32_t (&d)[8], uint32_t (&o)[8], int shift) {
  uint32_t z2 = d[2], z3 = d[6];
  uint32_t z1 = (z2 + z3) * 4433u;
  uint32_t t2 = z1 - z3 * 15137u, t3 = z1 + z2 * 6270u;
  uint32_t t0 = (d[0] + d[4]) << 13, t1 = (d[0] - d[4]) << 13;
  const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = d[7]; t1 = d[5]; t2 = d[3]; t3 = d[1];
  z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2;
  uint32_t z4 = t1 + t3;
  const uint32_t z5 = (z3 + z4) * 9633u;
  t0 *= 2446u; t1 *= 16819u; t2 *= 25172u; t3 *= 12299u;
  z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
  z3 = z3 * (uint32_t)-16069 + z5;
  z4 = z4 * (uint32_t)-3196 + z5;
  t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
  const uint32_t r = 1u << (shift - 1);
  o[0] = jd_sra(t10 + t3 + r, shift); o[7] = jd_sra(t10 - t3 + r, shift);
  o[1] = jd_sra(t11 + t2 + r, shift); o[6] = jd_sra(t11 - t2 + r, shift);
  o[2] = jd_sra(t12 + t1 + r, shift); o[5] = jd_sra(t12 - t1 + r, shift);
  o[3] = jd_sra(t13 + t0 + r, shift); o[4] = jd_sra(t13 - t0 + r, shift);
}
// libjpeg's range_limit[(x & 1023)] with the +128 level shift in it
JD_HD uint32_t jd_range(uint32_t x) {
  const uint32_t v = x & 1023u;
  return v < 128u ? v + 128u : v < 512u ? 255u : v < 896u ? 0u : v - 896u;
}
// A whole block: coef[natural * stride] * q[natural], columns then rows; dst gets 8 rows of 8
// samples at the given pitch, each row as two little-endian dwords (dst is 8-byte aligned).
JD_HD void jd_idct_block(const int16_t* coef, int stride, const uint16_t* q, uint8_t* dst,
                         long long pitch) {
  uint32_t ws[64];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    uint32_t d[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r)
      d[r] = (uint32_t)((int32_t)coef[(r * 8 + c) * stride] * (int32_t)q[r * 8 + c]);
    jd_idct8(d, o, 11);
#pragma unroll
    for (int r = 0; r < 8; ++r) ws[r * 8 + c] = o[r];
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    uint32_t d[8], o[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) d[c] = ws[r * 8 + c];
    jd_idct8(d, o, 18);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      lo |= jd_range(o[c]) << (8 * c);
      hi |= jd_range(o[4 + c]) << (8 * c);
    }
    uint32_t* w = reinterpret_cast<uint32_t*>(dst + r * pitch);
    w[0] = lo;
    w[1] = hi;
  }
}

// libjpeg's "fancy" triangle upsampling of one chroma plane at pixel (x, y): hs, vs in {1, 2},
// the plane holds cw x ch real samples (indices are clamped, which is libjpeg's edge rule).
JD_HD int jd_clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
JD_HD int jd_chroma(const uint8_t* pl, long long pitch, int cw, int ch, int hs, int vs, int x,
                    int y) {
  if (hs == 1) return pl[y * pitch + x];
  const int i = x >> 1, j = (x & 1) ? jd_clampi(i + 1, 0, cw - 1) : jd_clampi(i - 1, 0, cw - 1);
  if (vs == 1) {
    const uint8_t* r = pl + y * pitch;
    return (3 * r[i] + r[j] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int rn = y >> 1, rf = (y & 1) ? jd_clampi(rn + 1, 0, ch - 1) : jd_clampi(rn - 1, 0, ch - 1);
  const uint8_t* a = pl + rn * pitch;
  const uint8_t* b = pl + rf * pitch;
  const int cs = 3 * a[i] + b[i], co = 3 * a[j] + b[j];
  return (3 * cs + co + ((x & 1) ? 7 : 8)) >> 4;
}
// libjpeg's 16-bit fixed-point JFIF YCbCr -> RGB (jdcolor.c)
JD_HD void jd_rgb(int y, int cb, int cr, int& r, int& g, int& b) {
  cb -= 128;
  cr -= 128;
  r = jd_clampi(y + ((91881 * cr + 32768) >> 16), 0, 255);
  g = jd_clampi(y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255);
  b = jd_clampi(y + ((116130 * cb + 32768) >> 16), 0, 255);
}

// ---------------------------------------------------------------------------------------------
// A long restart interval decoded by many lanes.  The interval is cut at the row's multiples of
// kJdSplitBytes into subsequences, one lane each.  Huffman streams self-synchronise, so a lane
// that starts cold at its first bit soon walks the serial decoder's symbols; the lanes then
// exchange end states until lane i starts exactly where lane i - 1 stopped, which makes their
// concatenation the serial decode.  These are the per-lane steps; who runs which lane when is
// the caller's business (the kernels in jpeg_decode.hip, the host self-test lane by lane).
//
// A decoder state sits at a symbol boundary: the row byte and bit of the next symbol, the block
// of the MCU it belongs to and the zigzag index it continues at (0: the next symbol is a DC
// code).  A symbol is a Huffman code with its extra bits.  The byte of a state is never the 00
// of an FF 00 pair, so equal positions have equal states.
// S, a multiple of the row's 16-byte words.  64 rather than the first guess of 128: the longest
// block a baseline encoder writes for 8-bit noise is near 117 bytes, and at 64 such blocks
// cover whole subsequences, so lanes that start and end inside one block occur in ordinary
// files (and in the tests) rather than never.
constexpr int kJdSplitBytes = 64;
// "auto" splits intervals longer than this: where the probe's sweep of the interval length has
// the split path level with the one-lane walk (b64 1080p 4:2:0 q75: 40 MCUs, about 1000 bytes)
constexpr int kJdAutoSplitBytes = 16 * kJdSplitBytes;
constexpr int kJdSplitSymbols = 8 * kJdSplitBytes;    // a symbol has at least one bit
constexpr int kJdSplitBlocks = 4 * kJdSplitBytes + 1;  // a block has at least two
constexpr int jd_lanes_per_row(long long row_bytes) {  // every interval longer than S fits
  return (int)(3 * (row_bytes / kJdSplitBytes) + 3);
}

struct JdState {
  int32_t byte;  // < 0: no state
  int32_t sub;   // bit | block << 3 | zigzag << 8
};
JD_HD bool jd_same(const JdState& a, const JdState& b) {
  return a.byte == b.byte && a.sub == b.sub;
}
struct JdLaneSums {
  JdState end;      // the first symbol that starts at or after the lane's boundary
  int32_t nblk;     // DC symbols read = blocks this lane owns
  uint32_t dc[3];   // their differences summed per component, wrapping
};

// blocks the serial walk decodes in interval k
JD_HD int jd_interval_blocks(const JdInfo& I, int k) {
  const int bpm = (I.hs & 3) * (I.vs & 3) + 2, mcus = I.mw * I.mh;
  if (!I.ri) return mcus * bpm;
  const long long left = (long long)mcus - (long long)k * I.ri;
  return (int)(left < 0 ? 0 : left < I.ri ? left : I.ri) * bpm;
}

// where a lane whose subsequence begins at byte beg > istart starts before it knows better
JD_HD JdState jd_lane_cold(const uint8_t* row, int istart, int beg) {
  JdState s = {beg, 0};
  if (beg > istart && row[beg - 1] == 0xff && row[beg] == 0) s.byte = beg + 1;
  return s;
}

// the reader is certainly before row byte bound (cheap: stuffed bytes only move it back)
JD_HD bool jd_reader_before(const JdReader& r, int bound) {
  return r.bp - ((r.nbits + 7) >> 3) + r.pad < bound;
}
// the state at the reader's next bit; lo is the byte the reader started at; not overrun
JD_HD JdState jd_reader_state(JdReader& r, int lo, int b, int k) {
  const int nb = ((r.nbits + 7) >> 3) - r.pad;  // row bytes not wholly consumed, 0..8
  int q = r.bp;
  for (int i = 0; i < 8; ++i) {
    if (i >= nb) break;
    --q;
    if (q > lo && r.byte_at(q) == 0u && r.byte_at(q - 1) == 0xffu) --q;
  }
  JdState s = {q < lo ? lo : q, ((8 - (r.nbits & 7)) & 7) | b << 3 | k << 8};
  return s;
}
JD_HD JdReader jd_lane_reader(const uint8_t* row, int istart, int istop, const JdState& from,
                              int& lo) {
  lo = jd_clampi(from.byte, istart, istop);
  JdReader r(row, lo, istop);
  r.refill();
  r.skip(from.sub & 7);
  return r;
}

// One symbol at zigzag index k (0: DC).  Returns JD_SYM_ERR, or what it was, | JD_SYM_END when
// it ended the block (k is 0 again): val is the DC difference or the coefficient at zigzag idx.
enum : int { JD_SYM_ERR = -1, JD_SYM_DC = 0, JD_SYM_AC = 1, JD_SYM_RUN = 2, JD_SYM_END = 4 };
JD_HD int jd_lane_symbol(JdReader& r, const JdHuff& dc, const JdHuff& ac, int& k, int& idx,
                         int& val) {
  if (k == 0) {
    const int s = jd_symbol(r, dc);
    if (s < 0 || s > 15) return JD_SYM_ERR;
    val = s ? jd_receive_extend(r, s) : 0;
    k = 1;
    return JD_SYM_DC;
  }
  const int sym = jd_symbol(r, ac);
  if (sym < 0) return JD_SYM_ERR;
  const int run = sym >> 4, s = sym & 15;
  if (s == 0) {
    k = run == 15 ? k + 16 : 64;
    if (k < 64) return JD_SYM_RUN;
    k = 0;
    return JD_SYM_RUN | JD_SYM_END;
  }
  k += run;
  if (k > 63) return JD_SYM_ERR;
  idx = k;
  val = jd_receive_extend(r, s);
  if (++k < 64) return JD_SYM_AC;
  k = 0;
  return JD_SYM_AC | JD_SYM_END;
}

// Speculate / decode again: walks the symbols from `from` up to the first one that starts at or
// after row byte bound (<= istop) and sums what the lane would own.  Writes no pixels.  An
// invalid code or running out of bits leaves o.end without a state; that is no error here.
JD_HD void jd_lane_count(const uint8_t* row, const JdTables& t, int istart, int istop,
                         const JdState& from, int bound, JdLaneSums& o) {
  const JdInfo& I = t.info;
  const int ny = (I.hs & 3) * (I.vs & 3), bpm = ny + 2;
  o.end.byte = -1;
  o.end.sub = 0;
  o.nblk = 0;
  o.dc[0] = o.dc[1] = o.dc[2] = 0u;
  int lo, b = (from.sub >> 3) & 7, k = (from.sub >> 8) & 63;
  if (b >= bpm) b = 0;
  JdReader r = jd_lane_reader(row, istart, istop, from, lo);
  if (r.overrun()) return;
  for (int it = 0; it <= kJdSplitSymbols; ++it) {
    if (!jd_reader_before(r, bound)) {
      const JdState s = jd_reader_state(r, lo, b, k);
      if (s.byte >= bound) {
        o.end = s;
        return;
      }
    }
    const int c = b < ny ? 0 : b - ny + 1;
    int idx = 0, val = 0;
    const int kind = jd_lane_symbol(r, t.h[I.td[c] & 1], t.h[2 + (I.ta[c] & 1)], k, idx, val);
    if (kind < 0 || r.overrun()) return;
    if ((kind & 3) == JD_SYM_DC) {
      ++o.nblk;
      o.dc[c] += (uint32_t)val;
    }
    if (kind & JD_SYM_END) b = b + 1 == bpm ? 0 : b + 1;
  }
}

// Write: the lane's verified state `from`, g = the interval-wide index of the first block it
// owns, pred = the DC predictors there.  Decodes every block whose DC symbol starts before
// bound, to its end, into coef[natural * stride] and through the IDCT into the planes; stops at
// the interval's nblocks.  mcu0 is the interval's first MCU.  Returns 0, or 1 on anything the
// serial walk would call an error (and on any bound below being hit): the caller hands the
// interval back to the serial walk.
JD_HD int jd_lane_write(const uint8_t* row, const JdTables& t, int istart, int istop,
                        const JdState& from, int bound, int g, int nblocks, long long mcu0,
                        const uint32_t (&pred0)[3], int16_t* coef, int stride, uint8_t* pl,
                        long long pitch, long long plane_bytes) {
  const JdInfo& I = t.info;
  const int hs = I.hs & 3, vs = I.vs & 3, ny = hs * vs, bpm = ny + 2, mw = I.mw > 0 ? I.mw : 1;
  int pred[3] = {(int)pred0[0], (int)pred0[1], (int)pred0[2]};
  int lo, b = (from.sub >> 3) & 7, k = (from.sub >> 8) & 63;
  if (b >= bpm || g < 0) return 1;
  JdReader r = jd_lane_reader(row, istart, istop, from, lo);
  int idx = 0, val = 0;
  if (k != 0) {  // the tail of a block another lane owns
    const int c = b < ny ? 0 : b - ny + 1;
    for (int it = 0; it < 64 && k != 0; ++it)
      if (jd_lane_symbol(r, t.h[I.td[c] & 1], t.h[2 + (I.ta[c] & 1)], k, idx, val) < 0) return 1;
    if (k != 0) return 1;
    b = b + 1 == bpm ? 0 : b + 1;
  }
  for (int blk = 0; blk < kJdSplitBlocks; ++blk) {
    if (g >= nblocks) return 0;
    if (r.overrun()) return 1;
    if (!jd_reader_before(r, bound) && jd_reader_state(r, lo, b, 0).byte >= bound) return 0;
    const int c = b < ny ? 0 : b - ny + 1;
    const JdHuff& dc = t.h[I.td[c] & 1];
    const JdHuff& ac = t.h[2 + (I.ta[c] & 1)];
    for (int i = 0; i < 64; ++i) coef[i * stride] = 0;
    int kind = 0;
    for (int it = 0; it < 64; ++it) {
      kind = jd_lane_symbol(r, dc, ac, k, idx, val);
      if (kind < 0) return 1;
      if ((kind & 3) == JD_SYM_DC) {
        pred[c] = (int)((uint32_t)pred[c] + (uint32_t)val);
        coef[0] = (int16_t)pred[c];
      } else if ((kind & 3) == JD_SYM_AC) {
        coef[kJdZigzag[idx & 63] * stride] = (int16_t)val;
      }
      if (kind & JD_SYM_END) break;
    }
    if (!(kind & JD_SYM_END) || r.overrun()) return 1;
    const long long m = mcu0 + g / bpm;
    const int mx = (int)(m % mw), myr = (int)(m / mw);
    const int by = c == 0 ? myr * vs + b / hs : myr, bx = c == 0 ? mx * hs + b % hs : mx;
    jd_idct_block(coef, stride, t.q[I.tq[c] & 3],
                  pl + c * plane_bytes + (long long)by * 8 * pitch + bx * 8, pitch);
    ++g;
    b = b + 1 == bpm ? 0 : b + 1;
  }
  return 1;
}

}  // namespace kvedge
