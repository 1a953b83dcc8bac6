// Host self-test of the JPEG decoder core (csrc/kernels/jpeg_decode_core.h): the header parser,
// the bit reader, the Huffman walk, the IDCT and the colour formulas that the device kernels
// run, over a corpus of files -- the malformed ones above all -- on the CPU.  Built with
// -fsanitize=address,undefined (python -m kvedge_amd._build --asan) and run by
// tools/jpeg_decode_hostcheck.py, which writes the corpus and compares the result with
// ops.reference.jpeg_decode.  Every buffer is allocated at its exact size, so a read or write
// past a row, a table or a plane is reported.
//
//   kv_jpeg_decode_selftest [--parallel G] CORPUS OUT
//   CORPUS: int32 N, row_bytes, H, W, then N rows of row_bytes.  OUT: per file int32 status and
//   H * W * 3 RGB bytes.
//   --parallel G: every restart interval longer than one subsequence goes through the split
//   path's lane steps (speculate, synchronise in groups of G lanes, seams, chain check, prefix
//   sums, write) lane by lane, as the device's launches order them, and falls back to the serial
//   walk on any anomaly; the result must equal the serial walk's (exit 7 if not) and is what
//   OUT gets.  A small G puts seams into small files.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "jpeg_decode_core.h"

using namespace kvedge;

namespace {

constexpr int kSeamRounds = 8;

// The split path for interval k = [istart, istop): true if it completed (the planes hold the
// interval), false if it must be handed back.
bool parallel_interval(const uint8_t* row, const JdTables& T, int k, int istart, int istop, int G,
                       uint8_t* pl, long long pitch, long long plane) {
  const int S = kJdSplitBytes, nl = (istop - 1) / S - istart / S + 1;
  std::vector<int> beg(nl), bound(nl);
  std::vector<JdState> from(nl);
  std::vector<JdLaneSums> sums(nl);
  for (int l = 0; l < nl; ++l) {
    beg[l] = l ? (istart / S + l) * S : istart;
    bound[l] = std::min((beg[l] / S + 1) * S, istop);
    from[l] = jd_lane_cold(row, istart, beg[l]);
  }
  for (int g0 = 0; g0 < nl; g0 += G) {  // speculate + synchronise, one workgroup
    const int ge = std::min(g0 + G, nl);
    std::vector<char> need(nl, 1);
    for (int r = 0; r < G; ++r) {
      for (int l = g0; l < ge; ++l)
        if (need[l]) jd_lane_count(row, T, istart, istop, from[l], bound[l], sums[l]);
      bool any = false;
      need[g0] = 0;
      for (int l = g0 + 1; l < ge; ++l) {
        const JdState prev = sums[l - 1].end;
        need[l] = prev.byte >= 0 && !jd_same(prev, from[l]);
        if (need[l]) from[l] = prev;
        any |= need[l] != 0;
      }
      if (!any) break;
    }
  }
  const int nwg = (nl + G - 1) / G;
  for (int r = 0; r < kSeamRounds; ++r) {  // seams, odd then even
    int moved = 0;
    for (int half = 0; half < 2; ++half)
      for (int s = 1 + half; s < nwg; s += 2) {
        JdState e = sums[s * G - 1].end;
        for (int l = s * G; l < std::min(s * G + G, nl) && e.byte >= 0; ++l) {
          if (jd_same(from[l], e)) break;
          jd_lane_count(row, T, istart, istop, e, bound[l], sums[l]);
          from[l] = e;
          e = sums[l].end;
          ++moved;
        }
      }
    if (!moved) break;
  }
  int g = 0;  // chain check and prefix sums
  uint32_t pred[3] = {0, 0, 0};
  std::vector<int> g0s(nl);
  std::vector<uint32_t> preds((size_t)nl * 3);
  for (int l = 0; l < nl; ++l) {
    const JdState want = l ? sums[l - 1].end : JdState{istart, 0};
    if (want.byte < 0 || !jd_same(from[l], want)) return false;
    g0s[l] = g;
    g += sums[l].nblk;
    for (int c = 0; c < 3; ++c) {
      preds[(size_t)l * 3 + c] = pred[c];
      pred[c] += sums[l].dc[c];
    }
  }
  if (g != jd_interval_blocks(T.info, k)) return false;
  bool ok = true;
  int16_t coef[64];
  for (int l = 0; l < nl; ++l) {
    const uint32_t p[3] = {preds[(size_t)l * 3], preds[(size_t)l * 3 + 1], preds[(size_t)l * 3 + 2]};
    ok &= !jd_lane_write(row, T, istart, istop, from[l], bound[l], g0s[l],
                         jd_interval_blocks(T.info, k), (long long)k * T.info.ri, p, coef, 1, pl,
                         pitch, plane);
  }
  return ok;
}

// what the scan / decode / colour launches do for one file, one interval after the other;
// G > 0: long intervals try the split path first.  paths: completed, handed back.
int decode_file(const uint8_t* row, int n, int H, int W, uint8_t* rgb, int G, int (&paths)[2]) {
  JdTables* T = static_cast<JdTables*>(aligned_alloc(16, sizeof(JdTables)));
  memset(T, 0, sizeof(JdTables));
  int err = jd_parse_header(row, n, H, W, T);
  if (err) {
    memset(rgb, 0, (size_t)H * W * 3);
    free(T);
    return -err;
  }
  JdInfo& I = T->info;
  std::vector<int> mpos;
  bool eoi = false;
  for (int i = I.e0; i + 1 < n; ++i) {
    if (row[i] != 0xff) continue;
    if (row[i + 1] >= 0xd0 && row[i + 1] <= 0xd7) mpos.push_back(i);
    if (row[i + 1] == 0xd9) {
      mpos.push_back(i);
      eoi = true;
      break;
    }
  }
  const int nmark = (int)mpos.size(), present = eoi ? nmark : nmark + 1;
  err = (eoi ? 0 : JD_E_NOEOI) | (present != I.expected ? JD_E_INTERVALS : 0);
  I.nmark = nmark;
  I.present = present;
  mpos.resize((size_t)std::max(nmark, I.expected) + 1, 0);

  const long long pitch = (W + 15) / 16 * 16, plane = pitch * ((H + 15) / 16 * 16);
  uint8_t* pl = static_cast<uint8_t*>(aligned_alloc(16, (size_t)(3 * plane)));
  const int hs = I.hs, vs = I.vs, ny = hs * vs, bpm = ny + 2;
  const int mcus = I.mw * I.mh, iters = I.ri ? I.ri : mcus;
  std::vector<int16_t> coef((size_t)bpm * 64);
  for (int k = 0; k < I.expected; ++k) {
    bool failed = k >= present;
    int start = 0, stop = 0;
    if (!failed) {
      jd_interval(I, mpos.data(), k, n, (int)mpos.size(), start, stop);
      if (G > 0 && stop - start > kJdSplitBytes) {
        const bool ok = parallel_interval(row, *T, k, start, stop, G, pl, pitch, plane);
        ++paths[ok ? 0 : 1];
        if (ok) continue;
      }
    }
    JdReader rd(row, start, stop);
    int pred[3] = {0, 0, 0};
    for (int it = 0; it < iters; ++it) {
      const long long m = I.ri ? (long long)k * I.ri + it : it;
      if (m >= mcus) break;
      std::fill(coef.begin(), coef.end(), (int16_t)0);
      if (!failed) {
        for (int b = 0; b < bpm; ++b) {
          const int c = b < ny ? 0 : b - ny + 1;
          int16_t* blk = coef.data() + b * 64;
          if (jd_decode_block(rd, T->h[I.td[c]], T->h[2 + I.ta[c]], pred[c], blk, 1)) {
            failed = true;
            err |= JD_E_ENTROPY;
            memset(blk, 0, 128);
            break;
          }
        }
      }
      const int mx = (int)(m % I.mw), my = (int)(m / I.mw);
      for (int b = 0; b < bpm; ++b) {
        const int c = b < ny ? 0 : b - ny + 1;
        const int by = c == 0 ? my * vs + b / hs : my, bx = c == 0 ? mx * hs + b % hs : mx;
        jd_idct_block(coef.data() + b * 64, 1, T->q[I.tq[c]],
                      pl + c * plane + (long long)by * 8 * pitch + bx * 8, pitch);
      }
    }
  }
  const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      int r, g, b;
      jd_rgb(pl[y * pitch + x], jd_chroma(pl + plane, pitch, cw, ch, hs, vs, x, y),
             jd_chroma(pl + 2 * plane, pitch, cw, ch, hs, vs, x, y), r, g, b);
      uint8_t* d = rgb + ((size_t)y * W + x) * 3;
      d[0] = (uint8_t)r;
      d[1] = (uint8_t)g;
      d[2] = (uint8_t)b;
    }
  free(pl);
  free(T);
  return -err;
}

}  // namespace

int main(int argc, char** argv) {
  int G = 0;
  if (argc == 5 && !strcmp(argv[1], "--parallel")) {
    G = atoi(argv[2]);
    argv += 2;
    argc -= 2;
    if (G < 1 || G > 1024) return 2;
  }
  if (argc != 3) {
    fprintf(stderr, "usage: %s [--parallel G] CORPUS OUT\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  int32_t hd[4];
  if (!f || fread(hd, 4, 4, f) != 4) return 3;
  const int N = hd[0], n = hd[1], H = hd[2], W = hd[3];
  if (N < 0 || n < 16 || (n & 15) || H < 1 || H > 8192 || W < 1 || W > 8192) return 4;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 5;
  uint8_t* row = static_cast<uint8_t*>(aligned_alloc(16, (size_t)n));  // exactly one row
  std::vector<uint8_t> rgb((size_t)H * W * 3), serial(rgb.size());
  int paths[2] = {0, 0}, none[2] = {0, 0}, differ = 0;
  for (int i = 0; i < N; ++i) {
    if (fread(row, 1, (size_t)n, f) != (size_t)n) return 6;
    const int32_t st = decode_file(row, n, H, W, rgb.data(), G, paths);
    if (G && (decode_file(row, n, H, W, serial.data(), 0, none) != st || serial != rgb)) {
      fprintf(stderr, "file %d: the split path and the serial walk differ\n", i);
      ++differ;
    }
    fwrite(&st, 4, 1, o);
    fwrite(rgb.data(), 1, rgb.size(), o);
  }
  free(row);
  fclose(o);
  fclose(f);
  printf("jpeg_decode selftest: %d files decoded", N);
  if (G) printf(", split path completed %d intervals, handed back %d", paths[0], paths[1]);
  printf("\n");
  return differ ? 7 : 0;
}
