// Host self-test of the JPEG decoder core (csrc/kernels/jpeg_decode_core.h): the header parser,
// the bit reader, the Huffman walk, the IDCT and the colour formulas that the device kernels
// run, over a corpus of files -- the malformed ones above all -- on the CPU.  Built with
// -fsanitize=address,undefined (python -m kvedge_amd._build --asan) and run by
// tools/jpeg_decode_hostcheck.py, which writes the corpus and compares the result with
// ops.reference.jpeg_decode.  Every buffer is allocated at its exact size, so a read or write
// past a row, a table or a plane is reported.
//
//   kv_jpeg_decode_selftest CORPUS OUT
//   CORPUS: int32 N, row_bytes, H, W, then N rows of row_bytes.  OUT: per file int32 status and
//   H * W * 3 RGB bytes.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "jpeg_decode_core.h"

using namespace kvedge;

namespace {

// what the scan / decode / colour launches do for one file, one interval after the other
int decode_file(const uint8_t* row, int n, int H, int W, uint8_t* rgb) {
  JdTables* T = static_cast<JdTables*>(aligned_alloc(16, sizeof(JdTables)));
  memset(T, 0, sizeof(JdTables));
  int err = jd_parse_header(row, n, H, W, T);
  if (err) {
    memset(rgb, 0, (size_t)H * W * 3);
    free(T);
    return -err;
  }
  const JdInfo& I = T->info;
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

  const long long pitch = (W + 15) / 16 * 16, plane = pitch * ((H + 15) / 16 * 16);
  uint8_t* pl = static_cast<uint8_t*>(aligned_alloc(16, (size_t)(3 * plane)));
  const int hs = I.hs, vs = I.vs, ny = hs * vs, bpm = ny + 2;
  const int mcus = I.mw * I.mh, iters = I.ri ? I.ri : mcus;
  std::vector<int16_t> coef((size_t)bpm * 64);
  for (int k = 0; k < I.expected; ++k) {
    bool failed = k >= present;
    int start = 0, stop = 0;
    if (!failed) {
      start = k == 0 ? I.e0 : mpos[k - 1] + 2;
      stop = k < nmark ? mpos[k] : n;
      if (start > n) start = n;
      if (stop < start) stop = start;
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
  if (argc != 3) {
    fprintf(stderr, "usage: %s CORPUS OUT\n", argv[0]);
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
  std::vector<uint8_t> rgb((size_t)H * W * 3);
  for (int i = 0; i < N; ++i) {
    if (fread(row, 1, (size_t)n, f) != (size_t)n) return 6;
    const int32_t st = decode_file(row, n, H, W, rgb.data());
    fwrite(&st, 4, 1, o);
    fwrite(rgb.data(), 1, rgb.size(), o);
  }
  free(row);
  fclose(o);
  fclose(f);
  printf("jpeg_decode selftest: %d files decoded\n", N);
  return 0;
}
