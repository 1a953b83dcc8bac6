// Host-visible launcher ABI of libkvedge kernels (gfx950 only).
//
// The kernels take raw device pointers and a hipStream_t so they can be driven
// from the torch binding (csrc/bindings/ops.cpp), from native C++ tools and from
// hipGraph capture alike.  Every launcher is capture-safe: no allocation, no
// synchronisation, no host<->device copies (cdna_hip_programming.md G9).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

// ---------------------------------------------------------------------------
// K1/K2/K3: implicit-GEMM convolution / GEMM on MFMA, NHWC bf16, fp32 accumulate
//   y[m, y_coff + n] = act( sum_k A[m,k] * W[n,k] + bias[n] + res[m, n] )
//   m = (img, ho, wo), k = (r, s, c).  BN is folded into W/bias at load time.
// ---------------------------------------------------------------------------
typedef struct KvConvParams {
  const void* x;      // bf16 input, pixel stride ldx elements, channel offset x_coff
  const void* w;      // bf16 packed weights [Cout][Kpad]
  const float* bias;  // fp32 [Cout] or NULL
  const void* res;    // bf16 residual [M][ldr] or NULL
  void* y;            // bf16 output, row stride ldy, channel offset y_coff
  int N, H, W, Cin;   // input geometry (Cin = logical channels read)
  int ldx, x_coff;
  int Ho, Wo, Cout;
  int KH, KW, stride, pad;
  int K, Kpad;        // logical and padded (multiple of 64) reduction length
  int M;              // N*Ho*Wo
  int ldy, y_coff, ldr, r_coff;
  int act;            // bits[1:0]: 0 none, 1 relu, 2 silu; bit 2: residual after act
  int mode;           // 0 general, 1 1x1/s1/p0 GEMM, 2 stem (Cin=4, KW padded even),
                      // 4 dual 1x1 (bottleneck conv3 + fused downsample, v2 tiles only)
  // mode 4 second source: k in [K1, K) reads x2 [N, H2, W2, ldx2] at stride stride2
  // (the bottleneck's input, i.e. the downsample branch folded in as extra K).
  const void* x2;
  int K1, H2, W2, ldx2, stride2;
  // in_u8 = 1: x is uint8 RGB frames [N, 2H, 2W, 3] and the conv reads their
  // space-to-depth image [N, H, W, 16] (channel (dy*2+dx)*4 + c, channel 3 zero) built on
  // the fly -- the preprocess pass is fused away (v4 direct tile, 2x2 s2d stem only).
  int in_u8;
  // Fused bottleneck tail (v3 streaming tail tile, BN == Cout): after y is written,
  // z = ReLU(y . w_t^T + bias_t) -- the NEXT block's 1x1 reduce conv -- is computed from
  // the y tile still in LDS (w_t: bf16 [n_t][Cout], resident) and written to
  // z[m * ldz + z_coff + n]: y is never re-read from HBM.  n_t = 0: no tail.
  // pair_1x1 = 1 (v4 direct tiles, 3x3 stride 1): the same fields describe a 1x1 conv
  // (w_t [n_t][Cout], bias_t, no activation) applied to the 3x3's activated output, whose
  // result goes to z; y is not written (YOLO Detect branch pairs).
  const void* w_t;
  const float* bias_t;
  void* z;
  int n_t, ldz, z_coff, act_t;
  int pair_1x1;
  // Split-K (v8 tiles, small-M layers: edge batches): K slice z of the launch writes its fp32
  // partial sums to slab z of ws [ksplit][M][Cout] with plain 16-B stores, and a finalize
  // kernel sums the slabs, applies bias, residual and activation and writes y.  ws = NULL:
  // v8 tiles refuse.  (ksplit is set by the tile; ws must hold ksplit x M x Cout floats.)
  float* ws;
  int ksplit;
  long long ws_elems;  // floats in ws
  // mode 4, second source extras (YOLO neck): channel offset of x2's slice, and up2 = 1: x2
  // is a half-resolution map read at (ho / 2, wo / 2) -- the nearest 2x upsample of the
  // concat folded into the GEMM (H2 = Ho / 2).  v2 LDS-DMA tiles (and their v7 / v8 forms)
  // only; every other family refuses.
  int x2_coff;
  int up2;
} KvConvParams;

// tile: -1 = heuristic; otherwise an index into the tile table (kv_conv_num_tiles()).
int kv_conv2d(const KvConvParams* p, int tile, hipStream_t stream);
// image-chunk size of kv_conv2d launches (bytes per operand per launch); 0 = default
long long kv_set_conv_chunk_bytes(long long bytes);
int kv_conv_num_tiles(void);
int kv_conv_splitk_base(void);       // split-K tiles: [base, base + splitk_num_tiles)
int kv_conv_splitk_num_tiles(void);
// host replay of the v6 (conv_nloop.hip) counted-wait schedules: 0 = every tile is safe
int kv_nloop_sched_check(void);
int kv_conv_pick_tile(const KvConvParams* p);
// v9 seam tiles (conv3 + residual -> next conv1, p->n_t set): valid tile arguments of a tail
// call are kv_conv_num_tiles() + i, i < kv_conv_seam_num_tiles()
int kv_conv_seam_num_tiles(void);
// Fused 3x3 + 1x1 pair on the v4 direct family (p->pair_1x1 = 1, see KvConvParams): tile =
// direct tile 0-3; < 0 when no instantiation covers the shape.
int kv_conv_pair(const KvConvParams* p, int tile, hipStream_t stream);
int kv_conv_pair_num_tiles(void);

// K5: max pool NHWC (k x k, stride, pad); C % 8 == 0.  ldx/ldy allow channel slices.
// Fused ResNet stem (4x4 stride-1 conv over the s2d image [N,H,W,16], Cout 64, weights
// [64][256] packed, bias, ReLU) + 3x3/2 max pool -> y [N,(H+1)/2,(W+1)/2,ldy] at y_coff.
int kv_stem_pool(const void* x, const void* w, const float* bias, void* y, int N, int H, int W,
                 int ldy, int y_coff, hipStream_t s);
int kv_stem_pool_lds_bytes(int W);
int kv_stem_pool_frames(const void* frames, const void* w, const float* bias, void* y, int N,
                        int H0, int W0, const float* mean3, const float* inv_std3, int ldy,
                        int y_coff, hipStream_t s);
// second-generation frames-in stem + pool (stem12.hip): 12-channel s2d, K = 192, w [64][192]
int kv_stem12_pool_frames(const void* frames, const void* w, const float* bias, void* y, int N,
                          int H0, int W0, const float* mean3, const float* inv_std3, int ldy,
                          int y_coff, hipStream_t s);
int kv_stem12_lds_bytes(int Ws);
// YOLOv8n b0 + b1 fused from raw frames (yolo_stem2.hip): w0 [16][64] frames-in s2d stem,
// w1 [32][w1_ld] 3x3/2 16 -> 32; y [N, H0/4, W0/4, 32]
int kv_yolo_stem2(const void* frames, const void* w0, const float* bias0, const void* w1,
                  int w1_ld, const float* bias1, void* y, int N, int H0, int W0, hipStream_t s);
int kv_yolo_stem2_lds_bytes(int Ws);

int kv_maxpool2d(const void* x, void* y, int N, int H, int W, int C, int ldx, int x_coff,
                 int ldy, int y_coff, int k, int stride, int pad, int Ho, int Wo, hipStream_t s);
// K5b: YOLOv8 SPPF: buf holds [x | y1 | y2 | y3] channel slices (4*C wide); x is
// already written in slice 0; writes y1=mp5(x), y2=mp5(y1), y3=mp5(y2) in one pass.
int kv_sppf_pool(void* buf, int N, int H, int W, int C, hipStream_t s);
// K6: global average pool NHWC -> [N, C] bf16.
int kv_global_avgpool(const void* x, void* y, int N, int HW, int C, hipStream_t s);
// K6+K1 at edge batches: y[n, :ncls] = bf16(fc(bf16(mean over HW of x[n]))), x [N, HW, C] bf16,
// w [ncls][ldw] bf16 (packed 1x1 conv weight), bias fp32 [ncls] or NULL.
int kv_pooled_fc(const void* x, int N, int HW, int C, const void* w, int ldw, const float* bias,
                 void* y, int ncls, hipStream_t s);
// K7: row softmax, bf16 [rows, cols] -> fp32 probabilities; also writes argmax.
int kv_softmax_rows(const void* x, float* y, int64_t* argmax, int rows, int cols, hipStream_t s);
// K8: nearest 2x upsample of x [N,H,W,C] written into channel slice of y [N,2H,2W,ldy].
int kv_upsample2x(const void* x, void* y, int N, int H, int W, int C, int ldx, int x_coff,
                  int ldy, int y_coff, hipStream_t s);
// K9: YOLOv8 decode (DFL softmax + expectation + dist2bbox + class sigmoid/max).
//   feats: per level bf16 [N, HW_l, 64 + nc]; out boxes fp32 [N, A, 4] xyxy,
//   scores fp32 [N, A], cls int32 [N, A].  A = sum HW_l.
int kv_yolo_decode(const void* f0, const void* f1, const void* f2, int h0, int w0, int h1,
                   int w1, int h2, int w2, int s0, int s1, int s2, int N, int nc,
                   float* boxes, float* scores, int* cls, hipStream_t s);
// K10: class-aware NMS per image: score threshold, sort, greedy IoU suppression,
//   keep <= max_det.  out fp32 [N, max_det, 6] (x1,y1,x2,y2,score,cls); count int32 [N].
int kv_nms(const float* boxes, const float* scores, const int* cls, int N, int A,
           float conf_thres, float iou_thres, int max_det, float* out, int* count,
           hipStream_t s);
// K11: on-device synthetic camera frames, uint8 NHWC3, deterministic in (seed, step).
int kv_synth_frames(uint8_t* y, int N, int H, int W, uint64_t seed, uint64_t step,
                    hipStream_t s);
// K11b: same but the step counter is read from device memory and incremented, so a
// captured hipGraph produces fresh frames on every replay.  bump_done = 1: step[1] is a
// zeroed finished-block count and the kernel's last block advances step[0] (one launch);
// 0: a one-thread kernel after it does.
int kv_synth_frames_dev(uint8_t* y, int N, int H, int W, uint64_t seed, uint64_t* step,
                        int bump_done, hipStream_t s);
// K12: uint8 NHWC3 -> bf16 NHWC4 normalized ((x/255 - mean)/std), channel 3 = 0.
int kv_preprocess(const uint8_t* x, void* y, int N, int H, int W, const float* mean3,
                  const float* inv_std3, hipStream_t s);
// K12b: uint8 NHWC3 -> bf16 space-to-depth [N, H/2, W/2, 16] normalized
//   (channel (dy*2+dx)*4 + c, c == 3 zero) for the stride-1 s2d stem conv.
int kv_preprocess_s2d(const uint8_t* x, void* y, int N, int H, int W, const float* mean3,
                      const float* inv_std3, hipStream_t s);
// K13 (frame_resize.hip): native-resolution uint8 frames [N,Hs,Ws,3] -> model-size uint8
// frames [N,Hd,Wd,3], bilinear with half-pixel centres in 11-bit fixed point (bit-identical
// to ops.reference.frame_resize).  Each axis is five ints {S, R, off, c0, cn}: source extent,
// extent of the virtual resized image, crop offset inside it, first destination index that
// holds content, number of content indices.  Destination pixels outside the content are
// `pad` in all three channels; every destination byte is written.  Wd % 4 == 0, extents in
// 1..8192.
int kv_frame_resize(const uint8_t* src, uint8_t* dst, int N, int Hs, int Ws, int Hd, int Wd,
                    const int* axis_y, const int* axis_x, int pad, hipStream_t s);
// K14: kept boxes det fp32 [N,max_det,6] (x1,y1,x2,y2,score,cls; rows < count[n] only) from
// model coordinates back to source-frame pixels, in place:
// x = clamp((x - cx) * sx, 0, Ws), y = clamp((y - cy) * sy, 0, Hs).
int kv_det_to_source(float* det, const int* count, int N, int max_det, float cy, float sy,
                     float cx, float sx, int Hs, int Ws, hipStream_t s);
// K15 (roi_crop.hip): crop n * K + k of dst u8 [N*K,D,D,3] is the window of box row k of
// det fp32 [N,max_det,6] (x1,y1,x2,y2,score,cls in src pixels) cut from src u8 [N,Hs,Ws,3] and
// stretched to D x D with K13's fixed-point bilinear (bit-identical to
// ops.reference.roi_crop).  The window is clamped on the device to >= 1 x 1 inside the frame
// for any box, non-finite ones included; slots k >= min(max(count[n], 0), max_det) are `pad`;
// every destination byte is written.  D % 4 == 0, 1 <= K <= max_det, extents in 1..8192.
// Returns -1 D % 4, -2 extents, -3 K, -4 pad, -5 misaligned dst, -6 N or grid, -7 band.
int kv_roi_crop(const uint8_t* src, const float* det, const int* count, uint8_t* dst, int N,
                int Hs, int Ws, int max_det, int K, int D, int pad, hipStream_t s);
// ... with `band` destination rows per workgroup (4, 8, 16 or 32; 0 = the built-in choice):
// the probe's knob (tools/roi_crop_probe.py), same result for every band
int kv_roi_crop_band(const uint8_t* src, const float* det, const int* count, uint8_t* dst, int N,
                     int Hs, int Ws, int max_det, int K, int D, int pad, int band, hipStream_t s);
// K16 / K17 (frame_nv12.hip): K13 and K15 reading NV12 frames, src u8 [N, Hs * 3 / 2, Ws]
// (rows 0 .. Hs - 1 are Y; row Hs + (y >> 1), bytes x & ~1 and (x & ~1) + 1 are U and V of
// pixel (y, x)).  Each source tap is converted to RGB (integer BT.601 limited range, nv12.h)
// and the taps are blended as in K13, so the result equals K13 / K15 on the converted frame
// byte for byte.  Everything else as K13 / K15; in addition Hs and Ws are even (-8) and src is
// 2-byte aligned (-9).
int kv_frame_resize_nv12(const uint8_t* src, uint8_t* dst, int N, int Hs, int Ws, int Hd, int Wd,
                         const int* axis_y, const int* axis_x, int pad, hipStream_t s);
int kv_roi_crop_nv12(const uint8_t* src, const float* det, const int* count, uint8_t* dst, int N,
                     int Hs, int Ws, int max_det, int K, int D, int pad, hipStream_t s);
int kv_roi_crop_nv12_band(const uint8_t* src, const float* det, const int* count, uint8_t* dst,
                          int N, int Hs, int Ws, int max_det, int K, int D, int pad, int band,
                          hipStream_t s);
// K18 (track.hip): one IoU-tracker update of streams [slot0, slot0 + N) of state int32
// [S, kv_track_state_stride(T)] from the step's detections det fp32 [N,max_det,6] / count
// int32 [N] (batch row n is the next frame of stream slot0 + n); track_id int32 [N,max_det]
// gets each row's track id (-1: not confirmed, no free slot, or row >= count[n]), every
// element written.  Integer arithmetic on quarter-pixel boxes, bit-identical to
// ops.reference.track_update; the semantics and the state layout are at the top of track.hip.
// thr_q = floor(iou * 1024 + 0.5).  Other streams of `state` are neither read nor written.
// Returns -1 T not 64/128/192/256, -2 slot0 + N > S, -3 max_det outside 1..300, -4 max_age
// outside 0..255, -5 min_hits outside 1..255, -6 thr_q outside 1..1024, -7 misaligned state.
int kv_track_state_stride(int T);
int kv_track_update(const float* det, const int* count, int* state, int* track_id, int N, int S,
                    int slot0, int T, int max_det, int thr_q, int max_age, int min_hits,
                    int class_aware, hipStream_t s);
// K19 (zones.hip): line crossings and zone occupancy of streams [slot0, slot0 + N), one launch
// after the same step's kv_track_update.  track_state int32 [S, kv_track_state_stride(T)] is
// only read; zone_state int32 [S, kv_zone_state_stride(T)] (per-slot entries, then 48
// counters) is updated; table int32 [S, kv_zone_table_stride()] holds every stream's lines and
// polygon zones (read only); det / count as for K18.  zone_mask int32 [N,max_det] gets each
// row's zone bits, zone_counts int32 [N,48] the stream's counters after the step (line_fwd[8]
// line_back[8] zone_enter[8] zone_exit[8] zone_occ[8] zone_dwell[8]), every element written.
// Integer arithmetic, bit-identical to ops.reference.zone_update; semantics and both layouts
// are at the top of zones.hip.  The table lives in device memory, so its counts and its
// anchor mode are range-checked where it is built (ops.ZoneSet) and clamped in the kernel.
// Returns -1 T not 64/128/192/256, -2 slot0 + N > S, -3 max_det outside 1..300, -7 track or
// zone state not 16-byte aligned, -8 misaligned table.  N == 0 launches nothing.
int kv_zone_state_stride(int T);
int kv_zone_table_stride(void);
int kv_zone_update(const float* det, const int* count, const int* track_state, int* zone_state,
                   const int* table, int* zone_mask, int* zone_counts, int N, int S, int slot0,
                   int T, int max_det, hipStream_t s);
// K20 (frame_watch.hip): per-camera frame watch of streams [slot0, slot0 + N): a motion grid
// against a running background, and the dark / flat / frozen / scene conditions with their run
// counters and alarms.  src uint8: RGB [N,Hs,Ws,3] (nv12 == 0) or NV12 [N,Hs*3/2,Ws] (luma only
// is read); state int32 [S, kv_watch_state_stride(GH * GW)], GH = ceil(Hs / cell), GW =
// ceil(Ws / cell), holds the header (primed, run[5], raised[5], the six thresholds, which are
// clamped in the kernel) and the per-cell planes acc | sum | grad.  stats int32 [N,16] and mask
// uint8 [N,GH,GW]: every element written.  Integer arithmetic, bit-identical to
// ops.reference.frame_watch; the rules and the layout are at the top of frame_watch.hip.
// Returns -1 Hs outside 1..4096 or Ws outside 2..4096, -2 slot0 + N > S, -3 cell not 8/16/32,
// -4 row_step not 1/2/4, -5 bg_shift outside 0..8, -6 odd NV12 size, -7 misaligned state or
// stats, -9 N too large.  N == 0 launches nothing.
int kv_watch_state_stride(int cells);
int kv_frame_watch(const unsigned char* src, int* state, int* stats, unsigned char* mask, int N,
                   int S, int slot0, int Hs, int Ws, int nv12, int cell, int row_step,
                   int bg_shift, hipStream_t s);
// K21 (jpeg_encode.hip): baseline JPEG files of images uint8 RGB [M,H,W,3], three launches.
// qtab int32 [2,64] (luminance, chrominance quantisers in natural order, clamped to 1..255),
// huff int32 [4,256] (code | length << 16 by symbol: DC lum, DC chroma, AC lum, AC chroma) and
// header uint8 [kv_jpeg_header_bytes()] are read from device memory at run time.  Workspaces,
// with mcu = 16 (sub420) or 8, mh = ceil(H / mcu), nb = ceil(W / mcu) * (6 | 3): coef int16
// [M,mh,nb,64] (16-byte aligned), scratch uint8 [M,mh,nb * kv_jpeg_block_bytes() + 16], seglen
// int32 [M,mh].  out uint8 rows of cap bytes: row m gets file m and length[m] its size, or
// length[m] = -size and no byte of the row when size > cap; bytes past the file are left alone.
// Byte-identical to ops.reference.jpeg_encode; the format is at the top of jpeg_encode.hip.
// Returns -1 H or W outside 1..8192, -2 M outside 0..65535, -3 cap outside 1..2^31-1, -4 the
// worst-case file exceeds 2^31-1 bytes, -7 misaligned operand.  M == 0 launches nothing.
int kv_jpeg_header_bytes(void);
int kv_jpeg_block_bytes(void);
int kv_jpeg_encode(const unsigned char* images, const int* qtab, const int* huff,
                   const unsigned char* header, short* coef, unsigned char* scratch, int* seglen,
                   unsigned char* out, int* length, int M, int H, int W, int sub420,
                   long long cap, hipStream_t s);
// K22 (annotate.hip): boxes, labels and the privacy mosaic drawn into images uint8 RGB
// [N,H,W,3] in place, one launch.  table int32 [S, kv_annotate_table_stride()] (image n uses
// row slot0 + n) and font int32 [kv_annotate_font_words()] are read from device memory at run
// time, every word clamped.  det fp32 [N,max_det,6] / count int32 [N] / track_id int32
// [N,max_det] in an (Hs, Ws) pixel frame; det == nullptr (then count and track_id too): only
// the polygons apply; track_id == nullptr: every id is -1.  Byte-identical to
// ops.reference.annotate; the rules and the layout are at the top of annotate.hip.
// Returns -1 H outside 1..8192 or W outside 4..8192 or W % 4, -2 N outside 0..65535 or
// slot0 + N > S, -3 max_det outside 1..300, -4 Hs or Ws outside 1..4096, -5 count missing (or
// given without det), -7 misaligned operand.  N == 0 launches nothing.
int kv_annotate_table_stride(void);
int kv_annotate_font_words(void);
int kv_annotate(unsigned char* images, const int* table, const int* font, const float* det,
                const int* count, const int* track_id, int N, int S, int slot0, int H, int W,
                int Hs, int Ws, int max_det, hipStream_t s);
// K4 fallback: y = x*scale[c] + shift[c] (+relu) on NHWC bf16.
int kv_batchnorm_nhwc(const void* x, void* y, const float* scale, const float* shift,
                      int64_t rows, int C, int relu, hipStream_t s);

// ---------------------------------------------------------------------------
// v13 fused YOLOv8 C2f(32, 32, n=1, shortcut) (c2f_fused.hip): t = SiLU(W1 . x + b1) (a =
// t[:16], s = t[16:]), u = SiLU(conv3x3(s) + bm1), v = s + SiLU(conv3x3(u) + bm2),
// y = SiLU(W2 . [a, s, v] + b2); NHWC bf16, x [N, H, W, ldx] at x_coff (32 channels), y at
// y_coff (32); packed weights w1 [32][ldw1], wm1 / wm2 [16][ldwm] (tap-major, cin minor),
// w2 [32][ldw2]; fp32 biases.  S: output rows per workgroup (a multiple of 4 dividing H).
// ---------------------------------------------------------------------------
typedef struct KvC2fParams {
  const void* x;
  void* y;
  const void* w1;
  const float* b1;
  const void* wm1;
  const float* bm1;
  const void* wm2;
  const float* bm2;
  const void* w2;
  const float* b2;
  int N, H, W, ldx, x_coff, ldy, y_coff;
  int ldw1, ldwm, ldw2;
  int S;
} KvC2fParams;
int kv_c2f16_supported(int H, int W, int S);
int kv_c2f16_fused(const KvC2fParams* p, hipStream_t stream);

#ifdef __cplusplus
}
#endif
