"""What the kernel tests share about the conv tile table and their closeness rule
(test_kernels_gpu.py, shadow.py, test_model_walk_gpu.py): one place, so a new tile family
moves every test that walks the table at once."""

RRMS_TOL = 4e-3  # rms(err) / rms(ref): ~2-3x the two sides' independent bf16 output rounding
MAX_REL = 0.02   # max |err| <= 2 % of max |ref|

# The conv tile table (kv_conv_num_tiles() entries): first index of each family
# v1 (0-5) + v2 (6-31) + v3 (32-53) + v4 (54-57) + v6 (58-67) + v7 BK32 MF16 /
# direct-epilogue / N-160 (68-85) + v8 split-K (86-104) + v10 (105-107) + v12 (108-116)
# + v14 (117-120)
N_TILES = 121
# v2: LDS-DMA implicit GEMM; 8-wave (512-thread) tiles 24-28 (256x256 x2, 256x128, 128x256,
# 256x128 D3) and the v_mfma_f32_16x16x32 forms 29-31 (128x128 4-wave, 256x256 and 256x128
# 8-wave)
V2_0 = 6
STREAM0 = 32     # v3 tiles take 1x1 stride-1 GEMMs and dual-source convs only
DIRECT0 = 54     # v4 direct 3x3 (conv_direct.hip): its instantiation table only
# v6 A-resident N-loop 1x1 GEMM (58-67, conv_nloop.hip kNlTiles: one Kpad per tile;
# 63-65 are the fused-downsample (dual) forms, 66-67 step 128 K at a time)
NLOOP0 = 58
XP0 = 68         # v7: the v2 kernel's cross-stage pipelined loop (BK 32 rings, 8 waves)
SK0 = 86         # v8: split-K (conv_sk.hip kSkTiles): K slices per tile (clamped to the K steps)
# v10: the direct family's direct-epilogue forms (conv_direct.hip): 8 waves at 1 / 2
# workgroups per CU, the single-patch-buffer 4-wave form at 2 per CU
DE0 = 105
# v12: skinny edge-batch implicit GEMM (conv_skinny.hip kSknTiles): general / 1x1 / dual
# convs whose every K source has Cin % 64 == 0, M < 65536
SKN0 = 108
# v14: 8-phase ping-pong implicit GEMM (conv_pp.hip): 256x256, 512x128, then their
# persistent forms (one workgroup per CU walking tiles); modes 0 (Cin % 64), 1, 4
PP0 = 117

# family name -> tile index range
FAMILIES = {
    "v1": range(0, V2_0), "v2": range(V2_0, STREAM0), "v3": range(STREAM0, DIRECT0),
    "v4": range(DIRECT0, NLOOP0), "v6": range(NLOOP0, XP0), "v7": range(XP0, SK0),
    "v8": range(SK0, DE0), "v10": range(DE0, SKN0), "v12": range(SKN0, PP0),
    "v14": range(PP0, N_TILES),
}


def rrms(got, ref) -> float:
    """Relative RMS error: a dropped K chunk or a wrong tap moves every element, which
    this sees even when one large output makes the max bound loose."""
    got, ref = got.float(), ref.float()
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-12)).item()


def assert_close(got, ref, ctx=None):
    got, ref = got.float(), ref.float()
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    rr = rrms(got, ref)
    assert err <= MAX_REL * scale and rr <= RRMS_TOL, (ctx, err, scale, rr)
