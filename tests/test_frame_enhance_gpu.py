"""Low-light enhancement on the MI355X: the frame_enhance kernels against
ops.reference.frame_enhance byte for byte, with a canary image in front of and behind the batch,
in place and into ``out``."""
import pytest
import torch

from kvedge_amd import ops

pytestmark = pytest.mark.gpu

CANARY = 0xCD


def _images(kind, n, h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind == "dark":  # nearly every pixel in a handful of bins, heavy clipping
        return torch.randint(0, 21, (n, h, w, 3), dtype=torch.uint8, generator=g)
    if kind == "constant":  # everything in one bin: the residue rule
        return torch.full((n, h, w, 3), 37, dtype=torch.uint8)
    if kind == "full":
        return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)
    ramp = (torch.arange(w) * 255 // max(w - 1, 1)).to(torch.uint8)
    return ramp[None, None, :, None].expand(n, h, w, 3).contiguous()


def _twins(streams, hw, tiles, setup):
    cpu, gpu = ops.FrameEnhance(streams, hw, tiles), ops.FrameEnhance(streams, hw, tiles, "cuda")
    for e in (cpu, gpu):
        setup(e)
    assert torch.equal(gpu.params.cpu(), cpu.params) and torch.equal(gpu.axis.cpu(), cpu.axis)
    return cpu, gpu


def _check(images, cpu, gpu, slot0=0):
    """In place and into ``out``, each between two canary images; returns the reference's."""
    assert ops.load()
    n = images.shape[0]
    want, want_stats = ops.frame_enhance(images.clone(), cpu, slot0=slot0)
    for into_out in (False, True):
        buf = torch.full((n + 2, *images.shape[1:]), CANARY, dtype=torch.uint8, device="cuda")
        stats = torch.full((n, 2), -7, dtype=torch.int32, device="cuda")
        src = images.cuda() if into_out else buf[1:n + 1].copy_(images)
        got, got_stats = ops.frame_enhance(src, gpu, slot0=slot0, out_stats=stats,
                                           out=buf[1:n + 1] if into_out else None)
        torch.cuda.synchronize()
        assert got.data_ptr() == buf[1:].data_ptr() and got_stats.data_ptr() == stats.data_ptr()
        assert torch.equal(stats.cpu(), want_stats), (into_out, stats.cpu(), want_stats)
        assert torch.equal(buf[1:n + 1].cpu(), want), into_out
        assert bool((buf[0] == CANARY).all()) and bool((buf[n + 1] == CANARY).all()), into_out
        if into_out:
            assert torch.equal(src.cpu(), images)
    return want, want_stats


def _three_clips(e):
    """Clip 1.0 / 2.0 / 64.0; full, odd and auto-scaled strength."""
    e.set_clip(1.0, 0).set_clip(2.0, 1).set_strength(171, 1).set_clip(64.0, 2)
    e.set_mode("auto", 2).set_levels(4, 200, 2)


@pytest.mark.parametrize("kind", ["dark", "constant", "full", "ramp"])
@pytest.mark.parametrize("hw,tiles", [((8, 8), (1, 1)), ((12, 20), (2, 3)), ((40, 67), (8, 8)),
                                      ((64, 96), (16, 16))])
def test_against_the_reference(hw, tiles, kind):
    cpu, gpu = _twins(3, hw, tiles, _three_clips)
    images = _images(kind, 3, *hw)
    want, stats = _check(images, cpu, gpu)
    assert stats[:2, 1].tolist() == [256, 171]
    assert not torch.equal(want[0], images[0])  # nothing vacuous


def test_modes_off_on_and_auto_below_between_and_above_the_levels():
    def setup(e):
        e.set_mode("off", 0).set_mode("auto", 2).set_mode("auto", 3).set_mode("auto", 4)
        e.set_levels(24, 64, 2).set_levels(5, 15, 3).set_levels(2, 9, 4).set_strength(255, 3)

    cpu, gpu = _twins(5, (40, 67), (8, 8), setup)
    images = _images("dark", 5, 40, 67, seed=5)
    want, stats = _check(images, cpu, gpu)
    mean16 = stats[:, 0].tolist()
    assert all(150 <= m <= 170 for m in mean16)  # mean luma about 10
    alpha = stats[:, 1].tolist()
    assert alpha[:3] == [0, 256, 256] and 0 < alpha[3] < 255 and alpha[4] == 0
    assert torch.equal(want[0], images[0]) and torch.equal(want[4], images[4])


def test_one_bin_above_65535_catches_16_bit_counters():
    cpu, gpu = _twins(1, (260, 256), (1, 1), lambda e: e.set_clip(64.0))
    want, _ = _check(_images("constant", 1, 260, 256), cpu, gpu)
    assert int(want.max()) > 37


@pytest.mark.parametrize("n", [1, 2])
def test_slot0_one_of_three_cameras(n):
    cpu, gpu = _twins(3, (40, 68), (3, 5), _three_clips)
    luts = gpu.luts.clone()
    _check(_images("dark", n, 40, 68, seed=9), cpu, gpu, slot0=1)
    assert torch.equal(gpu.luts[0], luts[0])  # camera 0's tables are not touched
    with pytest.raises(ValueError):
        ops.frame_enhance(_images("dark", 3, 40, 68).cuda(), gpu, slot0=1)


def test_last_image_starts_beyond_2_31_bytes():
    n, hw = 44, (4096, 4096)
    frame = hw[0] * hw[1] * 3
    assert (n - 1) * frame > 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    if free < n * frame + (2 << 30):
        pytest.skip(f"needs {(n * frame >> 30) + 3} GiB of device memory")
    assert ops.load()
    gpu = ops.FrameEnhance(n, hw, device="cuda")
    images = torch.empty(n, *hw, 3, dtype=torch.uint8, device="cuda")
    images.random_(0, 21, generator=torch.Generator("cuda").manual_seed(2))
    last = images[n - 1:].cpu()
    got, stats = ops.frame_enhance(images, gpu)
    torch.cuda.synchronize()
    # cameras are independent: the reference runs the last one alone
    want, want_stats = ops.frame_enhance(last, ops.FrameEnhance(1, hw))
    assert torch.equal(stats[n - 1:].cpu(), want_stats)
    assert torch.equal(got[n - 1:].cpu(), want)


def test_captured_graph_reads_the_words_at_every_replay():
    cpu, gpu = _twins(2, (40, 68), (4, 4), lambda e: e)
    images = _images("dark", 2, 40, 68, seed=4)
    src, out = images.cuda(), torch.empty(2, 40, 68, 3, dtype=torch.uint8, device="cuda")
    stats = torch.empty(2, 2, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.frame_enhance(src, gpu, out=out, out_stats=stats)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        ops.frame_enhance(src, gpu, out=out, out_stats=stats)
    seen = []
    for change in (lambda e: e, lambda e: e.set_mode("off", 0).set_strength(90, 1),
                   lambda e: e.set_mode("on", 0)):
        change(cpu), change(gpu)
        g.replay()
        torch.cuda.synchronize()
        want, want_stats = ops.frame_enhance(images, cpu, out=torch.empty_like(images))
        assert torch.equal(out.cpu(), want) and torch.equal(stats.cpu(), want_stats)
        seen.append(out.cpu())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
