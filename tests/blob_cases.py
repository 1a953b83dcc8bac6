"""Grid patterns the motion-region tests share (test_motion_blobs_cpu.py / _gpu.py): a few lines
each, uint8 [GH, GW] with 1 = the cell moved."""
import torch

from kvedge_amd import ops

CELL = 16


def zeros(gh, gw):
    return torch.zeros(gh, gw, dtype=torch.uint8)


def serpentine(gh, gw):
    """One cell wide, half the grid: every other row whole, joined at alternating ends."""
    m = zeros(gh, gw)
    m[0::2] = 1
    m[1::4, gw - 1] = 1
    m[3::4, 0] = 1
    return m


def checkerboard(gh, gw):
    y, x = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
    return ((y + x) % 2 == 0).to(torch.uint8)


def comb(gh, gw):
    """Vertical bars on every other column, joined only along the bottom row."""
    m = zeros(gh, gw)
    m[:, 0::2] = 1
    m[gh - 1] = 1
    return m


def random(density, seed=7):
    def make(gh, gw):
        g = torch.Generator().manual_seed(seed)
        return (torch.rand(gh, gw, generator=g) < density).to(torch.uint8)
    return make


PATTERNS = {"zero": zeros, "one": lambda gh, gw: zeros(gh, gw) + 1, "serpentine": serpentine,
            "checker": checkerboard, "comb": comb, "rand10": random(0.1), "rand50": random(0.5)}


def regions_for(grid, streams=1, device="cpu"):
    """MotionRegions whose grid is ``grid`` at CELL, the last row and column of cells partial."""
    return ops.MotionRegions(streams, (grid[0] * CELL - 3, grid[1] * CELL - 5), CELL,
                             device=device)


def reference(mask, regions, slot0=0, max_blobs=16, connectivity=8):
    """ops.motion_blobs on CPU copies of ``mask`` and of the device tables of ``regions``."""
    cpu = ops.MotionRegions(regions.streams, regions.frame_hw, regions.cell)
    cpu.params.copy_(regions.params.cpu())
    cpu.ignore.copy_(regions.ignore.cpu())
    return ops.motion_blobs(mask.cpu(), cpu, slot0, max_blobs, connectivity)
