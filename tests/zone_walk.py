"""The 12-step walk and the region set shared by test_zones_cpu.py (which pins that the walk
is busy enough) and test_zones_gpu.py (which replays it on the device): S = 5 cameras of which
N = 3 are stepped from slot0 = 1, 8 rows each, 8 lines and 8 zones."""
import math

import torch

from kvedge_amd import ops

S, N, SLOT0, MAX_DET, STEPS = 5, 3, 1, 8, 12
TRACK_KW = dict(iou=0.3, max_age=2, min_hits=1, class_aware=True)
NAN, INF = float("nan"), float("inf")
ODD_ROWS = [  # the tracker test's rows no detector should emit
    (NAN, NAN, NAN, NAN), (NAN, 4.0, 20.0, NAN), (-INF, -INF, INF, INF), (INF, INF, -INF, -INF),
    (300.0, 200.0, 100.0, 50.0),  # inverted
    (12.0, 8.0, 12.0, 8.0),       # zero area
    (5000.0, 5000.0, 6000.0, 6000.0),  # beyond 4096 px
]
COUNTS = [(8, 8, 8), (8, 8, 7), (8, 6, 8), (8, 8, 8), (5, 8, 8), (8, 8, 8)]
# floors the reference alone must reach over the walk, so that no comparison is vacuous
MIN_CROSSINGS, MIN_ENTRIES, MIN_EXITS = 10, 10, 5

LINES = [  # (cameras, a, b, class)
    (None, (300.0, 0.0), (300.0, 800.0), -1),
    (None, (0.0, 350.0), (800.0, 350.0), -1),
    (None, (100.0, 100.0), (400.0, 400.0), -1),   # chained with the next one at (400, 400)
    (None, (400.0, 400.0), (700.0, 100.0), -1),
    (None, (200.0, 200.0), (200.0, 200.0), -1),   # A == B
    (None, (0.0, 520.0), (800.0, 450.0), 1),      # class 1 only
    ([SLOT0 + 1], (350.25, 300.0), (360.75, 420.5), -1),  # one camera, quarter pixels
    (None, (800.0, 0.0), (0.0, 800.0), -1),
]
ZONES = [  # (cameras, polygon, class)
    (None, [(50.0, 50.0), (450.0, 50.0), (450.0, 450.0), (50.0, 450.0)], -1),
    (None, [(300.0, 200.0), (700.0, 300.0), (350.0, 700.0)], -1),
    # 8 vertices, concave: a U opening upwards
    (None, [(100.0, 250.0), (200.0, 250.0), (200.0, 500.0), (500.0, 500.0), (500.0, 250.0),
            (600.0, 250.0), (600.0, 600.0), (100.0, 600.0)], -1),
    (None, [(0.0, 0.0), (800.0, 0.0), (800.0, 800.0), (0.0, 800.0)], 2),  # class 2 only
    # L shape
    (None, [(250.0, 100.0), (650.0, 100.0), (650.0, 300.0), (450.0, 300.0), (450.0, 650.0),
            (250.0, 650.0)], -1),
    ([SLOT0], [(380.0, 380.0), (420.5, 380.0), (420.5, 430.25), (380.0, 430.25)], -1),
    (None, [(100.0, 100.0), (300.0, 300.0), (500.0, 500.0)], -1),  # collinear: holds nothing
    (None, [(0.25, 300.25), (799.75, 300.25), (799.75, 420.75), (0.25, 420.75)], -1),
]


def regions(device="cpu", anchor="bottom"):
    """The ZoneSet of the walk: cameras 0 and S - 1 (never stepped) carry regions too."""
    zs = ops.ZoneSet(S, device)
    for i, (cams, a, b, cls) in enumerate(LINES):
        for cam in cams or [None]:
            zs.set_line(cam, i, a, b, cls=cls)
    for i, (cams, poly, cls) in enumerate(ZONES):
        for cam in cams or [None]:
            zs.set_zone(cam, i, poly, cls=cls)
    return zs.set_anchor(anchor)


def _walk(streams, objects, steps, seed, span=480.0):
    """[steps, streams, objects, 6]: boxes that swing out and back, up to 28 px a step with the
    speed changing smoothly (velocity * cos), so that the tracker keeps them through the turn
    and lines are crossed in both directions."""
    g = torch.Generator().manual_seed(seed)
    pos = 60.0 + torch.rand(streams, objects, 2, generator=g) * span
    size = 90.0 + torch.rand(streams, objects, 2, generator=g) * 60.0
    cls = torch.randint(0, 3, (streams, objects), generator=g).float()
    drift = (torch.rand(streams, objects, 2, generator=g) - 0.5) * 56.0
    phase = torch.rand(streams, objects, 1, generator=g) * 4.0
    out = []
    for step in range(steps):
        pos = pos + drift * torch.cos(math.pi * (step + phase) / (steps - 1))
        pos = pos + torch.randn(streams, objects, 2, generator=g) * 1.5
        box = torch.cat([pos, pos + size], dim=-1)
        score = torch.linspace(0.9, 0.1, objects).expand(streams, objects)
        out.append(torch.cat([box, score.unsqueeze(-1), cls.unsqueeze(-1)], dim=-1))
    return torch.stack(out)


WALK = _walk(N, MAX_DET, STEPS, seed=11)


def inputs(step):
    """(det [S, MAX_DET, 6], count [S]) of one step; the stepped cameras are rows
    SLOT0 .. SLOT0 + N - 1.  Every third step carries the odd rows; step 7 has a count past
    max_det and a negative one."""
    full = torch.zeros(S, MAX_DET, 6)
    full[SLOT0:SLOT0 + N] = WALK[step]
    if step % 3 == 2:
        for i, row in enumerate(ODD_ROWS):
            full[SLOT0 + i % N, (step + i) % MAX_DET, :4] = torch.tensor(row)
        full[SLOT0, 0, 5] = NAN
    cnt = torch.zeros(S, dtype=torch.int32)
    cnt[SLOT0:SLOT0 + N] = torch.tensor(COUNTS[step % len(COUNTS)], dtype=torch.int32)
    if step == 7:
        cnt[SLOT0] = 99   # past max_det: clamped
        cnt[SLOT0 + 1] = -3
    return full, cnt


def assert_busy(zone_state):
    """The floors, on the reference's zone state after the walk."""
    rows = slice(SLOT0, SLOT0 + N)
    fwd, back = int(zone_state.line_fwd[rows].sum()), int(zone_state.line_back[rows].sum())
    enter, leave = int(zone_state.zone_enter[rows].sum()), int(zone_state.zone_exit[rows].sum())
    assert fwd + back >= MIN_CROSSINGS and fwd >= 1 and back >= 1, (fwd, back)
    assert enter >= MIN_ENTRIES and leave >= MIN_EXITS, (enter, leave)
    return fwd, back, enter, leave
