"""What the JPEG encoder tests share (test_jpeg_encode_cpu.py, test_jpeg_encode_gpu.py,
test_snapshots_*.py): the test images, each built to reach one branch of the entropy coder, and
a cache of the reference's files so that a case is encoded once per session."""
import functools
import io

import numpy as np
import torch

from kvedge_amd.ops import reference as ref

SUBSAMPLINGS = ("444", "420")
QUALITIES = (1, 50, 100)


def constant(h, w, rgb=(200, 60, 30)):
    return np.broadcast_to(np.asarray(rgb, np.uint8), (h, w, 3)).copy()


def noise(h, w, seed=0):
    """Independent RGB noise with half of the pixels pushed to pure black or white: the
    saturated pixels give the luminance the spread that reaches the top AC categories."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    bw = rng.random((h, w)) < 0.5
    v[bw] = (rng.integers(0, 2, int(bw.sum()), dtype=np.uint8) * 255)[:, None]
    return v


def smooth(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([xx * 255 // max(w - 1, 1), yy * 255 // max(h - 1, 1),
                     (xx + yy) * 255 // max(h + w - 2, 1)], -1).astype(np.uint8)


def bw_blocks(h, w):
    """8 x 8 blocks alternately all black and all white: the largest DC differences."""
    yy, xx = np.mgrid[0:h, 0:w]
    v = (((yy >> 3) + (xx >> 3)) & 1) * 255
    return np.repeat(v[..., None], 3, -1).astype(np.uint8)


def sparse_zrl(h, w):
    """Grey blocks holding only the highest-frequency basis function: after the quantiser
    coefficient 63 stands alone behind 62 zeros (three ZRLs, no EOB)."""
    k = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    tile = np.rint(128 + 100 * np.outer(k, k))
    v = np.tile(tile, (-(-h // 8), -(-w // 8)))[:h, :w]
    return np.repeat(v[..., None], 3, -1).astype(np.uint8)


CONTENT = {"constant": constant, "noise": noise, "bw_blocks": bw_blocks,
           "sparse_zrl": sparse_zrl, "smooth": smooth}


@functools.lru_cache(maxsize=None)
def image(name, h, w):
    a = CONTENT[name](h, w)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference_file(name, h, w, sub, quality):
    """(file bytes, stats) of the reference for one image; computed once."""
    files, stats = ref.jpeg_encode(image(name, h, w)[None], sub, quality, stats=True)
    return files[0], stats[0]


def as_tensor(*arrays):
    return torch.from_numpy(np.stack(arrays))


def decode(data):
    from PIL import Image

    im = Image.open(io.BytesIO(bytes(data)))
    im.load()
    return im


def psnr(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return 10 * np.log10(255.0 ** 2 / max(float(np.mean(d * d)), 1e-12))


def dqt_bytes(data):
    """The two 64-byte quantisation tables of a file's header."""
    return [bytes(data[o:o + 64]) for o in ref.JPEG_DQT_OFFSETS]
