"""Shared by test_probe_bound.py / test_probe_bound_gpu.py: the probe bound's
input - the candidate-list length sum of an image at a quality - restated on
the CPU from the oracle's FDCT and quantisation tables, and the library's own
bound for it (icx_debug_probe_bound)."""
import numpy as np

from icx import _native as N
from tests.oracle_ffi import fmt_of, noise, smooth

# zig-zag position -> natural index (jpeg_natural_order)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
                   12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                   58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def flat(h, w, v=90):
    return np.full((h, w, 3), v, np.uint8)


def gradient(h, w):
    """Horizontal ramp, the same in every row and channel."""
    row = (np.arange(w) * 255 // max(1, w - 1)).astype(np.uint8)
    return np.ascontiguousarray(np.broadcast_to(row[None, :, None], (h, w, 3)))


def grey(img):
    return np.ascontiguousarray(img[:, :, 0])


KINDS = {"noise": lambda h, w: noise(h, w, 21), "smooth": lambda h, w: smooth(h, w, 22), "flat": flat,
         "gradient": gradient}


def list_sum(oracle, img, q):
    """Sum over the scan blocks of 1 (the DC) + the AC coefficients that
    quantise to nonzero at quality q: |c| >= d - d/2 with d = 8 * q[k]
    (jcdctmgr.c rounds |c| + d/2 down to a multiple of d)."""
    coefs = oracle.fdct(img).astype(np.int64)  # (blocks, 64), zig-zag order
    lum, chrom = (np.array(t, np.int64)[ZIGZAG] * 8 for t in oracle.qtables(q))
    thr = np.stack([lum - lum // 2, chrom - chrom // 2])
    nb = coefs.shape[0]
    comp = np.zeros(nb, np.int64) if img.ndim == 2 else (np.arange(nb) % 6 >= 4).astype(np.int64)
    nz = np.abs(coefs[:, 1:]) >= thr[comp][:, 1:]
    return int(nb + nz.sum())


def lib_bound(img, total, layout=N.TABLES_SEPARATE):
    h, w = img.shape[:2]
    return int(N.load().icx_debug_probe_bound(w, h, fmt_of(img), layout, total))


def probe_bound(oracle, img, q, layout=N.TABLES_SEPARATE):
    return lib_bound(img, list_sum(oracle, img, q), layout)
