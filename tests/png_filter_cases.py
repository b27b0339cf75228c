"""Shared by the PNG filter tests (test infrastructure only): the filtered
stream of an image from two references - the inflated IDAT of the host
encode_png's own file, and tests/png_ref.py's filter_rows over the rows in PNG
sample order - and the contents the filter is tried on."""
import struct
import zlib

import numpy as np

from icx import IndexedImage, default_palette
from icx import _native as N

from tests import png_ref


def idat_stream(png: bytes) -> np.ndarray:
    """The zlib-inflated IDAT chunks of a PNG file: its filtered rows."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    pos, z = 8, b""
    while pos < len(png):
        n, tag = struct.unpack(">I4s", png[pos:pos + 8])
        if tag == b"IDAT":
            z += png[pos + 8:pos + 8 + n]
        pos += 12 + n
    return np.frombuffer(zlib.decompress(z), np.uint8)


def grey_ramp_palette(alpha=False) -> np.ndarray:
    """A 256-entry map PNGMetadata writes as grey (or grey + alpha when some
    entry is not opaque): entry i is the grey level i."""
    a = ((np.arange(256, dtype=np.uint32) * 7 + 3) & 255) if alpha else np.full(256, 255, np.uint32)
    return (a << 24 | np.arange(256, dtype=np.uint32) * 0x010101).astype(np.uint32)


def sample_rows(img, fmt=None):
    """(rows in PNG sample order (h, row_bytes) uint8, RowFilter's
    bytesPerPixel, filtered) for the rasters png_ref covers; filtered = False
    for a palette image (filter 0 on every row).  None for the others."""
    if isinstance(img, IndexedImage):
        idx = img.indices
        if img.fmt == N.INDEXED8:
            ramp = np.array_equal(img.palette & 0xFFFFFF, np.arange(len(img.palette), dtype=np.uint32) * 0x010101) \
                and len(img.palette) == 256
            if ramp and np.all(img.palette >> 24 == 255):
                return idx, 1, True
            if ramp:
                return None  # grey + alpha: not in png_ref
            return idx, 1, False
        if len(img.palette) == 2 and list(img.palette) == [0xFF000000, 0xFFFFFFFF]:
            return np.packbits(idx & 1, axis=1), 1, True  # 1-bit grey
        return None
    if fmt is None:
        from icx.core import _fmt_of
        fmt = _fmt_of(img)
    h = img.shape[0]
    if fmt == N.GRAY8:
        return img.reshape(h, -1), 1, True
    if fmt == N.GRAY16:
        return np.ascontiguousarray(img.astype(">u2")).view(np.uint8).reshape(h, -1), 2, True
    if fmt in (N.BGR24, N.ABGR32):
        return np.ascontiguousarray(img[:, :, ::-1]).reshape(h, -1), img.shape[2], True
    if fmt in (N.RGB24, N.RGBA32):
        return img.reshape(h, -1), img.shape[2], True
    if fmt == N.XRGB32:
        return np.ascontiguousarray(img[:, :, 2::-1]).reshape(h, -1), 3, True
    if fmt == N.ARGB32:
        return np.ascontiguousarray(img[:, :, [2, 1, 0, 3]]).reshape(h, -1), 4, True
    return None


def ref_stream(img, fmt=None):
    """png_ref's filtered stream (flat uint8) or None where it has no say."""
    r = sample_rows(img, fmt)
    if r is None:
        return None
    rows, bpp, filtered = r
    if not filtered:
        return np.concatenate([np.zeros((rows.shape[0], 1), np.uint8), rows], axis=1).reshape(-1)
    return png_ref.filter_rows(np.ascontiguousarray(rows), bpp).reshape(-1)


# ---------------------------------------------------------------- contents
CONTENTS = ("noise", "gradient", "ramp", "repeat", "sparse", "zeros", "c200")


def content(kind, h, nbytes, seed):
    """(h, nbytes) uint8: noise; a smooth gradient; per-row random base plus a
    horizontal ramp; one noisy row repeated with sparse changes; sparse
    isolated ones; all zeros; constant 200 (the last two tie every filter)."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, (h, nbytes), dtype=np.uint8)
    if kind == "gradient":
        y, x = np.mgrid[0:h, 0:nbytes]
        return ((x * 3 // 4 + y * 5) & 255).astype(np.uint8)
    if kind == "ramp":
        base = rng.integers(0, 256, (h, 1))
        return ((base + np.arange(nbytes)[None, :] * 2) & 255).astype(np.uint8)
    if kind == "repeat":
        row = rng.integers(0, 256, nbytes, dtype=np.uint8)
        a = np.repeat(row[None, :], h, 0)
        mask = rng.random((h, nbytes)) < 0.01
        a[mask] = rng.integers(0, 256, int(mask.sum()), dtype=np.uint8)
        return a
    if kind == "sparse":
        return (rng.random((h, nbytes)) < 0.02).astype(np.uint8)
    if kind == "zeros":
        return np.zeros((h, nbytes), np.uint8)
    return np.full((h, nbytes), 200, np.uint8)


FORMATS = ("GRAY8", "GRAY16", "BGR24", "RGB24", "XRGB32", "ARGB32", "ABGR32", "RGBA32", "PALETTE", "GREYMAP",
           "GREYALPHA", "BINARY1", "BINARY4")


def make_image(name, h, w, kind, seed):
    """(image, fmt or None) of the named raster with the named content."""
    sb = {"GRAY8": 1, "GRAY16": 2, "BGR24": 3, "RGB24": 3}.get(name, 4 if name.endswith("32") else 1)
    raw = content(kind, h, w * sb, seed)
    if name == "GRAY8":
        return raw, N.GRAY8
    if name == "GRAY16":
        return np.ascontiguousarray(raw).view(np.uint16).reshape(h, w), N.GRAY16
    if name in ("BGR24", "RGB24"):
        return raw.reshape(h, w, 3), getattr(N, name)
    if name.endswith("32"):
        return raw.reshape(h, w, 4), getattr(N, name)
    if name == "PALETTE":
        return IndexedImage(raw, default_palette(False), N.INDEXED8), None
    if name == "GREYMAP":
        return IndexedImage(raw, grey_ramp_palette(), N.INDEXED8), None
    if name == "GREYALPHA":
        return IndexedImage(raw, grey_ramp_palette(True), N.INDEXED8), None
    if name == "BINARY1":
        return IndexedImage(raw & 1, default_palette(True), N.BINARY1), None
    pal = (0xFF000000 | np.arange(16, dtype=np.uint32) * 0x0F1011).astype(np.uint32)  # 4-bit palette, not a ramp
    return IndexedImage(raw & 15, pal, N.BINARY1), None
