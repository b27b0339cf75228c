"""The host half of the device PNG filter route, without a GPU:
icx_png_encode_filtered writes, from an image's filtered rows, the file
icx_png_encode writes from its pixels; icx_png_filtered_size; the error
statuses; the batch calls' NULL-context statuses."""
import ctypes

import numpy as np
import pytest

from icx import FilteredPng, IndexedImage
from icx import _native as N
from icx.core import _image_struct
from icx.pngio import encode_png, encode_png_filtered

from tests.png_filter_cases import idat_stream, make_image, ref_stream

# (raster, h, w, content): the formats of the issue plus a grey + alpha map and a 4-bit palette
CASES = [("GRAY8", 9, 37, "ramp"), ("BGR24", 7, 23, "repeat"), ("ABGR32", 6, 19, "noise"),
         ("GRAY16", 5, 21, "gradient"), ("PALETTE", 8, 33, "noise"), ("GREYMAP", 8, 33, "ramp"),
         ("BINARY1", 6, 29, "noise"), ("GREYALPHA", 4, 11, "noise"), ("BINARY4", 5, 13, "noise")]


def _filtered(img, fmt, stream):
    im, _ = _image_struct(img, fmt)
    return FilteredPng(stream, im.width, im.height, im.fmt, img.palette if isinstance(img, IndexedImage) else None)


@pytest.mark.parametrize("name,h,w,kind", CASES)
def test_encode_filtered_equals_encode(name, h, w, kind):
    img, fmt = make_image(name, h, w, kind, 5)
    png = encode_png(img, fmt)
    stream = idat_stream(png)
    im, _ = _image_struct(img, fmt)
    assert stream.size == N.load().icx_png_filtered_size(ctypes.byref(im))
    assert encode_png_filtered(_filtered(img, fmt, stream)) == png
    for level in (0, 9):
        assert encode_png_filtered(_filtered(img, fmt, stream), level) == encode_png(img, fmt, level)
    ref = ref_stream(img, fmt)
    if name in ("GREYALPHA", "BINARY4"):
        assert ref is None
        return
    assert ref is not None  # png_ref covers every format the issue names
    assert np.array_equal(ref, stream)
    assert encode_png_filtered(_filtered(img, fmt, ref)) == png


def test_encode_filtered_many_idat_chunks():
    """A stream that deflates to several 32 KiB IDAT chunks."""
    img, fmt = make_image("BGR24", 120, 301, "noise", 9)
    png = encode_png(img, fmt)
    assert png.count(b"IDAT") >= 3
    assert encode_png_filtered(_filtered(img, fmt, idat_stream(png))) == png


def test_filtered_size():
    lib = N.load()

    def size(name, h, w):
        img, fmt = make_image(name, h, w, "zeros", 0)
        im, _ = _image_struct(img, fmt)
        return lib.icx_png_filtered_size(ctypes.byref(im))

    assert size("GRAY8", 5, 7) == 5 * (7 + 1)
    assert size("GRAY16", 5, 7) == 5 * (14 + 1)
    assert size("BGR24", 3, 10) == 3 * (30 + 1)
    assert size("XRGB32", 3, 10) == 3 * (30 + 1)
    assert size("ABGR32", 3, 10) == 3 * (40 + 1)
    assert size("PALETTE", 4, 9) == 4 * (9 + 1)
    assert size("GREYALPHA", 4, 9) == 4 * (18 + 1)
    assert size("BINARY1", 4, 9) == 4 * (2 + 1)
    assert size("BINARY4", 4, 9) == 4 * (5 + 1)
    assert lib.icx_png_filtered_size(None) == 0
    # where icx_png_bound is 0: no dimensions, a palette type without a map, over 1 GiB of rows
    for im in (N.Image(None, 0, 4, 0, N.GRAY8), N.Image(None, 4, 4, 4, N.INDEXED8),
               N.Image(None, 40000, 40000, 160000, N.RGBA32)):
        assert lib.icx_png_bound(ctypes.byref(im)) == 0
        assert lib.icx_png_filtered_size(ctypes.byref(im)) == 0


def test_encode_filtered_error_statuses():
    lib = N.load()
    img, fmt = make_image("BGR24", 4, 5, "noise", 1)
    stream = idat_stream(encode_png(img, fmt))
    meta, keep = _filtered(img, fmt, stream).meta()
    cap = lib.icx_png_bound(ctypes.byref(meta))
    out = np.empty(cap, np.uint8)
    n = ctypes.c_size_t()

    def call(meta_p, data, length, level, outp, capv, np_):
        return lib.icx_png_encode_filtered(meta_p, data, length, level, outp, capv, np_)

    m, d, o = ctypes.byref(meta), stream.ctypes.data, out.ctypes.data
    assert call(m, d, stream.size, -1, o, cap, ctypes.byref(n)) == N.OK
    assert call(None, d, stream.size, -1, o, cap, ctypes.byref(n)) == N.E_NULL
    assert call(m, None, stream.size, -1, o, cap, ctypes.byref(n)) == N.E_NULL
    assert call(m, d, stream.size, -1, None, cap, ctypes.byref(n)) == N.E_NULL
    assert call(m, d, stream.size, -1, o, cap, None) == N.E_NULL
    assert call(m, d, stream.size - 1, -1, o, cap, ctypes.byref(n)) == N.E_INVALID
    assert call(m, d, stream.size + 1, -1, o, cap, ctypes.byref(n)) == N.E_INVALID
    assert call(m, d, stream.size, 10, o, cap, ctypes.byref(n)) == N.E_INVALID
    n.value = 0
    assert call(m, d, stream.size, -1, o, cap - 1, ctypes.byref(n)) == N.E_BUFFER
    assert n.value == cap
    bad = N.Image(None, 5, 4, 15, 99)
    assert call(ctypes.byref(bad), d, stream.size, -1, o, cap, ctypes.byref(n)) == N.E_INVALID
    nomap = N.Image(None, 5, 4, 5, N.INDEXED8)
    assert call(ctypes.byref(nomap), d, stream.size, -1, o, cap, ctypes.byref(n)) == N.E_INVALID


def test_batch_calls_reject_null_context_without_gpu():
    lib = N.load()
    fj = (N.PngFilterJob * 1)()
    ffj = (N.PngFitFilterJob * 1)()
    assert lib.icx_png_filter_batch(None, fj, 1) == N.E_NULL
    assert lib.icx_png_fit_filter_batch(None, ffj, 1) == N.E_NULL
    assert lib.icx_pool_png_fit_filter_batch(None, ffj, 1) == N.E_NULL
    assert lib.icx_png_filter_batch(None, None, 0) == N.E_NULL
    assert lib.icx_png_fit_filter_batch(None, None, 0) == N.E_NULL
    assert lib.icx_pool_png_fit_filter_batch(None, None, 0) == N.E_NULL


def test_cli_flag():
    from icx.cli import build_parser
    base = ["-f", "l", "-o", "o"]
    assert build_parser().parse_args(base).png_filter == "device"
    assert build_parser().parse_args(base + ["--png-filter", "host"]).png_filter == "host"
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--png-filter", "cpu"])
