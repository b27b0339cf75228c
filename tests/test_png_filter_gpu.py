"""The PNG row filter on the device (icx_png_filter_batch, the fused
icx_png_fit_filter_batch and the pipeline's --png-filter device route) against
two references: tests/png_ref.py's filter_rows over the rows in PNG sample
order, and the inflated IDAT of the host encode_png's own file."""
import os

import numpy as np
import pytest
from PIL import Image

import icx
from icx import DeviceImage, IndexedImage, pipeline
from icx import _native as N
from icx.core import CompressionParams
from icx.pngio import encode_png, encode_png_filtered

from tests.oracle_ffi import noise, smooth
from tests.png_filter_cases import CONTENTS, FORMATS, idat_stream, make_image, ref_stream

pytestmark = pytest.mark.gpu

# fewer bytes than bpp to the left and single rows; row lengths off every vector width
SHAPES = [(1, 1), (1, 7), (5, 1), (3, 2), (17, 341), (9, 1366)]


def _host_stream(img, fmt):
    return idat_stream(encode_png(img, fmt))


def _check(got, img, fmt, what):
    want = _host_stream(img, fmt)
    assert got.dtype == np.uint8 and got.size == want.size, what
    if not np.array_equal(got, want):
        n = want.size // img.shape[0]
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {bad.size} bytes differ from the host stream, first at row {bad[0] // n} "
                             f"byte {bad[0] % n}: got {got[bad[0]]}, want {want[bad[0]]} "
                             f"(types got {got[::n][:8]}, want {want[::n][:8]})")
    ref = ref_stream(img, fmt)
    if ref is not None:
        assert np.array_equal(got, ref), what + " (png_ref)"
    return ref


@pytest.mark.parametrize("h,w", SHAPES)
def test_device_stream_equals_references(codec, h, w):
    """Every format x every content at one shape, all in one call."""
    cases = [(f, c) for f in FORMATS for c in CONTENTS]
    made = [make_image(f, h, w, c, 11 + k) for k, (f, c) in enumerate(cases)]
    res = codec.png_filter_batch([m[0] for m in made], fmts=[m[1] for m in made])
    types = set()
    for (f, c), (img, fmt), r in zip(cases, made, res):
        assert (r.width, r.height) == (w, h)
        ref = _check(r.stream, img, fmt, f"{f} {c} {h}x{w}")
        if ref is not None and f != "PALETTE":
            types.update(int(t) for t in ref.reshape(h, -1)[:, 0])
    if h >= 9:  # the reference chose every filter type over these inputs: no subset passes
        assert types == {0, 1, 2, 3, 4}, types


def test_row_wider_than_any_tile(codec):
    """A 280 KB RGBA row: costs carry across the kernel's tiles."""
    h, w = 3, 70001
    kinds = ("noise", "ramp", "repeat", "sparse", "c200")
    made = [make_image("RGBA32", h, w, c, 3) for c in kinds]
    made.append(make_image("BGR24", 2, 50001, "ramp", 4))
    res = codec.png_filter_batch([m[0] for m in made], fmts=[m[1] for m in made])
    for c, (img, fmt), r in zip(kinds + ("bgr ramp",), made, res):
        _check(r.stream, img, fmt, f"wide {c}")


def test_mixed_call_host_and_device(codec):
    """One call mixing formats and sizes, host and DeviceImage inputs, host
    and device outputs."""
    spec = [("BGR24", 33, 257, "repeat"), ("GRAY16", 12, 100, "ramp"), ("ABGR32", 21, 97, "noise"),
            ("GRAY8", 40, 301, "sparse"), ("PALETTE", 9, 64, "noise"), ("BINARY1", 13, 75, "noise"),
            ("XRGB32", 5, 1201, "gradient"), ("GREYALPHA", 7, 31, "noise")]
    made = [make_image(f, h, w, c, 40 + k) for k, (f, h, w, c) in enumerate(spec)]
    lib = N.load()
    inputs, fmts, outs = [], [], []
    for k, (img, fmt) in enumerate(made):
        dev_in = k in (0, 2, 3)  # uint8 array rasters
        inputs.append(DeviceImage.from_host(codec, img) if dev_in else img)
        fmts.append(fmt)
        if k % 2:
            import ctypes
            from icx.core import _image_struct
            size = lib.icx_png_filtered_size(ctypes.byref(_image_struct(img, fmt)[0]))
            outs.append(DeviceImage(codec, (size,)))
        else:
            outs.append(None)
    res = codec.png_filter_batch(inputs, fmts=fmts, outputs=outs)
    for k, ((img, fmt), r) in enumerate(zip(made, res)):
        got = r.stream.numpy() if isinstance(r.stream, DeviceImage) else r.stream
        assert isinstance(r.stream, DeviceImage) == bool(k % 2)
        _check(got, img, fmt, f"mixed {spec[k]}")
    for x in inputs + outs:
        if isinstance(x, DeviceImage):
            x.free()


def test_job_statuses(codec):
    """Per-job statuses as icx_png_fit_batch's: a bad job fails alone."""
    import ctypes
    lib = N.load()
    img = noise(8, 8, 1)
    out = np.empty(8 * 25, np.uint8)
    jobs = (N.PngFilterJob * 4)()
    for j in jobs:
        j.img = N.Image(img.ctypes.data, 8, 8, 24, N.BGR24)
        j.out, j.cap = out.ctypes.data, out.nbytes
    jobs[1].img.px = None
    jobs[2].img.fmt = 42
    jobs[3].cap = out.nbytes - 1
    assert lib.icx_png_filter_batch(codec._ctx, jobs, 4) == N.OK
    assert [j.status for j in jobs] == [N.OK, N.E_NULL, N.E_INVALID, N.E_BUFFER]
    assert jobs[0].out_len == jobs[3].out_len == out.nbytes
    assert np.array_equal(out, _host_stream(img, N.BGR24))
    jobs[0].out = None
    assert lib.icx_png_filter_batch(codec._ctx, jobs, 1) == N.OK and jobs[0].status == N.E_NULL
    assert lib.icx_png_filter_batch(codec._ctx, None, 1) == N.E_NULL
    assert lib.icx_png_filter_batch(codec._ctx, jobs, -1) == N.E_INVALID
    fj = (N.PngFitFilterJob * 1)()
    fj[0].src = N.Image(img.ctypes.data, 8, 8, 24, N.BGR24)
    fj[0].min_width = fj[0].min_height = 4
    fj[0].out, fj[0].cap = out.ctypes.data, 3
    assert lib.icx_png_fit_filter_batch(codec._ctx, fj, 1) == N.OK
    assert fj[0].status == N.E_BUFFER and fj[0].out_len == 4 * (4 * 3 + 1) and (fj[0].out_w, fj[0].out_h) == (4, 4)


def _fit_group():
    rng = np.random.default_rng(7)
    pal = IndexedImage(rng.integers(0, 200, (260, 330), dtype=np.uint8),
                       (0xFF000000 | rng.integers(0, 1 << 24, 200)).astype(np.uint32), N.INDEXED8)
    bits = IndexedImage(rng.integers(0, 2, (301, 275), dtype=np.uint8), icx.default_palette(True), N.BINARY1)
    return [noise(300, 420, 1), np.ascontiguousarray(smooth(211, 517, 2)[:, :, 1]),
            rng.integers(0, 256, (233, 301, 4), dtype=np.uint8), noise(100, 140, 3),  # fits the box
            rng.integers(0, 65536, (190, 410), dtype=np.uint16), pal, bits, smooth(777, 333, 4)]


@pytest.mark.parametrize("pooled", [False, True])
def test_fused_fit_filter_equals_fit_then_encode(codec, pooled):
    imgs = _fit_group()
    params = CompressionParams(0.25, 1000, 150, 150, 60000)
    c = icx.Pool([0, 0]) if pooled else codec
    try:
        fused = c.png_fit_filter_batch(imgs, params)
        plain = c.png_fit_batch(imgs, params)
    finally:
        if pooled:
            c.close()
    assert [f is None for f in fused] == [p is None for p in plain] == [k == 3 for k in range(len(imgs))]
    for k, (f, p) in enumerate(zip(fused, plain)):
        if f is None:
            continue
        assert (f.height, f.width) == tuple(p.shape[:2])
        assert encode_png_filtered(f) == encode_png(p), k


def test_pipeline_device_and_host_filter_write_the_same_files(codec, tmp_path):
    rng = np.random.default_rng(3)
    src = tmp_path / "src"
    src.mkdir()
    Image.fromarray(np.ascontiguousarray(smooth(300, 420, 5)[:, :, ::-1])).save(src / "rgb.png")
    Image.fromarray(rng.integers(0, 256, (210, 330, 4), dtype=np.uint8), "RGBA").save(src / "rgba.png")
    Image.fromarray(np.ascontiguousarray(smooth(280, 390, 6)[:, :, 1])).save(src / "grey.png")
    Image.fromarray(rng.integers(0, 65536, (200, 310), dtype=np.uint16)).save(src / "grey16.png")
    Image.fromarray(np.ascontiguousarray(smooth(320, 440, 7)[:, :, ::-1])).quantize(200).save(src / "pal.png")
    Image.fromarray(noise(300, 400, 8)[:, :, 0]).convert("1").save(src / "bits.png")
    Image.fromarray(noise(90, 120, 9)).save(src / "small.png")  # fits the box: not written
    names = sorted(os.listdir(src))
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(str(src / n) for n in names))
    params = CompressionParams(0.25, 1000, 150, 150, 60000)
    reps, launches = {}, {}
    codec.profile(True)
    try:
        for mode in ("device", "host"):
            codec.profile_reset()
            reps[mode] = pipeline.CompressionBatch(lst, tmp_path / mode, params, 1, tmp_path / (mode + "cache"),
                                                   codecs=[codec], group_size=4, png_filter=mode).execute()
            launches[mode] = codec.profile_query("pngfilter")
    finally:
        codec.profile(False)
        codec.profile_reset()
    assert reps["device"].counts == reps["host"].counts and reps["device"].total == reps["host"].total == len(names)
    written = sorted(os.listdir(tmp_path / "host"))
    assert sorted(os.listdir(tmp_path / "device")) == written and len(written) == 6, written
    for n in written:
        assert (tmp_path / "device" / n).read_bytes() == (tmp_path / "host" / n).read_bytes(), n
    # a silent fall-back to the host filter would leave the device run without a launch
    assert launches["device"]["launches"] > 0 and launches["device"]["units"] > 0
    assert launches["host"]["launches"] == 0

