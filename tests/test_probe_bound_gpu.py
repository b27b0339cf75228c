"""The probe bound on the device: a cached probe whose
candidate lists prove it too big is decided without a trial - and nothing a
caller sees changes.  Every case runs the normal fit entry point three ways:
the oracle, a context with the bound (the default) and a context created
under ICX_PROBE_BOUND=0; bytes and every result field must agree, and the
`bound` profile stat must be what the CPU restatement of the bound predicts."""
import os

import numpy as np
import pytest

import icx
from icx import _native as N
from tests.oracle_ffi import noise, smooth
from tests.probe_bound_cases import flat, grey, probe_bound

pytestmark = pytest.mark.gpu

Q = 0.25  # cached probe quality = the search's upper bound: the list filter is the probe's own thresholds


@pytest.fixture(scope="module")
def codec_off(codec):
    """A second context with the shortcut off (the variable is read once, at creation)."""
    old = os.environ.get("ICX_PROBE_BOUND")
    os.environ["ICX_PROBE_BOUND"] = "0"
    try:
        c = icx.Codec(0)
    finally:
        if old is None:
            del os.environ["ICX_PROBE_BOUND"]
        else:
            os.environ["ICX_PROBE_BOUND"] = old
    yield c
    c.close()


def nblocks(img):
    h, w = img.shape[:2]
    return int(N.load().icx_num_blocks(w, h, 2 if img.ndim == 2 else 0))


def trials(o):
    """The oracle's encode count less the final re-encode at the chosen
    parameters, which the library does not perform (its best trial is the file)."""
    return o["encodes"] - (1 if o["success"] and not o["cache_hit"] else 0)


def fit(c, imgs, target, q0, cached):
    c.profile(True)
    c.profile_reset()
    try:
        res = c.fit(imgs, target, q0, cached=[icx.LearnedParams(*p) for p in cached])
        stats = {k: c.profile_query(k)["units"] for k in ("bound", "huff")}
    finally:
        c.profile(False)
    return res, stats


def check(codec, codec_off, oracle, imgs, target, q0, cached, want_bound):
    """Fit on both contexts and the oracle: equal results; the shortcut taken
    for exactly want_bound images.  Returns the results and the stats."""
    on, st_on = fit(codec, imgs, target, q0, cached)
    off, st_off = fit(codec_off, imgs, target, q0, cached)
    assert st_off["bound"] == 0
    assert st_on["bound"] == want_bound, (st_on, want_bound)
    for i, img in enumerate(imgs):
        o = oracle.fit(img, target, q0, cached=cached[i])
        for r in (on[i], off[i]):
            assert r["status"] == N.OK
            assert r["success"] == o["success"], i
            assert r["cache_hit"] == o["cache_hit"], i
            assert r["encodes"] == trials(o), (i, r["encodes"], o["encodes"])
            assert r["out_len"] == (len(o["data"]) if o["success"] else 0), i
            if o["success"]:
                assert r["data"] == o["data"], i
                assert np.float32(r["learned"].quality) == np.float32(o["quality"]), i
                assert r["learned"].scale == o["scale"], i
        assert on[i] == off[i], i
    return on, st_on, st_off


def test_threshold(codec, codec_off, oracle):
    img = noise(64, 96, 31)
    low = probe_bound(oracle, img, Q)
    assert low <= len(oracle.encode(img, Q))
    check(codec, codec_off, oracle, [img], low - 1, Q, [(Q, 1.0)], 1)  # bound > target: decided
    check(codec, codec_off, oracle, [img], low, Q, [(Q, 1.0)], 0)      # bound == target: coded


@pytest.mark.parametrize("w,h,g", [(200, 136, False), (1001, 67, False), (64, 48, True)])
def test_image_kinds(codec, codec_off, oracle, w, h, g):
    img = noise(h, w, 32)  # 200x136, 1001x67: dummy blocks at the right and bottom edges
    if g:
        img = grey(img)
    check(codec, codec_off, oracle, [img], probe_bound(oracle, img, Q) - 1, Q, [(Q, 1.0)], 1)


def test_filter_below_probe(codec, codec_off, oracle):
    """A cached quality below the tree's: the lists also hold entries that are
    zero at the probe's quality, so no bound is taken."""
    img = noise(64, 96, 33)
    target = probe_bound(oracle, img, 0.1) - 1
    check(codec, codec_off, oracle, [img], target, Q, [(0.1, 1.0)], 0)


def test_resized_probe(codec, codec_off, oracle):
    """A cached scale below 1: the probe, and so the bound, is of the resized image."""
    img = noise(136, 200, 34)
    dw, dh = oracle.scaled_dims(200, 136, 0.85)
    low = probe_bound(oracle, oracle.resize(img, dw, dh), Q)
    check(codec, codec_off, oracle, [img], low - 1, Q, [(Q, 0.85)], 1)
    check(codec, codec_off, oracle, [img], low, Q, [(Q, 0.85)], 0)


def mixed_case(oracle):
    """One target for five images: `near` misses narrowly (bound <= target <
    its probe's size), the larger noise frames are proved too big, the flat
    and the smooth frame fit at the probe."""
    near = noise(64, 96, 35)
    low, size = probe_bound(oracle, near, Q), len(oracle.encode(near, Q))
    target = (low + size) // 2
    imgs = [noise(80, 144, 36), flat(48, 64), near, noise(96, 128, 37), smooth(48, 64, 38)]
    lows = [probe_bound(oracle, im, Q) for im in imgs]
    sizes = [len(oracle.encode(im, Q)) for im in imgs]
    return imgs, target, lows, sizes


def test_mixed_batch(codec, codec_off, oracle):
    imgs, target, lows, sizes = mixed_case(oracle)
    decided = [low > target for low in lows]
    assert decided == [True, False, False, True, False]
    assert [s <= target for s in sizes] == [False, True, False, False, True]
    on, st_on, st_off = check(codec, codec_off, oracle, imgs, target, Q, [(Q, 1.0)] * 5, 2)
    # every image ends at full scale (a probe hit, or a search at scale 1), so
    # each of its encodes is over nblocks(img) blocks: the huff units are the
    # coded block-trials, the decided probes left out
    assert all(r["success"] and r["learned"].scale == 1.0 for r in on)
    nb = [nblocks(im) for im in imgs]
    assert st_off["huff"] == sum(r["encodes"] * n for r, n in zip(on, nb))
    assert st_on["huff"] == sum((r["encodes"] - d) * n for r, n, d in zip(on, nb, decided))


def test_search_trace_unchanged(codec, codec_off, oracle):
    """icx_find_best_quality (no probe, no bound): every trial keeps its size."""
    img = noise(64, 96, 39)
    target = probe_bound(oracle, img, Q) - 1
    best, want = oracle.find_best_quality(img, target, Q)
    for c in (codec, codec_off):
        trace = []
        got = c.find_best_quality_by_binary_search(img, target, Q, trace)
        assert np.float32(got) == np.float32(best)
        assert [(np.float32(q), s) for q, s, _ in trace] == [(np.float32(q), s) for q, s in want]
        assert all(s > 0 for _, s, _ in trace)
