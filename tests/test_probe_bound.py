"""The probe bound never exceeds a file's true size: the
library's own arithmetic (icx_debug_probe_bound, host-only) against the
oracle's encoder, over image kinds, sizes and qualities - and it is not
vacuous on the content it is meant to decide."""
import pytest

from icx import _native as N
from tests.probe_bound_cases import KINDS, grey, lib_bound, list_sum

SIZES = [(16, 16, False), (64, 48, False), (200, 136, False), (1001, 67, False), (64, 48, True)]  # w, h, grey
QUALITIES = [0.02, 0.0625, 0.125, 0.25, 0.5, 0.75, 0.95, 1.0]


@pytest.mark.parametrize("w,h,g", SIZES)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_bound_never_exceeds_true_size(oracle, kind, w, h, g):
    img = KINDS[kind](h, w)
    if g:
        img = grey(img)
    for q in QUALITIES:
        total = list_sum(oracle, img, q)
        low = lib_bound(img, total)
        size = len(oracle.encode(img, q))
        assert 0 < low <= size, (kind, w, h, g, q, total, low, size)


def test_bound_is_not_vacuous_on_noise(oracle):
    img = KINDS["noise"](136, 200)
    low = lib_bound(img, list_sum(oracle, img, 0.25))
    size = len(oracle.encode(img, 0.25))
    assert size / 2 <= low <= size, (low, size)


def test_bound_arithmetic_and_argument_checks():
    L = N.load()
    # 16x16 colour: 6 blocks; the standard tables' cheapest DC difference is 2
    # bits, their cheapest nonzero AC coefficient 3 bits
    hdr = L.icx_jpeg_header_size_layout(N.BGR24, N.TABLES_SEPARATE)
    assert L.icx_debug_probe_bound(16, 16, N.BGR24, N.TABLES_SEPARATE, 6) == hdr + 2 + 2       # 12 bits
    assert L.icx_debug_probe_bound(16, 16, N.BGR24, N.TABLES_SEPARATE, 6 + 10) == hdr + 2 + 6  # 42 bits
    assert L.icx_debug_probe_bound(16, 16, N.RGB24, N.TABLES_GROUPED, 6 * 64) == \
        L.icx_jpeg_header_size_layout(N.RGB24, N.TABLES_GROUPED) + 2 + (12 + 3 * 6 * 63 + 7) // 8
    assert L.icx_debug_probe_bound(8, 8, N.GRAY8, N.TABLES_SEPARATE, 1) == \
        L.icx_jpeg_header_size_layout(N.GRAY8, N.TABLES_SEPARATE) + 2 + 1
    for bad in [(0, 16, N.BGR24, 0, 6), (16, 16, N.XRGB32, 0, 6), (16, 16, N.BGR24, 2, 6), (16, 16, N.BGR24, 0, 5),
                (16, 16, N.BGR24, 0, 6 * 64 + 1)]:
        assert L.icx_debug_probe_bound(*bad) == -1, bad
