"""Decoder inputs with tables no encoder of this suite writes, pinned on the
CPU before the GPU sees them (tests/jpeg_recode.py, CPU suite).

Every other decoder test feeds Annex K Huffman tables (Pillow optimize=False,
the project's own encoder): 5 long-code prefixes per AC table, so the
second-level tables 5..7 and the canonical slow loop of icx_decode.h never run,
and quantiser-times-coefficient products stay in a real image's range.  Here:
 * re-coded twins of small files under crafted canonical tables decode to
   their source's pixels (libjpeg-turbo) and coefficients (oracle), and the
   class counts prove that each file reaches the second level / the slow loop;
 * files with scaled 8- and 16-bit quantisation tables decode in the oracle
   exactly as libjpeg-turbo without SIMD does (its SIMD IDCT differs from
   IJG's at such products), far into IDCT_range_limit's wrap;
 * the emulated device entropy decode (tests/dec_emu.cpp: the product's state
   machine and table builder) reproduces the oracle's coefficients for all of
   them, the lean walkers agree with the full ones, and only the six-table
   file leaves the device route (DecTab has four slots: host entropy decode).
"""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import jpeg_recode as R
from tests.test_decode_emu import emu, run  # noqa: F401  (the emulator fixture)


@pytest.fixture(scope="module")
def crafted():
    return R.crafted_set()


def _pil(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def _bgr(a):
    return a[:, :, ::-1] if a.ndim == 3 else a


def test_table_builders_cover_the_decoder_paths():
    """The counts the set's design rests on (9-bit first level, 8 second-level
    tables): Annex K's AC tables have 5 long prefixes (chroma DC: 1); the crafted ones have
    81, 21 (past 8: slow path) and 2 (second level only, 16-bit codes); the
    flat 10-bit DC table has exactly 8."""
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(b, "JPEG", quality=90)
    std = R.parse(b.getvalue()).tables
    assert [R.long_prefixes(*std[k]) for k in sorted(std)] == [0, 1, 5, 5]
    assert [R.long_prefixes(*R.wide(R.AC_SYMBOLS, L)) for L in (10, 12, 16)] == [81, 21, 2]
    assert R.long_prefixes(*R.dc_flat10()) == R.NSUB and R.long_prefixes(*R.dc_flat16()) == 1
    assert set(R.symbol_classes(*R.dc_flat10()).values()) == {1}
    assert set(R.symbol_classes(*R.short01()).values()) == {0, 1, 2}


def test_recoded_files_equal_their_sources(oracle, crafted):
    n = 0
    for name, (data, src, kind) in crafted.items():
        if kind != "table":
            continue
        assert np.array_equal(_pil(data), _pil(src)), name
        ref = oracle.jpeg_coefs(src)
        got = oracle.jpeg_coefs(data)
        assert got is not None and np.array_equal(got, ref), name
        rc, px = oracle.jpeg_decode(data)
        rc0, px0 = oracle.jpeg_decode(src)
        assert rc == 0 and rc0 == 0 and np.array_equal(px, px0), name
        n += 1
    assert n == 4 * 6 + 5


def test_optimised_files_decode_in_the_oracle(oracle, crafted):
    n = 0
    for name, (data, _, kind) in crafted.items():
        if kind != "opt":
            continue
        rc, px = oracle.jpeg_decode(data)
        assert rc == 0 and np.array_equal(px, _bgr(_pil(data))), name
        n += 1
    assert n == 5
    # the flat image's AC tables hold one symbol (EOB) at 1 bit, its DC tables at most two
    flat = R.parse(crafted["flat8_opt"][0]).tables
    assert all(bits[0] == 1 and vals == [0] for (tc, _), (bits, vals) in flat.items() if tc == 1)
    assert all(sum(bits) <= 2 and sum(bits[2:]) == 0 for bits, _ in flat.values())


def test_class_counts(crafted):
    """Each file reaches what its name claims (classes: first level, second
    level, slow)."""
    for name, (data, _, kind) in crafted.items():
        if kind != "table":
            continue
        first, second, slow = R.classes(None, data)
        what = name.split("_", 1)[1]
        if what in ("wide10", "wide12"):
            assert first > 0 and second > 0 and slow > 0, (name, first, second, slow)
        elif what == "wide16":
            assert second > 0 and slow == 0, (name, first, second, slow)
        elif what in ("dc10", "dc16"):
            assert second > 0 and slow == 0, (name, first, second, slow)
        elif what == "short01":  # (slow symbols only where the image has sizes above 4)
            assert first > 0 and second > 0, (name, first, second, slow)
        else:  # the layout variants mix all of them
            assert first > 0 and second > 0 and slow > 0, (name, first, second, slow)


_CHILD = r"""
import io, sys
import numpy as np
from PIL import Image
z = np.load(sys.argv[1])
np.savez(sys.argv[2], **{k: np.asarray(Image.open(io.BytesIO(z[k].tobytes()))) for k in z.files})
"""


def test_quantiser_range_oracle_equals_turbo_without_simd(oracle, crafted, tmp_path):
    """Scaled 8-bit and 16-bit quantisation tables, and tables at ids 2 and 3:
    the oracle's pixels equal libjpeg-turbo's with its SIMD IDCT off (a child
    process: turbo reads JSIMD_FORCENONE once), the coefficients are the
    source's, and more than a quarter of the samples sit at 0 or 255, i.e. the
    decode runs deep into IDCT_range_limit's saturation and wrap."""
    dqt = {k: v for k, v in crafted.items() if v[2] == "dqt"}
    assert len(dqt) == 12
    np.savez(tmp_path / "in.npz", **{k: np.frombuffer(v[0], np.uint8) for k, v in dqt.items()})
    r = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       env={**os.environ, "JSIMD_FORCENONE": "1"}, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    turbo = np.load(tmp_path / "out.npz")
    for name, (data, src, _) in dqt.items():
        rc, px = oracle.jpeg_decode(data)
        assert rc == 0, name
        assert np.array_equal(px, _bgr(turbo[name])), name
        assert np.array_equal(oracle.jpeg_coefs(data), oracle.jpeg_coefs(src)), name
        sat = float(np.mean((px == 0) | (px == 255)))
        assert sat > 0.25, (name, sat)
    # the scaled tables are what the names say
    q = R.parse(dqt["n420_q16x500"][0]).qt
    assert all(pq == 1 and max(v) == 500 for pq, v in q.values())
    assert sorted(R.parse(dqt["grey_qids23"][0]).qt) == [2]
    assert sorted(R.parse(dqt["n420_qids23"][0]).qt) == [2, 3]


@pytest.mark.parametrize("sub", [64, 1024])
def test_emulated_decode_of_the_crafted_set(emu, oracle, crafted, sub):
    """The product's table builder and walkers (the code the kernels compile)
    on the whole set: status 0 and the oracle's coefficients - the six-table
    file included, through the host route the product gives it."""
    for k, (name, (data, _, _)) in enumerate(crafted.items()):
        ref = oracle.jpeg_coefs(data)
        rc, got, _ = run(emu, data, ref.shape[0], seed=k + 1, sub=sub)
        assert rc == 0, (name, rc)
        assert np.array_equal(got, ref), name


def test_routes_and_lean_walkers_on_crafted_tables(emu, crafted):
    """Only a file with more than four distinct Huffman tables leaves the
    device's entropy decode; on every other crafted-table file the lean
    walkers (k_dec_init / k_dec_sync / k_dec_write) agree with the full state
    machine from random states, slow-path and second-level symbols included."""
    emu.dec_emu_lean_check.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    emu.dec_emu_lean_check.restype = ctypes.c_long
    emu.dec_emu_route.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    checked = 0
    for k, (name, (data, _, kind)) in enumerate(crafted.items()):
        buf = np.frombuffer(data, np.uint8)
        route = emu.dec_emu_route(buf.ctypes.data, buf.size)
        assert route == (1 if name == "n420_six_tables" else 0), (name, route)
        if kind == "dqt" or route:
            continue
        bad = emu.dec_emu_lean_check(buf.ctypes.data, buf.size, 64, 400, k + 1)
        assert bad == 0, (name, bad)
        checked += 1
    assert checked == 4 * 7 + 1 + 4
