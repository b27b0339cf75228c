"""The device JPEG decoder on Huffman and quantisation tables that no encoder
of this suite writes (tests/jpeg_recode.py; the inputs and the oracle are
pinned by test_decode_tables_cpu.py).  Bit-exact against the oracle.

What only these files reach on the device: second-level tables 5..7 and the
canonical slow loop (dec_symbol_from, dec_lean_symbol), the write pass's
scalar second-level look-up (dec_lean_lookup(const SplitLean&): ballot,
readlane loop, half-word select) in waves whose lanes mix first-level,
second-level and slow symbols, 16-bit codes, one-symbol tables, table ids 2
and 3, redefined tables; idct_limit's saturation and wrap, 16-bit quantisers
and products far beyond a real image's.  Every clean batch also asserts that
no file left the device route (the dec_recovered counter): a recovery flag
firing on intact files would cost throughput and change no pixel.
"""
import numpy as np
import pytest

from icx import _native as N
from tests import jpeg_recode as R
from tests.oracle_ffi import load_decode_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def crafted():
    return R.crafted_set()


@pytest.fixture(scope="module")
def refs(oracle, crafted):
    """The oracle's pixels of every crafted file, computed once."""
    out = {}
    for name, (data, _, _) in crafted.items():
        rc, px = oracle.jpeg_decode(data)
        assert rc == 0, name
        px.setflags(write=False)
        out[name] = px
    return out


def _clean_batch(codec, datas, **kw):
    """decode_jpg_batch of intact files: none may take the recovery route."""
    codec.profile_reset()
    res = codec.decode_jpg_batch(datas, **kw)
    assert codec.profile_query("dec_recovered")["units"] == 0
    return res


def test_crafted_set_in_one_batch(codec, crafted, refs):
    names = list(crafted)
    res = _clean_batch(codec, [crafted[k][0] for k in names], subsampling=1)
    for name, (st, img) in zip(names, res):
        assert st == N.OK, (name, st)
        assert img.shape == refs[name].shape and np.array_equal(img, refs[name]), name


def test_crafted_set_source_subsampling(codec, oracle, crafted):
    names = [k for k in crafted if k.startswith(("n420_", "grey_"))]
    assert len(names) == 2 * 7 + 5 + 12
    res = _clean_batch(codec, [crafted[k][0] for k in names], subsampling=2)
    for name, (st, img) in zip(names, res):
        rc, ref = oracle.jpeg_decode(crafted[name][0], 2)
        assert st == N.OK and rc == 0, (name, st, rc)
        assert np.array_equal(img, ref), name


def test_crafted_table_coefficients(codec, oracle, crafted):
    n = 0
    for name, (data, _, kind) in crafted.items():
        if kind == "dqt":
            continue
        ref = oracle.jpeg_coefs(data)
        got = codec.debug_decode_coefs(data)
        assert got.shape == ref.shape and np.array_equal(got, ref), name
        n += 1
    assert n == 4 * 7 + 1 + 5


@pytest.mark.parametrize("sub_bits", [2048, 16384])
def test_crafted_set_forced_subsequence_lengths(codec, crafted, refs, monkeypatch, sub_bits):
    """At 2048 bits the re-coded 64x96 files span more than 64 subsequences:
    the sync and write walks run waves whose lanes sit on first-level,
    second-level and slow symbols in the same step."""
    for what in ("wide10", "wide12", "wide16", "short01"):
        data = crafted["n420_" + what][0]
        scan = len(data) - data.index(b"\xff\xda")
        assert scan * 8 // 2048 > 64, what
    monkeypatch.setenv("ICX_DEC_SUB_BITS", str(sub_bits))
    names = list(crafted)
    res = _clean_batch(codec, [crafted[k][0] for k in names], subsampling=1)
    for name, (st, img) in zip(names, res):
        assert st == N.OK, (name, st)
        assert np.array_equal(img, refs[name]), (sub_bits, name)


def test_crafted_and_standard_tables_in_one_batch(codec, crafted, refs):
    """Tables of a different shape per image in one launch: crafted-table files
    interleaved with standard-table goldens."""
    _, jpgs, pxs = load_decode_golden()
    names = [k for k, v in crafted.items() if v[2] != "dqt"]
    gold = ["c130x250_s2_q95", "rst7_130x250_444"]
    datas, want = [], []
    for i, k in enumerate(names):
        datas.append(crafted[k][0])
        want.append(refs[k])
        g = gold[i % 2]
        datas.append(jpgs[g])
        want.append(pxs[g])
    res = _clean_batch(codec, datas, subsampling=1)
    for i, ((st, img), ref) in enumerate(zip(res, want)):
        assert st == N.OK, (i, st)
        assert np.array_equal(img, ref), i


def test_recovery_counter_moves_on_a_damaged_file(codec, oracle, crafted):
    """The counter the clean batches watch does count: one truncated file
    among intact ones raises it by exactly one (and decodes as the oracle's
    IJG 6b recovery does)."""
    good = crafted["n420_wide12"][1]
    cut = good[:len(good) * 2 // 3]
    codec.profile_reset()
    res = codec.decode_jpg_batch([good, cut, crafted["n420_wide12"][0]], subsampling=1)
    assert codec.profile_query("dec_recovered")["units"] == 1
    rc, ref = oracle.jpeg_decode(cut)
    assert rc == 0 and res[1][0] == N.OK and np.array_equal(res[1][1], ref)
    assert res[0][0] == N.OK and res[2][0] == N.OK
