"""Test inputs with Huffman and quantisation tables no encoder in this suite
writes (test infrastructure; plain Python + numpy, from ITU-T T.81).

recode() re-codes a baseline file's entropy-coded segment symbol by symbol
under other Huffman tables: every coefficient stays, only the tables, the
codes and the table selectors change.  The canonical table builders below
reach the parts of the device decoder that the Annex K tables leave idle
(icx_decode.h): its first level is 9 bits wide, the first 8 nine-bit prefixes
of longer codes get second-level tables, any further long code takes the
canonical maxcode loop (the slow path).  classes() counts a file's symbols by
those three classes with build_dec_huff's rule, so a test can prove that a
file exercises what its name claims.  rewrite_dqt() scales the quantisation
tables (8- or 16-bit, any table ids) and leaves the scan alone.

Every table built here is valid for libjpeg's jpeg_make_d_derived_tbl: no
length's codes reach the all-ones code.
"""
import functools

import numpy as np

LUT_BITS = 9   # ICX_DEC_LUT_BITS
NSUB = 8       # ICX_DEC_NSUB

# all AC symbols a baseline 8-bit file can hold: EOB, run 0..15 x size 1..10, ZRL.
# Ordered by size: codes of one length go out in this order, the first long
# prefixes get the second-level tables, so small sizes land in the second level
# and larger ones on the slow path - any image has plenty of both
AC_SYMBOLS = [0x00] + [r << 4 | s for s in range(1, 11) for r in range(16)] + [0xF0]
DC_SYMBOLS = list(range(16))


# ---------------------------------------------------------------- tables
def table(lengths):
    """(bits[16], vals) of a canonical table from [(symbol, length)], codes
    assigned in the order given within a length (T.81 Annex C)."""
    bits = [0] * 16
    vals = []
    for l in range(1, 17):
        for sym, sl in lengths:
            if sl == l:
                bits[l - 1] += 1
                vals.append(sym)
    code = 0
    for l in range(1, 17):
        # jpeg_make_d_derived_tbl: the codes of a length stay below the all-ones code
        assert code + bits[l - 1] < (1 << l), "code space exhausted at length %d" % l
        code = (code + bits[l - 1]) << 1
    assert len(set(vals)) == len(vals) == len(lengths)
    return bits, vals


def wide(vals, L):
    """The first symbol at 1 bit, the rest at L bits."""
    return table([(vals[0], 1)] + [(v, L) for v in vals[1:]])


def short01(vals=AC_SYMBOLS):
    """Symbol 0x01 at 1 bit, EOB at 2, the rest at 12: consecutive short codes,
    the most room for the lean tables' symbol pairs, next to slow-path codes."""
    return table([(0x01, 1), (0x00, 2)] + [(v, 12) for v in vals if v not in (0x00, 0x01)])


def dc_flat10():
    """All 16 DC symbols at 10 bits: codes 0..15, nine-bit prefixes 0..7 -
    exactly NSUB second-level tables and no slow entry (the boundary)."""
    return table([(v, 10) for v in DC_SYMBOLS])


def dc_flat16():
    """Every DC symbol at 16 bits: one prefix, the maximum code length."""
    return table([(v, 16) for v in DC_SYMBOLS])


def codes_of(bits, vals):
    """{symbol: (code, length)} of a (bits, vals) table."""
    out, code, k = {}, 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            out[vals[k]] = (code, l)
            code += 1
            k += 1
        code <<= 1
    return out


def symbol_classes(bits, vals):
    """{symbol: 0 first level | 1 second level | 2 slow} as build_dec_huff
    lays the table out: codes up to LUT_BITS long sit in the first level; the
    first NSUB distinct LUT_BITS-bit prefixes of longer codes, in code order,
    get second-level tables; codes under any later prefix take the slow loop."""
    out, prefixes = {}, []
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            if l <= LUT_BITS:
                out[vals[k]] = 0
            else:
                pre = code >> (l - LUT_BITS)
                if pre not in prefixes:
                    prefixes.append(pre)
                out[vals[k]] = 1 if prefixes.index(pre) < NSUB else 2
            code += 1
            k += 1
        code <<= 1
    return out


def long_prefixes(bits, vals):
    """Number of distinct LUT_BITS-bit prefixes of the table's longer codes."""
    pre = set()
    for sym, (code, l) in codes_of(bits, vals).items():
        if l > LUT_BITS:
            pre.add(code >> (l - LUT_BITS))
    return len(pre)


# ---------------------------------------------------------------- file structure
class Parsed:
    """A baseline file's header segments and scan."""
    pass


def parse(data):
    data = bytes(data)
    assert data[:2] == b"\xff\xd8"
    P = Parsed()
    P.segments = []          # (marker, payload) in file order, up to and including SOS
    P.tables = {}            # (class, id) -> (bits, vals), last definition wins
    P.qt = {}                # id -> (pq, 64 values in zig-zag order)
    P.ri = 0
    i = 2
    while True:
        assert data[i] == 0xFF, "marker expected at %d" % i
        while data[i + 1] == 0xFF:
            i += 1
        m = data[i + 1]
        n = int.from_bytes(data[i + 2:i + 4], "big")
        body = data[i + 4:i + 2 + n]
        P.segments.append((m, body))
        i += 2 + n
        if m == 0xC4:
            o = 0
            while o < len(body):
                tc, th = body[o] >> 4, body[o] & 15
                bits = list(body[o + 1:o + 17])
                cnt = sum(bits)
                P.tables[(tc, th)] = (bits, list(body[o + 17:o + 17 + cnt]))
                o += 17 + cnt
        elif m == 0xDB:
            o = 0
            while o < len(body):
                pq, tq = body[o] >> 4, body[o] & 15
                if pq:
                    v = [int.from_bytes(body[o + 1 + 2 * k:o + 3 + 2 * k], "big") for k in range(64)]
                else:
                    v = list(body[o + 1:o + 65])
                P.qt[tq] = (pq, v)
                o += 1 + (128 if pq else 64)
        elif m in (0xC0, 0xC1):
            P.h = int.from_bytes(body[1:3], "big")
            P.w = int.from_bytes(body[3:5], "big")
            P.comps = [(body[6 + 3 * c], body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c])
                       for c in range(body[5])]
        elif m == 0xDD:
            P.ri = int.from_bytes(body[:2], "big")
        elif m == 0xDA:
            ns = body[0]
            assert ns == len(P.comps) and bytes(body[1 + 2 * ns:]) == b"\x00\x3f\x00", "one interleaved scan"
            P.td_ta = [(body[2 + 2 * k] >> 4, body[2 + 2 * k] & 15) for k in range(ns)]
            break
        else:
            assert m not in (0xC2, 0xC3) and not 0xC5 <= m <= 0xCF, "baseline Huffman files only"
    # the entropy-coded segment: intervals between RSTn markers, unstuffed
    P.intervals, P.rst = [], []
    cur = bytearray()
    while True:
        b = data[i]
        if b != 0xFF:
            cur.append(b)
            i += 1
            continue
        nx = data[i + 1]
        if nx == 0x00:
            cur.append(0xFF)
            i += 2
        elif nx == 0xFF:
            i += 1
        elif 0xD0 <= nx <= 0xD7:
            P.intervals.append(bytes(cur))
            P.rst.append(nx)
            cur = bytearray()
            i += 2
        else:
            assert nx == 0xD9, "scan ends at marker %02x" % nx
            P.intervals.append(bytes(cur))
            break
    hmax = max(c[1] for c in P.comps)
    vmax = max(c[2] for c in P.comps)
    if len(P.comps) == 1:
        P.mcu_blocks = [0]
        P.nmcu = -(-P.w // 8) * -(-P.h // 8)
    else:
        P.mcu_blocks = [c for c, (_, h, v, _) in enumerate(P.comps) for _ in range(h * v)]
        P.nmcu = -(-P.w // (8 * hmax)) * -(-P.h // (8 * vmax))
    return P


class _Reader:
    def __init__(self, buf):
        self.buf = buf + b"\xff" * 4
        self.pos = 0
        self.n = 8 * len(buf)

    def peek16(self):
        p = self.pos
        w = int.from_bytes(self.buf[p >> 3:(p >> 3) + 4], "big")
        return (w >> (16 - (p & 7))) & 0xFFFF

    def take(self, n):
        v = 0
        while n > 0:
            k = min(n, 16)
            v = v << k | self.peek16() >> (16 - k)
            self.pos += k
            n -= k
        return v


def _decoder(bits, vals):
    """T.81 F.2.2.3 DECODE: per length, (first code, last code + 1, index of the first value)."""
    rows, code, k = [], 0, 0
    for l in range(1, 17):
        rows.append((l, code, code + bits[l - 1], k))
        code = (code + bits[l - 1]) << 1
        k += bits[l - 1]

    def dec(r):
        v = r.peek16()
        for l, lo, hi, k0 in rows:
            c = v >> (16 - l)
            if lo <= c < hi:
                r.pos += l
                return vals[k0 + c - lo]
        raise ValueError("no code within 16 bits at bit %d" % r.pos)
    return dec


def symbols(P, tables=None):
    """The scan as one list per restart interval of (component, class, symbol,
    extra bits' value, number of extra bits), decoded with the file's own
    tables (or `tables`, keyed as the file's SOS selects them)."""
    tables = tables or P.tables
    dec = {k: _decoder(*t) for k, t in tables.items()}
    out, mcu = [], 0
    for iv, buf in enumerate(P.intervals):
        r = _Reader(buf)
        ev = []
        last = iv == len(P.intervals) - 1
        stop = P.nmcu if last or not P.ri else min(P.nmcu, mcu + P.ri)
        while mcu < stop:
            for c in P.mcu_blocks:
                td, ta = P.td_ta[c]
                s = dec[(0, td)](r)
                ev.append((c, 0, s, r.take(s), s))
                k = 1
                while k < 64:
                    rs = dec[(1, ta)](r)
                    run, s = rs >> 4, rs & 15
                    ev.append((c, 1, rs, r.take(s), s))
                    if s == 0 and run != 15:
                        break
                    k += run + 1
                assert k <= 64, "run past the end of a block"
            mcu += 1
        assert r.pos <= r.n and r.n - r.pos < 8, "interval %d: %d bits left" % (iv, r.n - r.pos)
        out.append(ev)
    assert mcu == P.nmcu
    return out


def _dht(defs):
    return b"".join(bytes([tc << 4 | th]) + bytes(bits) + bytes(vals) for (tc, th), (bits, vals) in defs)


def _seg(m, body):
    return bytes([0xFF, m]) + (len(body) + 2).to_bytes(2, "big") + bytes(body)


def recode(data, tables, td_ta=None, split_dht=False, stale=None):
    """`data` with its scan re-coded under `tables` {(class, id): (bits, vals)}.
    td_ta: new (DC id, AC id) per component (default: the file's).  split_dht:
    one DHT segment per table instead of one for all.  stale: definitions
    {(class, id): (bits, vals)} written before the real ones of the same ids,
    which a reader must overwrite (the last definition wins)."""
    P = parse(data)
    td_ta = list(td_ta) if td_ta is not None else P.td_ta
    enc = {k: codes_of(*t) for k, t in tables.items()}
    scan = bytearray()
    for iv, ev in enumerate(symbols(P)):
        acc = nacc = 0
        body = bytearray()
        for c, cls, sym, extra, nextra in ev:
            code, l = enc[(cls, td_ta[c][cls])][sym]
            acc = (acc << l | code) << nextra | extra
            nacc += l + nextra
            while nacc >= 8:
                nacc -= 8
                body.append(acc >> nacc)
                acc &= (1 << nacc) - 1
        if nacc:  # byte-align with 1-bits (T.81 F.1.2.3)
            body.append((acc << (8 - nacc) | (1 << (8 - nacc)) - 1) & 0xFF)
        scan += bytes(body).replace(b"\xff", b"\xff\x00")
        if iv < len(P.rst):
            scan += bytes([0xFF, P.rst[iv]])
    out = bytearray(b"\xff\xd8")
    defs = sorted(tables.items())
    for m, body in P.segments:
        if m == 0xC4:
            continue
        if m == 0xDA:
            if stale:
                out += _seg(0xC4, _dht(sorted(stale.items())))
            if split_dht:
                for d in defs:
                    out += _seg(0xC4, _dht([d]))
            else:
                out += _seg(0xC4, _dht(defs))
            sel = b"".join(bytes([P.comps[c][0], td << 4 | ta]) for c, (td, ta) in enumerate(td_ta))
            body = bytes([len(td_ta)]) + sel + b"\x00\x3f\x00"
        out += _seg(m, body)
    return bytes(out + scan + b"\xff\xd9")


def classes(tables, data):
    """Symbols of the (re-coded) file's scan by decoder class: [first level,
    second level, slow].  tables: as the file's SOS selects them (None: the
    file's own DHT definitions)."""
    P = parse(data)
    tables = tables or P.tables
    cls_of = {k: symbol_classes(*t) for k, t in tables.items()}
    n = [0, 0, 0]
    for ev in symbols(P, tables):
        for c, cls, sym, _, _ in ev:
            n[cls_of[(cls, P.td_ta[c][cls])][sym]] += 1
    return n


def rewrite_dqt(data, factor, pq, ids=None):
    """`data` with every quantiser value multiplied by `factor` (capped at 255
    for 8-bit tables, pq=0), written as 8-bit (pq=0) or 16-bit (pq=1) tables in
    one DQT segment; ids {old: new} moves tables to other ids and fixes the
    frame header's selectors.  The scan is untouched."""
    P = parse(data)
    ids = ids or {}
    body = bytearray()
    for tq, (_, v) in sorted(P.qt.items()):
        v = [min(x * factor, 255) if pq == 0 else x * factor for x in v]
        # quantiser values above 32767 are outside what this suite pins: IJG 6b
        # multiplies in int, libjpeg-turbo's multiplier type is 16-bit, and the
        # two decode such files differently
        assert max(v) <= 32767
        body.append(pq << 4 | ids.get(tq, tq))
        body += b"".join(x.to_bytes(2, "big") for x in v) if pq else bytes(v)
    out, done = bytearray(b"\xff\xd8"), False
    for m, b in P.segments:
        if m == 0xDB:
            if not done:
                out += _seg(0xDB, body)
            done = True
            continue
        if m in (0xC0, 0xC1):
            b = bytearray(b)
            for c in range(b[5]):
                b[8 + 3 * c] = ids.get(b[8 + 3 * c], b[8 + 3 * c])
        out += _seg(m, b)
    sos = _seg(*P.segments[-1])
    return bytes(out) + bytes(data)[bytes(data).index(sos) + len(sos):]


# ---------------------------------------------------------------- the crafted set
def _pil_jpeg(img, **kw):
    import io

    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def crafted_set():
    """{name: (file, source file or None, kind)}: the inputs of
    test_decode_tables_cpu.py / test_decode_tables_gpu.py, built from seeded
    images.  kind "table": a re-coded twin of `source` (same coefficients,
    same pixels); "opt": a Pillow optimize=True file; "dqt": `source` with
    rewritten quantisation tables (same coefficients, other pixels).

    Sources: the smallest shapes that still span many subsequences once the
    subsequence length is forced to 2048 bits (the 64x96 noise file re-codes to
    17-24 KB, about 70-100 subsequences: more than one wave)."""
    from tests.oracle_ffi import noise, smooth
    rgb = lambda a: np.ascontiguousarray(a[:, :, ::-1])
    imgs = {
        "n420": (rgb(noise(64, 96, 31)), dict(quality=100, subsampling=2)),
        "s444r": (rgb(smooth(48, 64, 32)), dict(quality=90, subsampling=0, restart_marker_blocks=3)),
        "n422": (rgb(noise(33, 47, 33)), dict(quality=95, subsampling=1)),
        "grey": (np.ascontiguousarray(smooth(40, 56, 34)[:, :, 0]), dict(quality=85)),
    }
    src = {k: _pil_jpeg(a, **kw) for k, (a, kw) in imgs.items()}
    out = {}
    for k, data in src.items():
        own = parse(data).tables
        ids = sorted(own)
        ac = lambda t: {i: (t if i[0] == 1 else own[i]) for i in ids}
        dc = lambda t: {i: (t if i[0] == 0 else own[i]) for i in ids}
        for name, tabs in [("wide10", ac(wide(AC_SYMBOLS, 10))), ("wide12", ac(wide(AC_SYMBOLS, 12))),
                           ("wide16", ac(wide(AC_SYMBOLS, 16))), ("short01", ac(short01())),
                           ("dc10", dc(dc_flat10())), ("dc16", dc(dc_flat16()))]:
            out["%s_%s" % (k, name)] = (recode(data, tabs), data, "table")
        a, kw = imgs[k]
        out["%s_opt" % k] = (_pil_jpeg(a, optimize=True, **kw), None, "opt")
    # one-symbol tables with 1-bit codes
    out["flat8_opt"] = (_pil_jpeg(np.full((8, 8, 3), 77, np.uint8), quality=90, optimize=True), None, "opt")

    # table layouts on the 4:2:0 source
    data = src["n420"]
    W10, W12, W16, S01 = wide(AC_SYMBOLS, 10), wide(AC_SYMBOLS, 12), wide(AC_SYMBOLS, 16), short01()
    D10, D16, DW = dc_flat10(), dc_flat16(), wide(DC_SYMBOLS, 10)
    six = {(0, 0): D10, (0, 1): D16, (0, 2): DW, (1, 0): W10, (1, 1): S01, (1, 2): W12}
    out["n420_six_tables"] = (recode(data, six, td_ta=[(0, 0), (1, 1), (2, 2)]), data, "table")
    out["n420_ids23"] = (recode(data, {(0, 2): D10, (0, 3): DW, (1, 2): W12, (1, 3): W10},
                                td_ta=[(2, 2), (3, 3), (3, 3)]), data, "table")
    out["n420_two_slots"] = (recode(data, {(0, 1): DW, (1, 1): W10}, td_ta=[(1, 1)] * 3), data, "table")
    four = {(0, 0): D10, (0, 1): DW, (1, 0): W12, (1, 1): W10}
    out["n420_split_dht"] = (recode(data, four, split_dht=True), data, "table")
    # stale definitions of all four ids (other lengths, other symbol order), then the real ones
    stale = {(0, 0): D16, (0, 1): D10, (1, 0): wide(AC_SYMBOLS[::-1], 11), (1, 1): S01}
    out["n420_stale_dht"] = (recode(data, four, stale=stale), data, "table")

    # quantiser range (never a value above 32767: see rewrite_dqt)
    for k in ("n420", "grey"):
        for name, (f, pq, ids) in {"q8x3": (3, 0, None), "q8x20": (20, 0, None), "q16x3": (3, 1, None),
                                   "q16x40": (40, 1, None), "q16x500": (500, 1, None),
                                   "qids23": (3, 0, {0: 2, 1: 3})}.items():
            out["%s_%s" % (k, name)] = (rewrite_dqt(src[k], f, pq, ids), src[k], "dqt")
    return out
