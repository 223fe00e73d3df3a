"""Every entry point that reads ciphertext words, in the default dispatch, on
operands at and above n^2 (tests/wide_cases.py): a payload value anywhere in
[0, 2^(32 n2w)) reaches these kernels unreduced (the wire codec rejects only
wider values), and include/xhe.h promises the result for the operand mod n^2.
Every comparison is word-for-word equality with Python integers, which are
total there; all expected values are below n^2.

Keys: the golden fixtures, the structured keys "top" (n^2 of full width, q_max
= floor((2^(32 n2w) - 1) / n^2) of 1) and "bottom" (an n one bit short, q_max
around 15) at 2048, 3072 and 4096 bits, and for the n^2 operations the public
moduli 2^2048 - 159 and 2^2045 + 1 (q_max 63). The operations mod n^2 run on a
handle made from n alone, the decryption on a DJN private key with win_bits =
8 tables.

The Python reference is computed once per key for at most W.DISTINCT[K]
distinct tuples, tiled with a rolling start to the counts that select each
kernel shape (xfl_amd/csrc/paths.hpp; its names below), and every produced row
is compared:
  mulmod    17, 256 k_mulmod_wave (2048 bits); 300 ROW16 k_mulmod_n2; 4,200
            k_add_barrett for equal exponents (2048 bits), LANES4 k_mulmod_n2
  powmod    60 ROW16, 4,200 LANES4 (2048 bits: the digit kernels k_ndig_*);
            53-bit exponents, at 2048 bits also up to n - 1
  invert    1, 2, 3, 65 k_wtree_* (2048 bits); 4,200 the level tree
  segprod   60 and 4,200 elements, with gaps 0..3 (ALIGN), all-zero d and no d
            (WORDS); 4,200 in one segment
  multiexp  24 bases x 5 columns (k_mexp_horner_wave), 4,300 x 2
  pack      2048 bits, k = 7, shift 128: 41 groups (ROW16) and 4,101 (the
            digit kernel k_ndig_pack), the last group short
  decrypt   2048: 15 RNS, 1,100 ROW16, 5,200 QUAD4, 29,000 PMD1; 3072, 4096:
            15 ROW16, 6,000 k_dec_pmdx_*; 8192: 2, twice (four operands)
`units` operands are W.units_wide and W.wide mixed with residues below n^2, so
neighbouring lane groups take both sides of any entry branch; `nonunits` are
W.non_units (0, n, p, q, p^2, n^2 - n and their twins above n^2), where
Python is total as well: every operation but invert (tests/test_gpu_invert.py
holds its XHE_ENOINV on such a batch) and decrypt.
"""
import ctypes
import math
import random

import numpy as np
import pytest

from oracle import paillier_oracle as O
from tests import wide_cases as W
from tests.pack_cases import pack_ref
from tests.test_gpu_key_structure import Profile, _same, _tile

pytestmark = pytest.mark.gpu

WIN = 8  # fixed-base tables that build in milliseconds, as tests/pinned_cases.py WIN
N2_KEYS = W.key_names()
PRIV_KEYS = W.key_names(private_only=True)
KINDS = ("units", "nonunits")
DEC_BATCHES = {2048: (15, 1100, 5200, 29000), 3072: (15, 6000), 4096: (15, 6000), 8192: (2, 2)}
DEC_DISTINCT = {2048: 16, 3072: 8, 4096: 8, 8192: 4}  # (a decryption takes Python integers up to a second)


def _nat():
    from xfl_amd import _native as nat
    return nat


class Key:
    """one key's handles and operand lists, made once"""

    def __init__(self, name):
        nat = _nat()
        self.name = name
        self.K, self.n, self.p, self.q, self.h = W.key(name)
        self.n2 = self.n * self.n
        self.n2w = 2 * self.K // 32
        self.d = W.DISTINCT[self.K]
        self.small = self.K == 2048
        self.dk = nat.DeviceKey(self.K, self.n, None, None, None, device=0)
        assert self.dk.n2w == self.n2w

    def rng(self, what):
        return random.Random(f"wide-{self.name}-{what}")

    def operands(self, kind, what, units=False):
        """d operands: wide ones and residues below n^2 alternating (wide first, 3 in 4)"""
        n, n2, d = self.n, self.n2, self.d
        rng = self.rng(f"{kind}-{what}")
        if kind == "nonunits":
            assert not units
            return W.non_units(n, self.p or n, self.q or n, self.n2w, d, rng)
        ws = (W.units_wide if units else W.wide)(n, self.n2w, d - d // 4, rng)
        low = []
        for c in [1, n2 - 1, n + 1, 0][:3 if units else 4] + [rng.randrange(1, n2) for _ in range(d)]:
            if len(low) < d // 4 and (not units or math.gcd(c, n) == 1) and c not in low:
                low.append(c)
        out = W.mixed(ws, low)
        assert len(out) == d and 4 * sum(c >= n2 for c in out) >= 2 * d
        return out

    def up(self, ints):
        from xfl_amd.paillier import resident
        return resident.upload(_nat().ints_to_words(ints, self.n2w), 0)

    def up_words(self, w):
        from xfl_amd.paillier import resident
        return resident.upload(np.ascontiguousarray(w), 0)

    def words(self, ints, nw=None):
        return _nat().ints_to_words(ints, nw or self.n2w)


_keys = {}


def _key(name):
    if name not in _keys:
        _keys[name] = Key(name)
    return _keys[name]


def _down(t):
    from xfl_amd.paillier import resident
    return resident.download(t)


def _below(want, n2):
    assert all(0 <= x < n2 for x in want)
    return want


# ---------------------------------------------------------------- mulmod
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", N2_KEYS)
def test_mulmod_wide(name, kind):
    """equal exponents and gaps 0..3 in both directions; pairs wide on both
    sides, on the left only and on the right only"""
    from xfl_amd.paillier import resident
    k = _key(name)
    n2, d = k.n2, k.d
    rng = k.rng(f"mulmod-{kind}")
    x, y = k.operands(kind, "mulmod-a"), k.operands(kind, "mulmod-b")
    xw, yw = [c for c in x if c >= n2], [c for c in reversed(y) if c >= n2]
    xl, yl = [c for c in x if c < n2] + [n2 - 1], [c for c in y if c < n2] + [n2 - 1]
    # wide times wide, wide times narrow, narrow times wide
    a = [(xw, xw, xl)[i % 3][i // 3 % len((xw, xw, xl)[i % 3])] for i in range(d)]
    b = [(yw, yl, yw)[i % 3][i // 3 % len((yw, yl, yw)[i % 3])] for i in range(d)]
    if kind == "units":
        a[0] = b[0] = (1 << (32 * k.n2w)) - 1  # the largest product
    assert sum(u >= n2 and v >= n2 for u, v in zip(a, b)) >= d // 3 >= 2
    assert sum(u >= n2 > v for u, v in zip(a, b)) >= d // 3 and sum(v >= n2 > u for u, v in zip(a, b)) >= d // 3
    eq = [i % 5 - 40 for i in range(d)]
    ga = ([0, -3, 0, -1, -2, -3, -1, 0] + [rng.randrange(-3, 1) for _ in range(d)])[:d]
    gb = ([-3, 0, 0, -3, -2, 0, -2, -1] + [rng.randrange(-3, 1) for _ in range(d)])[:d]
    aw, bw = k.words(a), k.words(b)
    i32 = lambda v: np.asarray(v, dtype=np.int32).reshape(-1, 1)  # noqa: E731
    with Profile():
        for ea, eb, dmax in ((eq, eq, 0), (ga, gb, 3)):
            want = []
            for u, v, s, t in zip(a, b, ea, eb):
                lo = min(s, t)
                want.append(pow(u, 1 << (s - lo), n2) * pow(v, 1 << (t - lo), n2) % n2)
            ww = k.words(_below(want, n2))
            for count in (17, 256, 300, 4200):
                tl = lambda v: _tile(v, count, count)  # noqa: E731
                Profile.reset()
                out = resident.mulmod(k.dk, k.up_words(tl(aw)), tl(i32(ea)).reshape(-1), k.up_words(tl(bw)),
                                      tl(i32(eb)).reshape(-1), dmax)
                _same(_down(out), tl(ww), f"mulmod dmax={dmax} x {count}")
                Profile.ran(k_add_barrett=int(k.small and count == 4200 and dmax == 0))


# ---------------------------------------------------------------- powmod
def _pow_exponents(k, width, rng):
    if width == "full":
        n = k.n
        ks = [n - 1, 0, 1, (1 << 53) - 1, 0, 1, 15, 16] + [rng.randrange(n) for _ in range(k.d)]
        return ks[:k.d], n.bit_length()
    top = (1 << width) - 1
    ks = [top, 0, 1, 15, 0, 1, 16, 1 << (width - 1)] + [rng.getrandbits(width) for _ in range(k.d)]
    return ks[:k.d], width


@pytest.mark.parametrize("kind", ("units", "units-inverted", "nonunits"))
@pytest.mark.parametrize("name", N2_KEYS)
def test_powmod_wide(name, kind):
    """c^k and (c^-1)^k; the exponents 0 and 1 fall on wide bases (and k = 0
    on a non-unit: 1)"""
    from xfl_amd.paillier import resident
    k = _key(name)
    n2 = k.n2
    inverted = kind == "units-inverted"
    cs = k.operands(kind.split("-")[0], "powmod", units=kind != "nonunits")
    # (the operands under k = 0 and k = 1)
    assert cs[1] >= n2 if kind == "nonunits" else cs[0] >= n2 and cs[2] >= n2 and cs[4] >= n2
    cw = k.words(cs)
    with Profile():
        for width in (53, "full") if k.small else (53,):
            ks, kbits = _pow_exponents(k, width, k.rng(f"powmod-k-{width}"))
            assert ks[1] == 0 and ks[2] == 1 and ks[4] == 0
            want = [pow(c, e, n2) for c, e in zip(cs, ks)]
            if inverted:
                want = [pow(x, -1, n2) for x in want]
            assert kind != "nonunits" or want[1] == 1
            ww, kw = k.words(_below(want, n2)), k.words(ks, (kbits + 31) // 32)
            for count in (60, 4200) if width == 53 else (4200,):
                Profile.reset()
                out = resident.powmod(k.dk, k.up_words(_tile(cw, count, count)), _tile(kw, count, count), kbits,
                                      invert_first=inverted)
                _same(_down(out), _tile(ww, count, count), f"powmod {width} x {count}")
                Profile.ran(k_powmod_n2=1)


# ---------------------------------------------------------------- invert
@pytest.mark.parametrize("name", N2_KEYS)
def test_invert_wide(name):
    from xfl_amd.paillier import resident
    k = _key(name)
    cs = k.operands("units", "invert", units=True)
    cw, ww = k.words(cs), k.words(_below([pow(c, -1, k.n2) for c in cs], k.n2))
    for count in (1, 2, 3, 65, 4200):
        for start in (0, 2) if count <= 3 else (count,):  # (a batch of 1 .. 3 begins on a wide value, then on another)
            out = resident.invert(k.dk, k.up_words(_tile(cw, count, start)))
            _same(_down(out), _tile(ww, count, start), f"invert x {count}")


# ---------------------------------------------------------------- segprod
def _segprod(k, cs, d, dmax, has_d, seg, what):
    """xhe_segprod itself, as tests/pinned_cases.py _segprod calls it (the
    exponent array kept when it is all zero)"""
    import torch

    from xfl_amd.paillier import resident
    nat, dk, n2 = _nat(), k.dk, k.n2
    seg = np.asarray(seg, dtype=np.int64)
    pw = {}  # (c, d) -> c^(2^d): d distinct operands, 4 gaps
    want = []
    for s in range(len(seg) - 1):
        acc = 1
        for i in range(int(seg[s]), int(seg[s + 1])):
            key = (cs[i], d[i])
            if key not in pw:
                pw[key] = pow(cs[i], 1 << d[i], n2)
            acc = acc * pw[key] % n2
        want.append(acc)
    c = k.up(cs)
    dd = resident.upload(np.asarray(d, dtype=np.int32), 0) if has_d else None
    with resident._On(0):
        out = torch.empty((len(seg) - 1, dk.n2w), dtype=torch.int32, device="cuda:0")
    nat.check(nat.lib().xhe_segprod(dk.handle, resident._dp(c), resident._dp(dd), dmax, len(cs),
                                    seg.ctypes.data_as(ctypes.c_void_p), len(seg) - 1, resident._dp(out),
                                    resident._sp(0)), "segprod")
    _same(_down(out), k.words(_below(want, n2)), what)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", N2_KEYS)
def test_segprod_wide(name, kind):
    k = _key(name)
    distinct = k.operands(kind, "segprod")
    for count in (60, 4200):
        cs = [distinct[(count + i) % k.d] for i in range(count)]
        seg = [0, 0] + sorted({1, 1 + (count - 1) // 3, count})  # empty, one element, ragged
        gaps = [(7 * i + count) % 4 for i in range(count)]
        _segprod(k, cs, gaps, 3, True, seg, f"segprod gaps x {count}")
        _segprod(k, cs, [0] * count, 0, True, seg, f"segprod d = 0 x {count}")
        _segprod(k, cs, [0] * count, 0, False, seg, f"segprod no d x {count}")
    # one segment of wide elements only: every chunk of every level chains wide or just-reduced rows
    wide = [c for c in distinct if c >= k.n2]
    cs = [wide[i % len(wide)] for i in range(4200)]
    _segprod(k, cs, [0] * 4200, 0, False, [0, 4200], "segprod one segment, no d")
    _segprod(k, cs, [i % 4 for i in range(4200)], 3, True, [0, 4200], "segprod one segment, gaps")


# ---------------------------------------------------------------- multiexp
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", N2_KEYS)
def test_multiexp_wide(name, kind):
    from xfl_amd.paillier import resident
    k = _key(name)
    n2, KB = k.n2, 60
    distinct = k.operands(kind, "multiexp")
    with Profile():
        for nbases, ncols in ((24, 5), (4300, 2)):
            rng = k.rng(f"multiexp-{nbases}")
            bases = [distinct[(i + nbases) % k.d] for i in range(nbases)]
            nterms = min(nbases, 40)
            idx = [[rng.randrange(nbases) for _ in range(nterms)] for _ in range(ncols)]
            ex = [[rng.getrandbits(KB) for _ in range(nterms)] for _ in range(ncols)]
            ex[0][:3] = [0, 1, (1 << KB) - 1]
            idx[-1][-1] = nbases - 1
            want = []
            for j in range(ncols):
                acc = 1
                for t in range(nterms):
                    acc = acc * pow(bases[idx[j][t]], ex[j][t], n2) % n2
                want.append(acc)
            Profile.reset()
            out = resident.multiexp(k.dk, k.up(bases), idx, k.words([e for row in ex for e in row], 2), KB)
            _same(_down(out), k.words(_below(want, n2)), f"multiexp {nbases} x {ncols}")
            Profile.ran(k_mexp_horner=1)


# ---------------------------------------------------------------- pack
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", [name for name in N2_KEYS if W.key(name)[0] == 2048])
def test_pack_wide(name, kind):
    """k = 7, shift 128: 32 distinct groups, group g rotated by g, so wide
    values stand in the first, a middle and the last slot; tiled to 41 and
    4,101 groups, the last one of 3 elements"""
    from xfl_amd.paillier import resident
    k = _key(name)
    n2, kk, s = k.n2, 7, 128
    distinct = k.operands(kind, "pack")
    groups = [[distinct[(g + 3 * t) % k.d] for t in range(kk)] for g in range(k.d)]
    for slot in (0, 3, 6):
        assert any(g[slot] >= n2 for g in groups) and any(g[slot] < n2 for g in groups)
    full = pack_ref([c for g in groups for c in g], kk, s, n2)
    short = pack_ref([c for g in groups for c in g[:3] + [1] * 4], kk, s, n2)
    with Profile():
        for ngroups in (41, 4101):
            order = [(ngroups + j) % k.d for j in range(ngroups)]
            cs = [c for j in order for c in groups[j]][:kk * (ngroups - 1) + 3]
            want = [full[j] for j in order[:-1]] + [short[order[-1]]]
            Profile.reset()
            out = resident.pack(k.dk, k.up(cs), kk, s)
            _same(_down(out), k.words(_below(want, n2)), f"pack x {ngroups} groups")
            Profile.ran(k_pack=1)


# ---------------------------------------------------------------- decrypt
@pytest.mark.parametrize("name", PRIV_KEYS)
def test_decrypt_wide(name):
    nat = _nat()
    k = _key(name)
    K, d = k.K, DEC_DISTINCT[k.K]
    ok = O.derive_private(k.p, k.q, k.h)
    us = W.units_wide(k.n, k.n2w, d - d // 4, k.rng("decrypt"))
    cs = W.mixed(us, [k.n2 - 1, k.p * k.p + 1, 1, k.n + 1][:d // 4])
    assert all(math.gcd(c % k.n2, k.n) == 1 for c in cs) and sum(c >= k.n2 for c in cs) >= d // 2
    ms = [O.decrypt_raw(ok, c) for c in cs]
    assert ms[0] == O.decrypt_raw(ok, cs[0] % k.n2)
    assert ms[:2] != ms[1:3] and all(0 <= m < k.n for m in ms)
    cw, mw = k.words(cs), k.words(ms, K // 32)
    with Profile():
        dk = nat.DeviceKey(K, k.n, k.p, k.q, k.h, win_bits=WIN) if k.h else nat.DeviceKey(K, k.n, k.p, k.q, None)
        for i, count in enumerate(DEC_BATCHES[K]):
            Profile.reset()
            got = dk.decrypt_words(_tile(cw, count, 2 * i))
            _same(got, _tile(mw, count, 2 * i), f"decrypt x {count}")
            rns = int(K == 2048 and count <= 1024)
            Profile.ran(k_dec_rns=rns, k_dec_wave=0, k_dec_pow=1 - rns)
