"""CPU: every constant of a key's device blob against its defining identity.

xfl_amd/csrc/keyconst.hpp derives the constant blob and the KeyDev that points
into it on the host. tests/native/keyconst_check.cpp (its own main, built here
with ASan + UBSan like test_host_sanitize.py's harness, started as a separate
process) derives the image of a key, binds it to the host vector and prints
every KeyDev field with the limbs it points at. This module rebuilds Python
integers from the limbs and checks each constant against int/pow, for the five
golden keys in private form and the 2048-bit DJN key also in public form, for
the structured keys of tests/structured_keys.py whose primes sit at the ends of
their range (2048 bits: top, bottom and pattern; 3072 bits: bottom; as private
DJN keys), and that a field is present (non-null, 16-byte aligned, inside the blob, disjoint
from every other) exactly when a key of that size and kind uses it.

The RNS blocks' contents stay with tests/test_rns_constants.py.

Every key runs sanitized: BigU's division is bit-serial, but the sanitized
program needs 2.4 / 3.5 / 4.0 / 14.6 s for the 2048 / 3072 / 4096 / 8192-bit
private keys (measured on an 8-core build host), under the minute at which an
unsanitized build for the largest key would have been the plan.
"""
import os
import subprocess

import pytest

from tests.conftest import FIXTURES, hx, load_fixture

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
XHE_WIN_SPLIT = 0x100

# (fixture, private, window): the split layout on the key whose production window uses it
CASES = [(fx, True, 23 | XHE_WIN_SPLIT if fx == "paillier_2048_djn.json" else 16) for fx in FIXTURES]
CASES.append(("paillier_2048_djn.json", False, 16))
# structured_<bits>_<name>: tests/structured_keys.key(bits, name) as a private DJN key
CASES += [(f"structured_2048_{name}", True, 16) for name in ("top", "bottom", "pattern")]
CASES.append(("structured_3072_bottom", True, 16))


def _key_bits(fixture):
    return int(fixture.split("_")[1])  # paillier_<bits>_... / structured_<bits>_...


def _load_key(fixture):
    """the fixture's key record; for a structured key the same fields from structured_keys and the oracle"""
    if not fixture.startswith("structured_"):
        return load_fixture(fixture)["key"]
    from oracle import paillier_oracle as O
    from tests import structured_keys as SK
    k = SK.key(_key_bits(fixture), fixture.split("_", 2)[2])
    return {"n": hex(k.n), "p": hex(k.p), "q": hex(k.q), "djn_on": True, "h_pow_n": hex(k.h),
            "hp": hex(O.derive_private(k.p, k.q, k.h)["hp"])}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("keyconst") / "keyconst_check")
    # keydev.hpp takes uint2 from <hip/hip_vector_types.h>, which a host compiler reads with the platform macro
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", *SAN, "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    os.path.join(HERE, "native", "keyconst_check.cpp"), "-o", exe], check=True)
    return exe


class Image:
    """The parsed output of keyconst_check for one key."""

    def __init__(self, text, n, p, q, h, priv, djn):
        self.n, self.p, self.q, self.h, self.priv, self.djn = n, p, q, h, priv, djn
        self.K = 0
        self.scalars, self.fields = {}, {}
        for line in text.splitlines():
            t = line.split()
            if t[0] == "words":
                self.words = int(t[1])
            elif t[0] == "S":
                self.scalars[t[1]] = int(t[2])
            elif t[0] == "F":
                off, w, ln = int(t[2]), int(t[3]), int(t[4])
                assert t[5:] != ["OUT-OF-BLOB"], line[:80]
                assert len(t) == 5 + ln, (t[1], ln, len(t))
                self.fields[t[1]] = None if off < 0 else (off, w, [int(x, 16) for x in t[5:]])
        self.K = self.scalars["K"]

    def present(self, name):
        return self.fields[name] is not None

    def limbs(self, name):
        assert self.fields[name] is not None, f"{name} is null"
        return self.fields[name][2]

    def width(self, name):
        return self.fields[name][1]

    def val(self, name):
        w = self.width(name)
        ls = self.limbs(name)
        assert all(x < (1 << w) for x in ls), name
        return sum(x << (w * i) for i, x in enumerate(ls))

    def R(self, name):
        """2^(W S) of the row `name`."""
        return 1 << (self.width(name) * len(self.limbs(name)))

    def pairs(self, name):
        """(e, f, R) of a row of interleaved digit pairs."""
        w, ls = self.width(name), self.limbs(name)
        e = sum(x << (w * i) for i, x in enumerate(ls[0::2]))
        f = sum(x << (w * i) for i, x in enumerate(ls[1::2]))
        return e, f, 1 << (w * (len(ls) // 2))


_images = {}


def _image(case, program):
    fx, priv, win = case
    if case not in _images:
        k = _load_key(fx)
        n, p, q = hx(k["n"]), hx(k["p"]), hx(k["q"])
        djn = bool(k["djn_on"])
        h = hx(k["h_pow_n"]) if djn else None
        line = " ".join([f"{_key_bits(fx):x}", f"{(1 if priv else 0) | (2 if djn else 0):x}", f"{win:x}", f"{n:x}",
                         f"{p:x}" if priv else "-", f"{q:x}" if priv else "-", f"{h:x}" if djn else "-"]) + "\n"
        env = dict(os.environ)
        env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
        env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
        env.pop("LD_PRELOAD", None)  # the sanitizer runtime must come first in the child
        r = subprocess.run([program], input=line, capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        _images[case] = Image(r.stdout, n, p, q, h, priv, djn)
        _images[case].win, _images[case].key = win, k
    return _images[case]


def _cases(keep):
    """A fixture over the cases `keep` selects (the image of a key is derived once per module)."""
    @pytest.fixture(params=[c for c in CASES if keep(_key_bits(c[0]), c[1])],
                    ids=lambda c: f"{c[0][9:-5] if c[0].endswith('.json') else c[0][11:]}-"
                                  f"{'priv' if c[1] else 'pub'}-w{c[2] & 0xff}")
    def fixture(request, program):
        return _image(request.param, program)
    return fixture


img = _cases(lambda K, priv: True)
img_priv = _cases(lambda K, priv: priv)
img_2048 = _cases(lambda K, priv: K == 2048)
img_wide = _cases(lambda K, priv: K != 2048 and priv)


def _ceil_div(a, b):
    return -(-a // b)


MODS = ["N", "R1", "R2", "R3"]


def _expected_fields(im):
    K, priv, djn = im.K, im.priv, im.djn
    mods = ["n2", "n2X"]
    rows = ["n_words", "n2_words", "maxpos", "minneg", "n_lim", "nR2_n2", "n2.Rpow", "n2X.Rpow"]
    if K == 2048:
        mods += ["nd"]
        rows += ["n2_mu", "n2w_N", "n2w_np", "n2w_C", "n2w_R2", "nd_kn2", "nd_rmn", "nd_topc", "nd_dw", "nd_d1", "nd_dwt"]
    if priv:
        mods += ["p2", "q2", "p2L", "q2L", "p2X", "q2X", "p", "q"]
        rows += ["nR2_p2", "nR2_q2", "nR_p2", "nR_q2", "nR2_p2L", "nR2_q2L", "q2invR_p2", "q2_lim", "p2x4_lim",
                 "pm1_words", "qm1_words", "pinv_lim", "qinv_lim", "hpR", "hqR", "qinvpR", "q_lim", "p2x_lim", "p_lim",
                 "ep_words", "eq_words"]
        if djn:
            rows += ["nR2C_p2X", "nR2C_q2X", "R1C_p2X", "R1C_q2X", "hM_p2", "hM_q2"]
        if K == 2048:
            rows += ["p2_nprime", "q2_nprime", "rns", "rns_p", "rns_q", "topc_p", "topc_q"]
        else:
            mods += ["dp", "dq"]
            rows += [f"x_{c}_{x}" for c in ("kn2", "rmn", "topc", "fold", "dwt", "dw", "hpR") for x in "pq"]
    elif djn:
        rows += ["hM_n2"]
    return set(rows) | {f"{m}.{c}" for m in mods for c in MODS}


def test_presence(img):
    want = _expected_fields(img)
    assert want <= set(img.fields)
    spans = []
    for name, f in img.fields.items():
        assert (f is not None) == (name in want), f"{name}: {'unexpected' if f else 'missing'}"
        if f:
            off, _, ls = f
            assert off % 4 == 0 and len(ls) > 0 and off + len(ls) <= img.words, name
            spans.append((off, off + len(ls), name))
    spans.sort()
    for a, b in zip(spans, spans[1:]):
        assert a[1] <= b[0], f"{a[2]} overlaps {b[2]}"
    assert spans[-1][1] + 3 & ~3 == img.words  # nothing stored that no field names


def test_scalars(img):
    s, n = img.scalars, img.n
    assert (s["K"], s["nw"], s["n2w"]) == (img.K, img.K // 32, img.K // 16)
    assert (s["priv"], s["djn"], s["n_bits"]) == (int(img.priv), int(img.djn), n.bit_length())
    rb = n.bit_length() // 2 if img.djn else n.bit_length()
    assert (s["rand_bits"], s["rand_words"]) == (rb, (rb + 31) // 32)
    assert s["ndig"] == int(img.K == 2048) and s["pmdx_dec"] == int(img.priv and img.K != 2048)
    if img.djn:
        w, split = img.win & 0xff, bool(img.win & XHE_WIN_SPLIT) and img.priv
        nwin, nhi = _ceil_div(rb, w), 0
        if split and rb % w and rb % w <= rb // w:
            nwin, nhi = rb // w, rb % w
        assert nhi * (w + 1) + (nwin - nhi) * w >= rb
        assert (s["win"], s["nwin"], s["nhi"]) == (w, nwin, nhi)
    else:
        assert (s["win"], s["nwin"], s["nhi"]) == (0, 0, 0)


def _check_mod(im, name, N, npow=0):
    S, W = len(im.limbs(name + ".N")), im.width(name + ".N")
    R = 1 << (W * S)
    assert R > N
    assert im.val(name + ".N") == N, name
    assert im.val(name + ".R1") == R % N, name
    assert im.val(name + ".R2") == R * R % N, name
    assert im.val(name + ".R3") == R * R * R % N, name
    assert im.scalars[name + ".n0inv"] == (-pow(N, -1, 1 << W)) % (1 << W), name
    if npow:
        rows, S4 = im.limbs(name + ".Rpow"), (S + 3) & ~3
        assert len(rows) == npow * S4
        for j in range(npow):
            row = rows[j * S4:(j + 1) * S4]
            assert sum(x << (W * i) for i, x in enumerate(row)) == pow(R, j, N), (name, j)
    else:
        assert not im.present(name + ".Rpow")


def test_moduli(img):
    n, p, q = img.n, img.p, img.q
    _check_mod(img, "n2", n * n, 34)  # kRpowRows = kRawChunk + 2
    _check_mod(img, "n2X", n * n, 34)
    if img.K == 2048:
        _check_mod(img, "nd", n)
    if img.priv:
        for m in ("p2", "p2L", "p2X"):
            _check_mod(img, m, p * p)
        for m in ("q2", "q2L", "q2X"):
            _check_mod(img, m, q * q)
        _check_mod(img, "p", p)
        _check_mod(img, "q", q)
        if img.K != 2048:
            _check_mod(img, "dp", p)
            _check_mod(img, "dq", q)


def test_n_constants(img):
    n = img.n
    n2 = n * n
    assert img.val("n_words") == n and img.val("n2_words") == n2 and img.val("n_lim") == n
    assert img.val("maxpos") == n // 3 and img.val("minneg") == n - n // 3
    R = img.R("n2.N")
    assert img.val("nR2_n2") == n * R * R % n2
    if img.djn and not img.priv:
        assert img.val("hM_n2") == img.h * R % n2


def test_prime_square_constants(img_priv):
    img = img_priv
    n, p, q = img.n, img.p, img.q
    p2, q2 = p * p, q * q
    R, RL, RX = img.R("p2.N"), img.R("p2L.N"), img.R("p2X.N")
    assert img.val("q2_lim") == q2 and img.val("p2x4_lim") == 4 * p2
    for x, X2 in (("p2", p2), ("q2", q2)):
        assert img.val(f"nR2_{x}") == n * R * R % X2
        assert img.val(f"nR_{x}") == n * R % X2
        assert img.val(f"nR2_{x}L") == n * RL * RL % X2
    v = img.val("q2invR_p2")
    assert v < p2 and v * q2 % p2 == R % p2
    if img.djn:
        assert RX % R == 0
        C = (RX // R) ** img.scalars["nwin"]  # C = (R'/R)^nwin
        for x, X2 in (("p2", p2), ("q2", q2)):
            assert img.val(f"R1C_{x}X") == C * RX % X2
            assert img.val(f"nR2C_{x}X") == n * C * RX * RX % X2
            assert img.val(f"hM_{x}") == img.h * R % X2


def test_decrypt_constants(img_priv):
    img = img_priv
    n, p, q, s = img.n, img.p, img.q, img.scalars
    T = img.R("p.N")
    assert img.val("p_lim") == p and img.val("q_lim") == q and img.val("p2x_lim") == 2 * p
    v = img.val("qinvpR")
    assert v < p and v * q % p == T % p
    for x, X, Y in (("p", p, q), ("q", q, p)):
        v = img.val(f"{x}inv_lim")
        assert v < T and v * X % T == 1
        # hp = L_p((1 + n)^(p-1) mod p^2)^-1 mod p, the long way (the library uses the binomial shortcut)
        hx_ = pow((pow(1 + n, X - 1, X * X) - 1) // X, -1, X)
        assert img.val(f"h{x}R") == hx_ * T % X
        assert img.val(f"{x}m1_words") == X - 1 and s[f"{x}m1_bits"] == (X - 1).bit_length()
        e = n % (X * (X - 1))
        assert img.val(f"e{x}_words") == e and s[f"e{x}_bits"] == e.bit_length()
        if img.K != 2048:
            Rd = img.R("dp.N")
            assert img.val(f"x_hpR_{x}") == hx_ * Rd % X
    assert pow((pow(1 + n, p - 1, p * p) - 1) // p, -1, p) == hx(img.key["hp"])


def _check_topc(im, name, M):
    W, ls = im.width(name), im.limbs(name)
    R = 1 << (W * len(ls))
    E = (1 - R) % M
    assert ls == [((1 << W) - 1) + ((E >> (W * i)) & ((1 << W) - 1)) for i in range(len(ls))], name


def _check_digits(im, name, M, w):
    """(e, f) of w: e, f < M and R e + M f = w R^2 (mod M^2)."""
    e, f, R = im.pairs(name)
    assert e < M and f < M, name
    assert (R * e + M * f) % (M * M) == w * R * R % (M * M), name


def test_digit_constants_2048(img_2048):
    img = img_2048
    n = img.n
    n2 = n * n
    R = img.R("nd.N")
    assert img.val("nd_kn2") == _ceil_div(R, n) * n2 and img.val("nd_rmn") == R - n
    _check_topc(img, "nd_topc", n)
    _check_digits(img, "nd_d1", n, 1)
    _check_digits(img, "nd_dw", n, R * R)
    _check_digits(img, "nd_dwt", n, R * R * pow(img.R("n2.N"), -1, n2))
    if img.priv:
        assert img.R("topc_p") == img.R("p.N")
        _check_topc(img, "topc_p", img.p)
        _check_topc(img, "topc_q", img.q)


def test_digit_constants_wide(img_wide):
    img = img_wide
    for x, X, Y in (("p", img.p, img.q), ("q", img.q, img.p)):
        R = img.R("dp.N")
        assert img.val(f"x_kn2_{x}") == _ceil_div(R, X) * X * X and img.val(f"x_rmn_{x}") == R - X
        _check_topc(img, f"x_topc_{x}", X)
        assert img.val(f"x_fold_{x}") == Y * R ** 3 % X
        _check_digits(img, f"x_dw_{x}", X, R * R)
        _check_digits(img, f"x_dwt_{x}", X, R * R * pow(img.R("p2.N"), -1, X * X))


def test_wave_and_barrett_constants_2048(img_2048):
    img = img_2048
    n2 = img.n * img.n
    Rw, RX = img.R("n2w_N"), img.R("n2X.N")
    assert img.val("n2w_N") == n2
    v = img.val("n2w_np")
    assert v < Rw and (v * n2 + 1) % Rw == 0
    assert img.val("n2w_R2") == Rw * Rw % n2
    assert img.val("n2w_C") == Rw * Rw * pow(RX, -1, n2) % n2
    W, S1 = img.width("n2_mu"), len(img.limbs("n2_mu"))
    assert (W, S1) == (27, 153) and img.val("n2_mu") == (1 << (W * 2 * (S1 - 1))) // n2
    if img.priv:
        R = img.R("p2.N")
        for x, X in (("p2", img.p), ("q2", img.q)):
            v = img.val(f"{x}_nprime")
            assert v < R and (v * X * X + 1) % R == 0
