"""Ciphertext packing on the CPU: pack_factor, a Python-integer model of the
pack that the oracle decrypts and unpack_columns takes apart again,
decrypt_unpack's index mapping, and the planner's paths::pack through
tests/native/pack_paths_check.cpp (plain g++, its own process)."""
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import paillier_oracle as O
from tests import pack_cases as PK
from tests.conftest import ROOT, hx, load_fixture

HERE = os.path.dirname(os.path.abspath(__file__))
B = 1 << 128


# ---------------------------------------------------------------- pack_factor
@pytest.mark.parametrize("bits,k", [(2048, 7), (3072, 11), (4096, 15), (8192, 31)])
def test_pack_factor_golden_keys(bits, k):
    from xfl_amd.paillier_acceleration import pack_factor
    n = PK.modulus(bits)
    assert n.bit_length() in (bits - 1, bits)
    assert pack_factor(n) == k
    assert pack_factor(n, 2, 1 << 128) == k
    assert pack_factor(n, 1, 1 << 128) == (n.bit_length() - 2) // 128


def test_pack_factor_boundaries():
    from xfl_amd.paillier_acceleration import pack_factor
    n = PK.modulus(2048)
    # k * num * 128 <= bitlen(n) - 2 (2045 or 2046): 15 slots of 128 bits fit once, 16 do not fit at all
    assert pack_factor(n, 15) == 1 and pack_factor(n, 16) == 0 and pack_factor(n, 8) == 1 and pack_factor(n, 7) == 2
    assert pack_factor(n, 2, 1 << 64) == 15 and pack_factor(n, 2, 1 << 256) == 3
    # a slot width the device does not unpack: no packing
    assert pack_factor(n, 2, 10 ** 38) == 0 and pack_factor(n, 2, 1 << 48) == 0 and pack_factor(n, 0) == 0
    # bitlen(n) - 1 = k * s exactly is one bit short (the packed value must keep its sign bit)
    m = (1 << 256) + 1  # bitlen 257: one 256-bit slot needs 258
    assert pack_factor(m, 1, 1 << 256) == 0 and pack_factor(m << 1, 1, 1 << 256) == 1


# ---------------------------------------------------------------- the model
def _plaintexts(count, rng):
    """(grad, hess) digit pairs: negative grads, zeros, the slot extremes"""
    top = (1 << 127) - 1
    edge = [(-top, top), (top, -top), (0, 0), (-1, 0), (0, -1), (top, top), (-top, -top), (1, 1)]
    pairs = edge + [(rng.randrange(-top, top + 1), rng.randrange(0, top + 1)) for _ in range(count)]
    rng.shuffle(pairs)
    return pairs[:count]


@pytest.mark.parametrize("count", [13, 7, 1])
def test_python_model_decrypts_and_unpacks(count):
    """pow and % on the golden key: the packed ciphertexts decrypt (oracle) to
    embed's layout with num * k slots, and unpack to the original values"""
    from xfl_amd.paillier_acceleration import _centred_digits, pack_factor, umbed, unpack_columns
    g = load_fixture(PK.FIXTURE[2048])
    key = g["key"]
    ok = O.derive_private(hx(key["p"]), hx(key["q"]), hx(key["h_pow_n"]))
    n = ok["n"]
    rng = random.Random(count)
    k, s = pack_factor(n), 256
    assert k == 7
    pairs = _plaintexts(count, rng)
    xs = [a * B + b for a, b in pairs]
    cts = [O.encrypt_m(ok, x % n, rng.randrange(1, ok["djn_exp_bound"])) for x in xs]
    packed = PK.pack_ref(cts, k, s, n * n)
    assert len(packed) == -(-count // k)
    ms = [O.signed_value(ok, O.decrypt_raw(ok, c)) for c in packed]
    padded = xs + [0] * (len(packed) * k - count)
    assert ms == [sum(x << (s * (k - 1 - t)) for t, x in enumerate(padded[j * k:(j + 1) * k]))
                  for j in range(len(packed))]
    cols = np.array(umbed(ms, 2 * k), dtype=np.float32)
    got = unpack_columns(cols, count, 2, k)
    want = np.array(umbed(xs, 2), dtype=np.float32)
    assert len(got) == 2
    for i in range(2):
        assert got[i].dtype == np.float32 and np.array_equal(got[i].view(np.uint32), want[i].view(np.uint32))
    # the values themselves, not only their float32 images
    exact = [_centred_digits(m, 2 * k, B) for m in ms]
    flat = [tuple(exact[j][t * 2:(t + 1) * 2]) for j in range(len(packed)) for t in range(k)][:count]
    assert flat == pairs


# ---------------------------------------------------------------- index mapping
@pytest.mark.parametrize("count,num,k", [(13, 2, 7), (14, 2, 7), (1, 2, 7), (8, 3, 4), (5, 1, 2)])
def test_unpack_columns_mapping(count, num, k):
    from xfl_amd.paillier_acceleration import unpack_columns
    ng = -(-count // k)
    cols = np.zeros((num * k, ng), dtype=np.float32)
    for j in range(ng):
        for t in range(k):
            for i in range(num):
                cols[t * num + i, j] = 1000 * i + j * k + t  # output i, element j k + t
    out = unpack_columns(list(cols), count, num, k)
    assert len(out) == num
    for i in range(num):
        assert out[i].shape == (count,) and out[i].tolist() == [1000 * i + e for e in range(count)]
    for bad_count in (ng * k + 1, (ng - 1) * k):
        with pytest.raises(ValueError):
            unpack_columns(list(cols), bad_count, num, k)
    with pytest.raises(ValueError):
        unpack_columns(list(cols[:-1]), count, num, k)


# ---------------------------------------------------------------- the planner
# literals, from the rule as paths.hpp states it: 16 lanes up to kPackRowMax
# groups, the batch shape beyond (in digits where powmod takes them: 2048
# bits, 4 lanes, a key with digit constants, $XHE_NDIG on); the pins override
_P2 = "pack K=2048 lanes=4 ndig=1"
ROWS = [
    (f"{_P2} ngroups=1", "ROW16/MONT"),
    (f"{_P2} ngroups=2341", "ROW16/MONT"),
    (f"{_P2} ngroups=1 XHE_N2_TPI=4", "LANES4/NDIG"),
    (f"{_P2} ngroups=65 XHE_N2_TPI=4", "LANES4/NDIG"),
    (f"{_P2} ngroups=65 XHE_N2_TPI=16", "ROW16/MONT"),
    (f"{_P2} ngroups=65 XHE_N2_TPI=4 XHE_NDIG=0", "LANES4/MONT"),
    (f"{_P2} ngroups=65 XHE_NDIG=0", "ROW16/MONT"),
    (f"{_P2} ngroups=1000000 XHE_N2_TPI=16", "ROW16/MONT"),
    (f"{_P2} ngroups=1000000", "LANES4/NDIG"),
    (f"{_P2} ngroups=1000000 XHE_NDIG=0", "LANES4/MONT"),
    (f"{_P2} ngroups=1000000 XHE_N2_TPI=8", "LANES4/NDIG"),  # not an accepted value: unset
    ("pack K=2048 lanes=4 ndig=0 ngroups=1000000", "LANES4/MONT"),
    ("pack K=3072 lanes=4 ndig=0 ngroups=1000000", "LANES4/MONT"),
    ("pack K=3072 lanes=4 ndig=1 ngroups=1000000", "LANES4/MONT"),
    ("pack K=4096 lanes=16 ndig=0 ngroups=3", "ROW16/MONT"),
    ("pack K=4096 lanes=16 ndig=0 ngroups=1000000", "LANES4/MONT"),  # the batch shape (16 lanes at this size)
    ("pack K=8192 lanes=16 ndig=0 ngroups=2 XHE_N2_TPI=4", "LANES4/MONT"),
]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("pack_paths")), "pack_paths_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    os.path.join(HERE, "native", "pack_paths_check.cpp"), "-o", exe], check=True)
    return exe


def _ask(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines), r.stdout
    return out


def test_planner_rows(check_exe):
    got = _ask(check_exe, [line for line, _ in ROWS])
    assert got == [want for _, want in ROWS], list(zip([line for line, _ in ROWS], got))


def test_planner_threshold_and_pins(check_exe):
    """the crossover sits at kPackRowMax exactly, and each pin changes a decision the default makes"""
    consts = dict(tok.split("=") for tok in _ask(check_exe, ["const"])[0].split())
    row_max = int(consts["kPackRowMax"])
    assert row_max >= 1
    at, past = f"{_P2} ngroups={row_max}", f"{_P2} ngroups={row_max + 1}"
    lines = [at, past, f"{at} XHE_N2_TPI=4", f"{past} XHE_N2_TPI=16", f"{past} XHE_NDIG=0"]
    a, p, a4, p16, pnd = _ask(check_exe, lines)
    assert (a, p) == ("ROW16/MONT", "LANES4/NDIG")
    assert a4 == "LANES4/NDIG" != a
    assert p16 == "ROW16/MONT" != p
    assert pnd == "LANES4/MONT" != p


def test_constant_documented():
    """kPackRowMax's comment carries the measurement it was set from"""
    src = open(os.path.join(ROOT, "xfl_amd", "csrc", "paths.hpp")).read()
    head = src[:src.index("constexpr int64_t kPackRowMax")]
    comment = head[head.rindex("// Ciphertext packing"):]
    for outputs in ("512", "2,341", "4,096", "16,384"):
        assert outputs in comment, outputs
    assert " ms" in comment


# ---------------------------------------------------------------- the drop-in's host logic
def test_pack_ciphertexts_host_logic(monkeypatch):
    """grouping, exponents, shape and the error cases of pack_ciphertexts, with
    the device call replaced by the Python-integer pack"""
    from tests import dropin_cases as C
    from xfl_amd import _native as nat
    from xfl_amd.paillier import PaillierArray, PaillierCiphertext, ops, resident
    from xfl_amd.paillier_acceleration import pack_ciphertexts
    _, pub = C.ctxs(load_fixture(PK.FIXTURE[2048]))
    n2 = pub.n * pub.n
    calls = []

    def pack_words(ctx, cw, k, shift_bits, num_cores=-1):
        calls.append((len(cw), k, shift_bits))
        return nat.ints_to_words(PK.pack_ref(nat.words_to_ints(cw), k, shift_bits, n2), cw.shape[1])
    monkeypatch.setattr(ops, "pack_words", pack_words)
    monkeypatch.setattr(resident, "device_for", lambda *a, **kw: None)
    cs = PK.inputs(2048, 9, 7, "host")
    objs = np.array([PaillierCiphertext(pub, c, 0) for c in cs], dtype=object)
    for arr in (objs, PaillierArray(objs)):
        got = pack_ciphertexts(arr)
        assert isinstance(got, PaillierArray) and got.shape == (2,) and not got.exponents.any()
        assert got.context is pub and not got.is_resident
        assert [c.raw_ciphertext for c in got] == PK.pack_ref(cs, 7, 256, n2)
    assert [c.raw_ciphertext for c in pack_ciphertexts(objs, k=2)] == PK.pack_ref(cs, 2, 256, n2)
    assert [c.raw_ciphertext for c in pack_ciphertexts(objs, num=1, k=3)] == PK.pack_ref(cs, 3, 128, n2)
    assert calls == [(9, 7, 256), (9, 7, 256), (9, 2, 256), (9, 3, 128)]
    assert pack_ciphertexts(PaillierArray(objs)[:0]).shape == (0,)
    for kw in (dict(k=8), dict(k=0), dict(k=True), dict(num=1, k=16), dict(interval=10 ** 38), dict(num=16)):
        with pytest.raises(ValueError):
            pack_ciphertexts(objs, **kw)
    with pytest.raises(ValueError, match="1-D"):
        pack_ciphertexts(PaillierArray(objs[:6]).reshape(2, 3))
    moved = np.array([PaillierCiphertext(pub, cs[0], 0), PaillierCiphertext(pub, cs[1], -3)], dtype=object)
    with pytest.raises(ValueError, match="exponent 0"):
        pack_ciphertexts(moved)
    holes = PaillierArray(objs).take([0, -1, 2], allow_fill=True)
    with pytest.raises(ValueError, match="missing"):
        pack_ciphertexts(holes)
    with pytest.raises(TypeError):
        pack_ciphertexts(np.arange(4))
    assert len(calls) == 4
