"""Ciphertext operands at and above n^2, shared by tests/test_wide_cases.py,
tests/test_gpu_wide_operands.py, tests/pinned_cases.py and the drop-in test of
tests/test_gpu_resident.py.

A received payload may hold any value below 2^(32 n2w) (the wire codec rejects
only wider ones), and Python's integers are total there: pow(c, k, n^2),
a * b % n^2, pow(c, -1, n^2) and the decryption all answer for c mod n^2. How
far a value can exceed n^2 depends on the key: q_max(n, n2w) = (2^(32 n2w) - 1)
// n^2 is 1 to 4 for an n of full width, 8 or so for an n one bit short and 63
for the modulus 2^2045 + 1, so an entry that reduces with one conditional
subtraction is right for the first kind of key and wrong for the last.

A plain module (no fixtures). The lists are ordered by what they must not
lose when d is small: wide(n, n2w, 5, rng) still holds 2^(32 n2w) - 1,
q_max n^2 and n^2.
"""
import math


GOLDEN = {"golden-2048-djn": "paillier_2048_djn.json", "golden-2048-nodjn": "paillier_2048_nodjn.json",
          "golden-3072": "paillier_3072_djn.json", "golden-4096": "paillier_4096_djn.json",
          "golden-8192": "paillier_8192_djn.json"}
STRUCTURED = [(K, name) for K in (2048, 3072, 4096) for name in ("top", "bottom")]
PUB_MODULI = {"all_ones_2048": 2 ** 2048 - 159, "sparse_2046": 2 ** 2045 + 1}  # tests/test_gpu_key_structure.py's
# distinct operands per key (the Python reference is computed once for them and tiled)
DISTINCT = {2048: 32, 3072: 16, 4096: 16, 8192: 8}

_keys = {}


def key(name):
    """(K, n, p, q, h) of a key of key_names(); p, q, h are None for the public moduli"""
    if name not in _keys:
        from tests import structured_keys as SK
        from tests.conftest import hx, load_fixture
        if name in GOLDEN:
            g = load_fixture(GOLDEN[name])
            k = g["key"]
            _keys[name] = (g["key_bits"], hx(k["n"]), hx(k["p"]), hx(k["q"]),
                           hx(k["h_pow_n"]) if k["djn_on"] else None)
        elif name in PUB_MODULI:
            _keys[name] = (2048, PUB_MODULI[name], None, None, None)
        else:
            K, which = name.split("-")
            k = SK.key(int(K), which)
            _keys[name] = (k.K, k.n, k.p, k.q, k.h)
    return _keys[name]


def key_names(private_only=False):
    names = list(GOLDEN) + [f"{K}-{which}" for K, which in STRUCTURED]
    return names if private_only else names + list(PUB_MODULI)


def q_max(n, n2w):
    return ((1 << (32 * n2w)) - 1) // (n * n)


def _fixed(n, n2w):
    """the edge values, most telling first; those that fit n2w words, once each"""
    n2, top = n * n, 1 << (32 * n2w)
    qm = q_max(n, n2w)
    assert qm >= 1, "n^2 does not fit n2w words"
    e = [top - 1, qm * n2, n2]
    # metamorphic twins: u + j n^2 has the expected value of u
    e += [u + j * n2 for j in (qm, 1) for u in (n + 1, n2 - 1, 1)]
    e += [n2 + 1, qm * n2 - 1, qm * n2 + 1, 2 * n2 - 1, top - 2, top >> 1]
    # all ones below a limb boundary of the two radices in use
    for radix in (28, 27):
        e += [(1 << (radix * k)) - 1 for k in range(n2.bit_length() // radix, 32 * n2w // radix + 1)]
    out = []
    for x in e:
        if 0 <= x < top and (x >= n2 or x == top >> 1) and x not in out:
            out.append(x)
    return out


def _fill(fixed, keep, n, n2w, d, rng):
    """d distinct values: the fixed ones, the last quarter (two at least)
    random draws from [n^2, 2^(32 n2w))"""
    n2, top = n * n, 1 << (32 * n2w)
    fixed = [x for x in fixed if keep(x)]
    out = fixed[:max(0, d - max(2, d // 4))]
    while len(out) < d:
        x = rng.randrange(n2, top)
        if keep(x) and x not in out:
            out.append(x)
    assert len(set(out)) == d and all(0 <= x < top for x in out)
    assert 4 * sum(x >= n2 for x in out) >= 3 * d
    return out


def wide(n, n2w, d, rng):
    """d distinct integers below 2^(32 n2w), at least 3/4 of them >= n^2"""
    return _fill(_fixed(n, n2w), lambda x: True, n, n2w, d, rng)


def units_wide(n, n2w, d, rng):
    """wide() restricted to gcd(c mod n^2, n) = 1 (invert, powmod_inv, decrypt)"""
    n2 = n * n
    return _fill(_fixed(n, n2w), lambda x: math.gcd(x % n2, n) == 1, n, n2w, d, rng)


def non_units(n, p, q, n2w, d, rng):
    """d distinct values whose residue mod n^2 shares a factor with n: 0, n, p,
    q, p^2, n^2 - n and their twins u + j n^2 for j in (q_max, 1), then random
    multiples of p and of q with a random j"""
    n2, top = n * n, 1 << (32 * n2w)
    qm = q_max(n, n2w)
    base = [0, n, p, q, p * p, n2 - n]
    out = []
    for x in [u + j * n2 for u in base for j in (0, qm, 1)]:
        if x < top and x not in out:
            out.append(x)
    out = out[:d]
    while len(out) < d:
        f = (p, q)[len(out) % 2]
        j = rng.randrange(1, qm + 1)
        x = f * rng.randrange(1, min(n2, top - j * n2) // f) + j * n2
        if x < top and x not in out:
            out.append(x)
    assert all(math.gcd(x % n2, n) != 1 for x in out)
    return out


def mixed(wide_values, narrow_values):
    """the two lists interleaved, wide first, so that neighbouring lane groups
    of one wave take both sides of any entry branch"""
    out = []
    for i in range(max(len(wide_values), len(narrow_values))):
        out += wide_values[i:i + 1] + narrow_values[i:i + 1]
    return out


def truncated(x, n):
    """the naive reading of a wide operand: its words above n^2's own ignored"""
    return x & ((1 << (n * n).bit_length()) - 1)
