"""The kernel paths only a $XHE_* switch reaches, one case per switch setting
(tests/test_gpu_pinned_paths.py runs each in a child process on the GPU;
tests/test_pinned_paths_host.py checks on the CPU that no case is vacuous).

The switches (xfl_amd/csrc/paths.hpp parse_pins, INTEGRATION.md "Other kernel
switches") are read once per process, $XHE_NDIG_PUB when a key is created, so
a case is a fresh child: run_case(name) builds the case's key with win_bits =
8 tables, runs every (operation, count) of the case and prints one JSON line
each, {"case", "op", "count", "checked", "bad", "first_bad"}: `checked` rows
were compared word for word with Python integers, `bad` of them differ. The
parent asserts that the lines are the table's and that checked == count and
bad == 0 on each, so a child that does less than the table says fails.

Every row a kernel produces is compared. The expected values of an operation
come from at most DISTINCT[K] (input, expected) tuples, tiled to the count
with a rolling start so that neighbouring rows differ.

CASES, per case:
  name    the pytest id
  env     the switches of the child's environment (XHE_* path switches only)
  key     (fixture, mode): the golden fixture whose n, p, q, h make the key,
          and which of them the key is created from (priv_djn, priv_nodjn,
          pub_djn, pub_nodjn)
  ops     [(operation, counts)]; an operation is a name of OPS, with a
          parameter after ':' (powmod:53 = 53-bit exponents, powmod:full =
          exponents up to n - 1; multiexp:24 = 24 bases, its count the
          columns). segprod* counts are input elements: `checked` adds up the
          lengths of the segments compared. A name with `_wide` is the same
          operation on operands at and above n^2 (wide_operands below, from
          tests/wide_cases.py: include/xhe.h promises the result for the
          operand mod n^2), listed in every case that runs its narrow twin,
          at that case's counts.
  paths   [(line, decision)] or [(line, decision, default line)]: input lines
          of tests/native/paths_check.cpp without switches. With the case's
          env appended the planner must answer `decision`; the same line
          alone (or `default line`, where a flag or the lanes of the line are
          themselves what the switch changed: pub_nd under $XHE_NDIG_PUB, the
          lanes under $XHE_N2_TPI, which an `n2` line of the case then shows)
          must answer something else.
  labels  [(operation, count, launch label, launches)]: what xhe_profile_read
          counts for that run; an int is exact, ">0" at least one
  confirms_default  the pin names the path the default takes anyway (one case,
          below)

Block edges: the counts are 1, an odd one and one past a block of the shape in
play - k_add_barrett 32 elements a block (33), 4 lanes x 256 threads 64 (65),
16 lanes 16 (17), one lane x 128 threads 128 (129), one lane x 256 threads 256
(257), the 4-lane digit kernels of 128 threads 32 (33), block-per-element
kernels 1 and 15. Larger only where a threshold has to be passed: 2,049
($XHE_PUB_TPI=64 past kPubWaveMax), 4,200 ($XHE_N2_TPI=16 past kN2RowMax),
1,100 ($XHE_DEC_TPI=64 past kDecWaveMax) and 5,121 ($XHE_DEC_TPI=16 at
3072/4096 bits past kDecRowMax: up to there 16 lanes are the default, so only
that count makes the case differ from the default dispatch).

Not in the table:
  $XHE_ENC_TPI   every private DJN key is built with kd.pmd or kd.pmdx set
                 (xhe.hip build_private_tables), so paths::enc_djn never
                 returns POW_X, POW_LDS or POW through the ABI: the pin
                 reaches no kernel for any key the library builds.
  $XHE_PMD_SPLIT tests/test_gpu_pmd_log.py pins 1, 4 and 16 lanes at 1 .. 129
                 elements against the oracle (COVERED_ELSEWHERE).
  $XHE_DEC_TPI=16 at 8192 bits is in the table but cannot differ from the
                 default: the 8192-bit cases use the golden vectors tiled to at
                 most 5 elements, where 16 lanes are the default
                 (confirms_default; the host test allows exactly this case).
Beyond the switch settings INTEGRATION.md names, dec-tpi1-pmdx0-8192 runs
k_dec_pow<MP2, 0> in the 16-lane batch shape of 8192-bit keys, an
instantiation no default dispatch reaches either.
"""
import ctypes
import json
import math
import os
import random
import sys
import time

import numpy as np

from tests.conftest import ROOT, hx, load_fixture

WIN = 8  # fixed-base tables that build in milliseconds
DISTINCT = {2048: 32, 3072: 8, 4096: 8, 8192: 5}
FIXTURE = {"2048-djn": "paillier_2048_djn.json", "2048-nodjn": "paillier_2048_nodjn.json",
           "3072": "paillier_3072_djn.json", "4096": "paillier_4096_djn.json", "8192": "paillier_8192_djn.json"}
# switches that other modules test by pinning them in children of their own
COVERED_ELSEWHERE = {"XHE_PMD_SPLIT": "tests/test_gpu_pmd_log.py"}
NO_KERNEL = ("XHE_ENC_TPI",)  # see the docstring

_D2 = "decrypt K=2048 lanes=1 pmdx_dec=0 rns=1"
_D3 = "decrypt K=3072 lanes=2 pmdx_dec=1 rns=0"
_D4 = "decrypt K=4096 lanes=4 pmdx_dec=1 rns=0"
_D8 = "decrypt K=8192 lanes=16 pmdx_dec=1 rns=0"
_PUB2 = "enc_nodjn K=2048 priv=0 ndig=1"
_DEC2 = ("decrypt_golden", "decrypt_arb", "decrypt_arb_wide")
_DECX = ("decrypt_golden", "decrypt_arb_wide")  # 3072 bits and up
_N2OPS = ("add_eq", "add_gap", "powmod:53", "powmod:full", "powmod_inv:53", "powmod_inv:full", "segprod", "segprod_eq",
          "add_eq_wide", "add_gap_wide", "powmod_wide:53", "powmod_inv_wide:53", "segprod_wide", "segprod_eq_wide")
# narrow operation -> its twin on operands at and above n^2
WIDE_TWIN = {"add_eq": "add_eq_wide", "add_gap": "add_gap_wide", "powmod:53": "powmod_wide:53",
             "powmod_inv:53": "powmod_inv_wide:53", "invert": "invert_wide", "segprod": "segprod_wide",
             "segprod_eq": "segprod_eq_wide", "segprod_nod": "segprod_nod_wide", "multiexp:24": "multiexp_wide:24",
             "decrypt_arb": "decrypt_arb_wide"}


def _ops(names, counts):
    return [(op, counts) for op in names]


CASES = [
    # ------------------------------------------------------------- decrypt
    {"name": "dec-rns0-2048-djn", "env": {"XHE_DEC_RNS": "0"}, "key": ("2048-djn", "priv_djn"),
     "ops": _ops(_DEC2, (1, 15, 1024)),
     "paths": [(f"{_D2} count=1", "WAVE"), (f"{_D2} count=15", "WAVE"), (f"{_D2} count=1024", "WAVE")],
     "labels": [(op, c, lab, n) for op in _DEC2 for c in (1, 15, 1024)
                for lab, n in (("k_dec_wave", ">0"), ("k_dec_rns", 0))]},
    {"name": "dec-rns0-2048-nodjn", "env": {"XHE_DEC_RNS": "0"}, "key": ("2048-nodjn", "priv_nodjn"),
     "ops": _ops(_DEC2, (1, 15, 1024)),
     "paths": [(f"{_D2} count=1", "WAVE"), (f"{_D2} count=1024", "WAVE")],
     "labels": [(op, c, lab, n) for op in _DEC2 for c in (1, 15, 1024)
                for lab, n in (("k_dec_wave", ">0"), ("k_dec_rns", 0))]},
    {"name": "dec-tpi1-2048", "env": {"XHE_DEC_TPI": "1"}, "key": ("2048-djn", "priv_djn"),
     "ops": _ops(_DEC2, (1, 15, 129)),
     "paths": [(f"{_D2} count=1", "PMD1"), (f"{_D2} count=129", "PMD1")],
     "labels": [("decrypt_golden", 129, "k_dec_rns", 0), ("decrypt_golden", 129, "k_dec_pow", ">0")]},
    {"name": "dec-tpi4-2048", "env": {"XHE_DEC_TPI": "4"}, "key": ("2048-djn", "priv_djn"),
     "ops": _ops(_DEC2, (1, 15, 65)),
     "paths": [(f"{_D2} count=1", "QUAD4"), (f"{_D2} count=65", "QUAD4")],
     "labels": [("decrypt_golden", 65, "k_dec_rns", 0), ("decrypt_golden", 65, "k_dec_pow", ">0")]},
    {"name": "dec-tpi16-2048", "env": {"XHE_DEC_TPI": "16"}, "key": ("2048-djn", "priv_djn"),
     "ops": _ops(_DEC2, (1, 15, 17)),
     "paths": [(f"{_D2} count=1", "ROW16"), (f"{_D2} count=17", "ROW16")],
     "labels": [("decrypt_golden", 17, "k_dec_rns", 0), ("decrypt_golden", 17, "k_dec_pow", ">0")]},
    {"name": "dec-tpi64-2048", "env": {"XHE_DEC_TPI": "64"}, "key": ("2048-djn", "priv_djn"),
     "ops": _ops(_DEC2, (15, 1100)),
     "paths": [(f"{_D2} count=1100", "RNS")],
     "labels": [(op, 1100, lab, n) for op in _DEC2 for lab, n in (("k_dec_rns", ">0"), ("k_dec_pow", 0))]},
    {"name": "dec-tpi4-3072", "env": {"XHE_DEC_TPI": "4"}, "key": ("3072", "priv_djn"),
     "ops": _ops(_DECX, (1, 15, 65)),
     "paths": [(f"{_D3} count=1", "QUAD4"), (f"{_D3} count=65", "QUAD4")]},
    {"name": "dec-tpi4-4096", "env": {"XHE_DEC_TPI": "4"}, "key": ("4096", "priv_djn"),
     "ops": _ops(_DECX, (1, 15, 65)),
     "paths": [(f"{_D4} count=1", "QUAD4"), (f"{_D4} count=65", "QUAD4")]},
    {"name": "dec-tpi4-8192", "env": {"XHE_DEC_TPI": "4"}, "key": ("8192", "priv_djn"),
     "ops": _ops(_DECX, (1, 5)),
     "paths": [(f"{_D8} count=1", "QUAD4"), (f"{_D8} count=5", "QUAD4")]},
    {"name": "dec-tpi16-3072", "env": {"XHE_DEC_TPI": "16"}, "key": ("3072", "priv_djn"),
     "ops": _ops(_DECX, (1, 15, 17, 5121)),
     "paths": [(f"{_D3} count=5121", "ROW16")]},
    {"name": "dec-tpi16-4096", "env": {"XHE_DEC_TPI": "16"}, "key": ("4096", "priv_djn"),
     "ops": _ops(_DECX, (1, 15, 17, 5121)),
     "paths": [(f"{_D4} count=5121", "ROW16")]},
    {"name": "dec-tpi16-8192", "env": {"XHE_DEC_TPI": "16"}, "key": ("8192", "priv_djn"),
     "ops": _ops(_DECX, (1, 5)),
     "paths": [(f"{_D8} count=1", "ROW16"), (f"{_D8} count=5", "ROW16")], "confirms_default": True},
    {"name": "dec-tpi1-8192", "env": {"XHE_DEC_TPI": "1"}, "key": ("8192", "priv_djn"),
     "ops": _ops(_DECX, (1, 5)),
     "paths": [(f"{_D8} count=1", "PMDX"), (f"{_D8} count=5", "PMDX")]},
    {"name": "dec-tpi1-pmdx0-3072", "env": {"XHE_DEC_TPI": "1", "XHE_DEC_PMDX": "0"}, "key": ("3072", "priv_djn"),
     "ops": _ops(_DECX, (1, 15, 129)),
     "paths": [(f"{_D3} count=1", "POW1"), (f"{_D3} count=129", "POW1")]},
    {"name": "dec-tpi1-pmdx0-4096", "env": {"XHE_DEC_TPI": "1", "XHE_DEC_PMDX": "0"}, "key": ("4096", "priv_djn"),
     "ops": _ops(_DECX, (1, 15, 65)),
     "paths": [(f"{_D4} count=1", "POW1"), (f"{_D4} count=65", "POW1")]},
    {"name": "dec-tpi1-pmdx0-8192", "env": {"XHE_DEC_TPI": "1", "XHE_DEC_PMDX": "0"}, "key": ("8192", "priv_djn"),
     "ops": _ops(_DECX, (1, 5)),
     "paths": [(f"{_D8} count=1", "POW1"), (f"{_D8} count=5", "POW1")]},
    # ------------------------------------------------- encrypt, 2048 bits
    {"name": "enc-ndigpub0", "env": {"XHE_NDIG_PUB": "0"}, "key": ("2048-djn", "pub_djn"),
     "ops": [("encrypt", (1, 65))],
     "paths": [("pins", "ndig_pub=0"),
               ("enc_pub_djn K=2048 pub_nd=0", "PUB", "enc_pub_djn K=2048 pub_nd=1")],
     "labels": [("encrypt", 65, "k_djn_pub", 1)]},
    {"name": "enc-nodjnpmd0", "env": {"XHE_NODJN_PMD": "0"}, "key": ("2048-nodjn", "priv_nodjn"),
     "ops": [("encrypt", (1, 257)), ("enc_dec", (1, 257))],
     "paths": [("enc_nodjn K=2048 priv=1 ndig=1 count=1", "CRT"), ("enc_nodjn K=2048 priv=1 ndig=1 count=257", "CRT")],
     "labels": [("encrypt", 257, "k_nodjn_crt", 1)]},
    {"name": "enc-ndig0-lanes4", "env": {"XHE_NDIG": "0", "XHE_PUB_TPI": "4", "XHE_N2_TPI": "4"},
     "key": ("2048-nodjn", "pub_nodjn"),
     "ops": [("encrypt", (1, 65))] + _ops(("powmod:53", "powmod:full", "powmod_inv:53", "powmod_inv:full",
                                           "powmod_wide:53", "powmod_inv_wide:53"), (1, 65)),
     "paths": [(f"{_PUB2} count=1", "PUB"), (f"{_PUB2} count=65", "PUB"), ("n2 count=65", "LANES4"),
               ("powmod K=2048 lanes=4 ndig=1", "MONT")],
     "labels": [("encrypt", 65, "k_nodjn_pub", 1), ("encrypt", 65, "k_nodjn_pub_wave", 0),
                ("powmod:53", 65, "k_powmod_n2", 1)]},
    {"name": "enc-pubtpi4", "env": {"XHE_PUB_TPI": "4"}, "key": ("2048-nodjn", "pub_nodjn"),
     "ops": [("encrypt", (1, 15, 33))],
     "paths": [(f"{_PUB2} count=1", "NDIG"), (f"{_PUB2} count=33", "NDIG")],
     "labels": [("encrypt", c, lab, n) for c in (1, 15, 33)
                for lab, n in (("k_nodjn_pub_wave", 0), ("k_nodjn_pub", 1))]},
    {"name": "enc-pubtpi64", "env": {"XHE_PUB_TPI": "64"}, "key": ("2048-nodjn", "pub_nodjn"),
     "ops": [("encrypt", (2049,))],
     "paths": [(f"{_PUB2} count=2049", "PUB_WAVE")],
     "labels": [("encrypt", 2049, "k_nodjn_pub_wave", 1), ("encrypt", 2049, "k_nodjn_pub", 0)]},
    # ------------------------------------------------------ mod n^2 operations
    {"name": "n2-lanes4-2048", "env": {"XHE_N2_TPI": "4", "XHE_ADD_WAVE": "0"}, "key": ("2048-nodjn", "pub_nodjn"),
     "ops": _ops(_N2OPS, (1, 33, 65)) + _ops(("invert", "invert_wide"), (1, 2, 3, 65))
            + _ops(("multiexp:24", "multiexp_wide:24"), (5,)),
     "paths": [("n2 count=1", "LANES4"), ("n2 count=65", "LANES4"),
               ("add K=2048 lanes=4 count=33 dmax=0", "BARRETT"), ("add K=2048 lanes=4 count=33 dmax=3", "MONT"),
               ("powmod K=2048 lanes=4 ndig=1", "NDIG", "powmod K=2048 lanes=16 ndig=1"),
               ("invert K=2048 lanes=4 count=65", "TREE", "invert K=2048 lanes=16 count=65"),
               ("horner K=2048 lanes=4 ncols=5", "LANES", "horner K=2048 lanes=16 ncols=5")],
     "labels": [("add_eq", c, "k_add_barrett", 1) for c in (1, 33, 65)]
               + [("add_gap", c, "k_add_barrett", 0) for c in (1, 33, 65)]},
    # (a full-width power takes the 4-lane 3072-bit k_powmod_n2 1.2 s for one element and 2.7 s for 65: the
    # exponent's width does not depend on the block edge, which the 53-bit powers run at every count)
    {"name": "n2-lanes4-3072", "env": {"XHE_N2_TPI": "4", "XHE_ADD_WAVE": "0"}, "key": ("3072", "pub_nodjn"),
     "ops": _ops([op for op in _N2OPS if not op.endswith(":full")], (1, 33, 65))
            + [("powmod:full", (65,)), ("powmod_inv:full", (33,))] + _ops(("invert", "invert_wide"), (1, 2, 3, 65))
            + _ops(("multiexp:24", "multiexp_wide:24"), (5,)),
     "paths": [("n2 count=1", "LANES4"), ("n2 count=33", "LANES4"), ("n2 count=65", "LANES4")]},
    {"name": "n2-lanes4-addbar0", "env": {"XHE_N2_TPI": "4", "XHE_ADD_WAVE": "0", "XHE_ADD_BAR": "0"},
     "key": ("2048-nodjn", "pub_nodjn"),
     "ops": _ops(("add_eq", "add_eq_wide"), (1, 33, 65)),
     "paths": [("n2 count=65", "LANES4"), ("add K=2048 lanes=4 count=33 dmax=0", "MONT")],
     "labels": [("add_eq", c, "k_add_barrett", 0) for c in (1, 33, 65)]},
    {"name": "add-wave0", "env": {"XHE_ADD_WAVE": "0"}, "key": ("2048-nodjn", "pub_nodjn"),
     "ops": _ops(("add_eq", "add_gap", "add_eq_wide", "add_gap_wide"), (1, 17, 256)),
     "paths": [("add K=2048 lanes=16 count=1 dmax=0", "MONT"), ("add K=2048 lanes=16 count=17 dmax=3", "MONT"),
               ("add K=2048 lanes=16 count=256 dmax=0", "MONT")],
     "labels": [("add_eq", 17, "k_add_barrett", 0)]},
    {"name": "sum-words0", "env": {"XHE_SUM_WORDS": "0"}, "key": ("2048-nodjn", "pub_nodjn"),
     "ops": _ops(("segprod_eq", "segprod_nod", "segprod_eq_wide", "segprod_nod_wide"), (60,)),
     "paths": [("segprod count=60 dmax=0 has_d=1", "ALIGN"), ("segprod count=60 dmax=0 has_d=0", "ALIGN")]},
    {"name": "sum-words0-lanes4", "env": {"XHE_SUM_WORDS": "0", "XHE_N2_TPI": "4"}, "key": ("2048-nodjn", "pub_nodjn"),
     "ops": _ops(("segprod_eq", "segprod_nod", "segprod_eq_wide", "segprod_nod_wide"), (60, 65)),
     "paths": [("n2 count=60", "LANES4"), ("segprod count=60 dmax=0 has_d=1", "ALIGN"),
               ("segprod count=65 dmax=0 has_d=0", "ALIGN")]},
    {"name": "mexp-wave0", "env": {"XHE_MEXP_WAVE": "0"}, "key": ("2048-nodjn", "pub_nodjn"),
     "ops": [("multiexp:24", (5,)), ("multiexp:300", (3,)), ("multiexp_wide:24", (5,))],
     "paths": [("horner K=2048 lanes=16 ncols=5", "LANES"), ("horner K=2048 lanes=16 ncols=3", "LANES")],
     "labels": [("multiexp:24", 5, "k_mexp_horner", 1)]},
    {"name": "n2-row16-4200", "env": {"XHE_N2_TPI": "16"}, "key": ("2048-nodjn", "pub_nodjn"),
     "ops": _ops(("add_eq", "add_gap", "powmod:53", "powmod:full", "powmod_inv:53", "invert", "add_eq_wide",
                  "add_gap_wide", "powmod_wide:53", "powmod_inv_wide:53", "invert_wide"), (4200,)),
     "paths": [("n2 count=4200", "ROW16"),
               ("add K=2048 lanes=16 count=4200 dmax=0", "MONT", "add K=2048 lanes=4 count=4200 dmax=0"),
               ("powmod K=2048 lanes=16 ndig=1", "MONT", "powmod K=2048 lanes=4 ndig=1")],
     "labels": [("add_eq", 4200, "k_add_barrett", 0)]},
]

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def expected_lines(case):
    """the (op, count) pairs the child has to report"""
    return sorted((op, c) for op, counts in case["ops"] for c in counts)


def switches():
    """every XHE_* name a case sets"""
    return sorted({k for c in CASES for k in c["env"]})


# ------------------------------------------------------------------ the parent's side
_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import torch
torch.cuda.init()
from tests import pinned_cases
pinned_cases.run_case({name!r})
"""


def child_argv(name):
    return [sys.executable, "-c", _CHILD.format(root=ROOT, name=name)]


def parse_pins_names():
    """the switch names parse_pins of xfl_amd/csrc/paths.hpp looks up"""
    import re
    src = open(os.path.join(ROOT, "xfl_amd", "csrc", "paths.hpp")).read()
    body = src[src.index("Pins parse_pins("):]
    body = body[:body.index("return p;")]
    names = re.findall(r'"(XHE_[A-Z0-9_]+)"', body)
    assert len(names) == len(set(names)) >= 14, names
    return names


def child_env(case, environ=None):
    """the parent's environment without any XHE_* path switch, plus the case's"""
    drop = set(parse_pins_names())
    env = {k: v for k, v in (os.environ if environ is None else environ).items() if k not in drop}
    env.update(case["env"])
    return env


def parse_report(stdout):
    """the child's JSON lines"""
    out = []
    for line in stdout.splitlines():
        if line.startswith("{"):
            out.append(json.loads(line))
    return out


# ------------------------------------------------------------------- the child's side
def _tile(w, count, start=0):
    """count rows: the rows of w repeated, beginning at row `start`"""
    w = np.roll(w, -start, axis=0)
    return np.ascontiguousarray(np.tile(w, (-(-count // w.shape[0]), 1))[:count])


def wide_operands(K, n, d, what, units):
    """d operands of a key, 3 in 4 of them at or above n^2 (tests/wide_cases.py
    wide / units_wide), residues below n^2 between them. Row 1 is the largest
    one: _tile's rolling start makes it the operand of a batch of one."""
    from tests import wide_cases as W
    rng = random.Random(f"pinned-{K}-{what}-wide")
    ws = (W.units_wide if units else W.wide)(n, 2 * K // 32, d - d // 4, rng)
    low = [n * n - 1, 1, n + 1] + [rng.randrange(2, n * n) | 1 for _ in range(d)]
    low = [c for c in low if not units or math.gcd(c, n) == 1][:d // 4]
    out = low[:1] + W.mixed(ws, low[1:])
    assert len(set(out)) == len(out) == d
    return out


def _pad(edge, draw, d):
    """d values: the first edge, a random one, the other edges, random ones"""
    return (edge[:1] + [draw()] + edge[1:] + [draw() for _ in range(d)])[:d]


class Child:
    def __init__(self, case):
        from oracle import paillier_oracle as O
        from xfl_amd import _native as nat
        self.O, self.nat, self.case = O, nat, case
        for name, value in case["env"].items():
            assert os.environ.get(name) == value, f"{name} is not {value} in this process"
        fx, mode = case["key"]
        g = load_fixture(FIXTURE[fx])
        k = g["key"]
        self.g, self.K, self.mode = g, g["key_bits"], mode
        self.n, self.p, self.q = hx(k["n"]), hx(k["p"]), hx(k["q"])
        self.n2 = self.n * self.n
        self.h = hx(k["h_pow_n"]) if k["djn_on"] else None
        self.d = DISTINCT[self.K]
        n, p, q, h = self.n, self.p, self.q, self.h
        if mode == "priv_djn":
            self.dk = nat.DeviceKey(self.K, n, p, q, h, win_bits=WIN)
        elif mode == "priv_nodjn":
            self.dk = nat.DeviceKey(self.K, n, p, q, None)
        elif mode == "pub_djn":
            self.dk = nat.DeviceKey(self.K, n, None, None, h, win_bits=WIN)
        else:
            assert mode == "pub_nodjn", mode
            self.dk = nat.DeviceKey(self.K, n, None, None, None)
        assert self.dk.private == mode.startswith("priv") and self.dk.djn == mode.endswith("_djn")
        self._vec = {}

    # ---- plumbing
    def rng(self, what):
        return random.Random(f"pinned-{self.K}-{what}")

    def words(self, ints, nw):
        return self.nat.ints_to_words(ints, nw)

    def up(self, a):
        from xfl_amd.paillier import resident
        return resident.upload(np.ascontiguousarray(a), self.dk.device)

    def down(self, t):
        from xfl_amd.paillier import resident
        return resident.download(t)

    def vec(self, op, make):
        """the distinct tuples of an operation, computed once per child"""
        if op not in self._vec:
            self._vec[op] = make()
        return self._vec[op]

    def report(self, op, count, got, want, weight=None):
        """one JSON line: every row of got against want"""
        if got.shape != want.shape or got.dtype != want.dtype:
            checked, bad = 0, np.arange(max(len(got), len(want)))
        else:
            bad = np.nonzero(np.any(got != want, axis=1))[0]
            checked = len(want) if weight is None else int(weight)
        print(json.dumps({"case": self.case["name"], "op": op, "count": count, "checked": checked, "bad": int(bad.size),
                          "first_bad": bad[:6].tolist()}), flush=True)

    def launches(self, label):
        tot, cnt = ctypes.c_double(), ctypes.c_int64()
        self.nat.check(self.nat.lib().xhe_profile_read(label.encode(), ctypes.byref(tot), ctypes.byref(cnt)))
        return cnt.value

    def wide(self, what, units=True):
        return wide_operands(self.K, self.n, self.d, what, units)

    def units(self, count, rng):
        """count residues mod n^2 coprime to n: tests/test_gpu_add_barrett.py's edges that are, then random ones"""
        from tests.test_gpu_add_barrett import _edge
        out = []
        for c in [x % self.n2 for x in _edge(self.n2)] + [self.n + 1, (1 << (2 * self.K - 1)) % self.n2]:
            if c and math.gcd(c, self.n) == 1 and c not in out:
                out.append(c)
        while len(out) < count:
            c = rng.randrange(1, self.n2)
            if math.gcd(c, self.n) == 1:
                out.append(c)
        return out[:count]

    # ---- encrypt
    def _enc_vectors(self):
        n, n2, d = self.n, self.n2, self.d
        rng = self.rng("encrypt")
        rb, nb = n.bit_length() // 2, n.bit_length()
        ms = _pad([n - 1, n // 3, 0, 1, n - n // 3], lambda: rng.randrange(n), d)
        raw = [(1 + n * m) % n2 for m in ms]
        if self.mode.endswith("_djn"):
            assert self.dk.rand_bits == rb
            rs = _pad([(1 << rb) - 1, 1 << (rb - 1), 1, 2], lambda: rng.randrange(1, 1 << rb), d)
            if self.mode == "priv_djn":
                ok = self.O.derive_private(self.p, self.q, self.h)
                cts = [self.O.encrypt_m(ok, m, a) for m, a in zip(ms, rs)]
            else:
                cts = [c * pow(self.h, a, n2) % n2 for c, a in zip(raw, rs)]
        else:
            assert self.dk.rand_bits == nb
            rs = _pad([n - 1, 1 << (nb - 1), 1, 2, n - 2, (1 << (nb - 1)) - 1], lambda: rng.randrange(1, n), d)
            assert all(0 < r < n for r in rs)
            cts = [c * pow(r, n, n2) % n2 for c, r in zip(raw, rs)]
        dk = self.dk
        return self.words(ms, dk.nw), self.words(rs, dk.rand_words), self.words(cts, dk.n2w)

    def op_encrypt(self, op, count, arg):
        mw, rw, cw = self.vec("encrypt", self._enc_vectors)
        got = self.dk.encrypt_words(_tile(mw, count, count), _tile(rw, count, count))
        self.report(op, count, got, _tile(cw, count, count))

    def op_enc_dec(self, op, count, arg):
        """the pinned encryption decrypts (default dispatch) back to m"""
        mw, rw, _ = self.vec("encrypt", self._enc_vectors)
        ct = self.dk.encrypt_words(_tile(mw, count, count), _tile(rw, count, count))
        self.report(op, count, self.dk.decrypt_words(ct), _tile(mw, count, count))

    # ---- decrypt
    def _golden(self):
        """the fixture's golden ciphertexts and m, as tests/test_gpu_shapes.py _PIN_SCRIPT collects them"""
        g = self.g
        cts, want = [], []
        for name, enc in g["encrypt"].items():
            if not isinstance(enc, dict) or name not in g["decrypt"]:
                continue
            dec = g["decrypt"][name]
            cts += [hx(r) for r in enc["raw"]]
            want += [hx(m) for m in dec["m"][len(dec["m"]) - len(enc["raw"]):]]
        assert len(cts) == len(want) >= self.d
        pick = [i * len(cts) // self.d for i in range(self.d)]  # spread over the fixture's cases
        return self.words([cts[i] for i in pick], self.dk.n2w), self.words([want[i] for i in pick], self.dk.nw)

    def _arbitrary(self):
        assert self.K == 2048
        n, n2, p, q = self.n, self.n2, self.p, self.q
        rng = self.rng("arb")
        cs = [1, n2 - 1, p * p - 1, p * p + 1, q * q - 2, n + 1] + [rng.randrange(1, n2) for _ in range(10)]
        assert all(math.gcd(c, n) == 1 for c in cs)
        ok = self.O.derive_private(p, q, self.h)
        return self.words(cs, self.dk.n2w), self.words([self.O.decrypt_raw(ok, c) for c in cs], self.dk.nw)

    def op_decrypt_golden(self, op, count, arg):
        cw, mw = self.vec(op, self._golden)
        self.report(op, count, self.dk.decrypt_words(_tile(cw, count, count)), _tile(mw, count, count))

    def _arbitrary_wide(self):
        """any key size: units at and above n^2, the oracle on the unreduced value"""
        cs = self.wide("arb")
        ok = self.O.derive_private(self.p, self.q, self.h)
        ms = [self.O.decrypt_raw(ok, c) for c in cs]
        assert ms[1] == self.O.decrypt_raw(ok, cs[1] % self.n2) and cs[1] >= self.n2
        return self.words(cs, self.dk.n2w), self.words(ms, self.dk.nw)

    def op_decrypt_arb_wide(self, op, count, arg):
        cw, mw = self.vec(op, self._arbitrary_wide)
        self.report(op, count, self.dk.decrypt_words(_tile(cw, count, count)), _tile(mw, count, count))

    def op_decrypt_arb(self, op, count, arg):
        cw, mw = self.vec(op, self._arbitrary)
        self.report(op, count, self.dk.decrypt_words(_tile(cw, count, count)), _tile(mw, count, count))

    # ---- mod n^2
    def _add_vectors(self, gaps, wide=False):
        from tests.test_gpu_add_barrett import _edge
        n2, d = self.n2, self.d
        rng = self.rng(f"add-{gaps}")
        e = [x for x in _edge(n2) if x < 1 << (32 * self.dk.n2w)]  # (up to 2^4096 - 1: above n^2 at 2048 bits)
        pairs = [(n2 - 1, n2 - 1), (0, n2 - 1), (1, n2 - 2), (n2 // 2, n2 - 1)]
        pairs += [(e[i], e[(5 * i + 3) % len(e)]) for i in range(len(e))]
        pairs += [(rng.randrange(n2), rng.randrange(n2)) for _ in range(d)]
        pairs = pairs[:d - 2] + [(rng.randrange(n2), rng.randrange(n2)) for _ in range(2)]
        if wide:  # both sides, the left one, the right one at or above n^2
            x, y = self.wide(f"add-{gaps}-a", units=False), self.wide(f"add-{gaps}-b", units=False)
            pairs = [(x[i] if i % 3 != 2 else pairs[i][0], y[(5 * i + 3) % d] if i % 3 != 1 else pairs[i][1])
                     for i in range(d)]
        a, b = [x for x, _ in pairs], [y for _, y in pairs]
        if gaps:
            ea = ([0, -3, 0, -1, -2, -3, -1, 0] + [rng.randrange(-3, 1) for _ in range(d)])[:d]
            eb = ([-3, 0, 0, -3, -2, 0, -2, -1] + [rng.randrange(-3, 1) for _ in range(d)])[:d]
        else:
            ea = eb = [i % 5 - 40 for i in range(d)]
        want = []
        for x, y, s, t in zip(a, b, ea, eb):
            lo = min(s, t)
            want.append(pow(x, 1 << (s - lo), n2) * pow(y, 1 << (t - lo), n2) % n2)
        i32 = lambda v: np.asarray(v, dtype=np.int32).reshape(-1, 1)  # noqa: E731
        w = self.dk.n2w
        return self.words(a, w), self.words(b, w), i32(ea), i32(eb), self.words(want, w)

    def _add(self, op, count, gaps, wide=False):
        from xfl_amd.paillier import resident
        aw, bw, ea, eb, want = self.vec(op, lambda: self._add_vectors(gaps, wide))
        t = lambda v: _tile(v, count, count)  # noqa: E731
        out = resident.mulmod(self.dk, self.up(t(aw)), t(ea).reshape(-1), self.up(t(bw)), t(eb).reshape(-1),
                              3 if gaps else 0)
        self.report(op, count, self.down(out), t(want))

    def op_add_eq(self, op, count, arg):
        self._add(op, count, False)

    def op_add_gap(self, op, count, arg):
        self._add(op, count, True)

    def op_add_eq_wide(self, op, count, arg):
        self._add(op, count, False, True)

    def op_add_gap_wide(self, op, count, arg):
        self._add(op, count, True, True)

    def _pow_vectors(self, width, inverted, wide=False):
        cs, ks, kbits, want = self.vec(f"pow-{width}-{wide}", lambda: self._pow_ints(width, wide))
        if inverted:
            want = [pow(x, -1, self.n2) for x in want]  # (c^-1)^k
        w = self.dk.n2w
        return self.words(cs, w), self.words(ks, (kbits + 31) // 32), kbits, self.words(want, w)

    def _pow_ints(self, width, wide=False):
        n, n2, d = self.n, self.n2, self.d
        rng = self.rng(f"powmod-{width}")
        cs = self.wide("powmod") if wide else self.units(d, rng)
        if width == "full":  # tests/test_gpu_ndig.py's exponent edges; k = n - 1 is the full-width one
            kbits = n.bit_length()
            ks = _pad([n - 1, 0, 1, (1 << 53) - 1, 15, 16], lambda: rng.randrange(n), d)
        else:
            kbits = int(width)
            top = (1 << kbits) - 1
            ks = _pad([top, 0, 1, 15, 16, 1 << (kbits - 1)], lambda: rng.getrandbits(kbits), d)
        return cs, ks, kbits, [pow(c, k, n2) for c, k in zip(cs, ks)]

    def _powmod(self, op, count, width, inverted, wide=False):
        from xfl_amd.paillier import resident
        cw, kw, kbits, want = self.vec(op, lambda: self._pow_vectors(width, inverted, wide))
        out = resident.powmod(self.dk, self.up(_tile(cw, count, count)), _tile(kw, count, count), kbits,
                              invert_first=inverted)
        self.report(op, count, self.down(out), _tile(want, count, count))

    def op_powmod(self, op, count, arg):
        self._powmod(op, count, arg, False)

    def op_powmod_inv(self, op, count, arg):
        self._powmod(op, count, arg, True)

    def op_powmod_wide(self, op, count, arg):
        self._powmod(op, count, arg, False, True)

    def op_powmod_inv_wide(self, op, count, arg):
        self._powmod(op, count, arg, True, True)

    def op_invert(self, op, count, arg, wide=False):
        from xfl_amd.paillier import resident

        def make():
            cs = self.wide("invert") if wide else self.units(self.d, self.rng("invert"))
            return self.words(cs, self.dk.n2w), self.words([pow(c, -1, self.n2) for c in cs], self.dk.n2w)
        cw, want = self.vec(op, make)
        out = resident.invert(self.dk, self.up(_tile(cw, count, count)))
        self.report(op, count, self.down(out), _tile(want, count, count))

    def op_invert_wide(self, op, count, arg):
        self.op_invert(op, count, arg, True)

    def _segprod(self, op, count, d, dmax, has_d):
        """out[s] = prod c_i^(2^d_i) over an empty segment, one of length 1 and
        what the count leaves for up to two more; xhe_segprod called as
        xfl_amd.paillier.resident.segprod calls it, but with the exponent
        array kept (has_d) when it is all zero"""
        import torch

        from xfl_amd.paillier import resident
        nat, dk, n2 = self.nat, self.dk, self.n2
        if op.partition(":")[0].endswith("_wide"):
            cs = self.vec("segprod-wide", lambda: self.wide("segprod", units=False))
        else:
            cs = self.vec("segprod-units", lambda: self.units(self.d, self.rng("segprod")))
        cs = [cs[(count + i) % len(cs)] for i in range(count)]
        seg = np.asarray([0, 0] + sorted({1, 1 + (count - 1) // 3, count}), dtype=np.int64)
        assert seg[-1] == count and (seg[2] - seg[1]) == 1
        want = []
        for s in range(len(seg) - 1):
            acc = 1
            for i in range(int(seg[s]), int(seg[s + 1])):
                acc = acc * pow(cs[i], 1 << int(d[i]), n2) % n2
            want.append(acc)
        assert want[0] == 1
        dev = dk.device
        c = self.up(self.words(cs, dk.n2w))
        dd = self.up(np.asarray(d, dtype=np.int32)) if has_d else None
        with resident._On(dev):
            out = torch.empty((len(seg) - 1, dk.n2w), dtype=torch.int32, device=f"cuda:{dev}")
        nat.check(nat.lib().xhe_segprod(dk.handle, resident._dp(c), resident._dp(dd), dmax, count,
                                        seg.ctypes.data_as(ctypes.c_void_p), len(seg) - 1, resident._dp(out),
                                        resident._sp(dev)), "segprod")
        self.report(op, count, self.down(out), self.words(want, dk.n2w), weight=int(seg[-1]))

    def op_segprod(self, op, count, arg):  # gaps 0 .. 3: the alignment squarings
        d = [(7 * i + count) % 4 for i in range(count)]
        self._segprod(op, count, d, max(d), True)

    def op_segprod_eq(self, op, count, arg):  # all-equal exponents, the array given
        self._segprod(op, count, [0] * count, 0, True)

    def op_segprod_nod(self, op, count, arg):  # no exponent array
        self._segprod(op, count, [0] * count, 0, False)

    op_segprod_wide, op_segprod_eq_wide, op_segprod_nod_wide = op_segprod, op_segprod_eq, op_segprod_nod

    def op_multiexp_wide(self, op, ncols, arg):
        self.op_multiexp(op, ncols, arg, True)

    def op_multiexp(self, op, ncols, arg, wide=False):
        from xfl_amd.paillier import resident
        nbases, n2, KB = int(arg), self.n2, 60
        rng = self.rng(op)
        if wide:
            distinct = self.vec("multiexp-wide", lambda: self.wide("multiexp", units=False))
        else:
            distinct = self.vec("multiexp-units", lambda: self.units(self.d, self.rng("multiexp")))
        bases = [distinct[(i + nbases) % len(distinct)] for i in range(nbases)]
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
        out = resident.multiexp(self.dk, self.up(self.words(bases, self.dk.n2w)), idx,
                                self.words([e for row in ex for e in row], 2), KB)
        self.report(op, ncols, self.down(out), self.words(want, self.dk.n2w))

    # ---- one case
    def run(self):
        L = self.nat.lib()
        labels = {}
        for op, count, label, n in self.case.get("labels", ()):
            labels.setdefault((op, count), []).append((label, n))
        for op, counts in self.case["ops"]:
            name, _, arg = op.partition(":")
            fn = getattr(self, "op_" + name)
            for count in counts:
                want = labels.get((op, count))
                if want:
                    L.xhe_profile(1)  # (resets the records)
                t0 = time.perf_counter()
                try:
                    fn(op, count, arg)
                    print(f"{op} x {count}: {time.perf_counter() - t0:.2f} s", file=sys.stderr)  # reference + kernels
                    for label, n in want or ():
                        ran = self.launches(label)
                        assert ran > 0 if n == ">0" else ran == n, f"{op} x {count}: {label} ran {ran} times, not {n}"
                finally:
                    if want:
                        L.xhe_profile(0)


OPS = sorted(name[3:] for name in vars(Child) if name.startswith("op_"))


def run_case(name):
    Child(BY_NAME[name]).run()
