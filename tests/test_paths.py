"""CPU: the kernel path chosen for every call shape, threshold and switch.

xfl_amd/csrc/paths.hpp decides which kernel serves a call: pure functions of
the key bits, the lanes of the limb shape, the key's table flags, the element
count and the $XHE_* switches. tests/native/paths_check.cpp (its own main,
plain g++, started as a separate process) prints the decision for each input
line. The expected answers below are literals, written from the rules as
INTEGRATION.md and the comments of paths.hpp state them - not computed by a
second copy of the logic: a threshold or a rule that moves has to be moved
here too, by hand.

Lanes per key size, as xhe.hip's shapes have them: the batch p^2 shape MP2
has 1 / 2 / 4 / 16 lanes at 2048 / 3072 / 4096 / 8192 bits; the batch n^2
shape MN2 4 / 4 / 16 / 16, the small-batch n^2 shape MN2X 16 everywhere.
"""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CONSTANTS = ("kEncRowMax=20480 kPmdSplit16Max=2048 kPmdSplit4Max=16384 kPubWaveMax=2048 kN2RowMax=4096 "
             "kWaveAddMax=256 kWtreeMax=256 kMexpWaveMax=4096 kDecWaveMax=1024 kDecRowMax=5120 kDecQuadMax=28672")

UNSET = ("enc_tpi=-1 pmd_split=0 pub_tpi=0 n2_tpi=0 dec_tpi=0 ndig_pub=1 ndig=1 nodjn_pmd=1 add_wave=1 add_bar=1 "
         "sum_words=1 mexp_wave=1 dec_pmdx=1 dec_rns=1")


def _pins(**changed):
    """UNSET with the named fields replaced (a formatting helper: no rule in it)"""
    out = UNSET
    for k, v in changed.items():
        out, n = re.subn(rf"\b{k}=-?\d+", f"{k}={v}", out)
        assert n == 1, k
    return out


ROWS = {}

ROWS["const"] = [("const", CONSTANTS)]

# switch parsing: on/off switches are off only when the value starts with '0'
# (the empty string is on); integers through atoll, values outside a pin's set dropped
ROWS["pins"] = [
    ("pins", UNSET),
    ("pins XHE_NDIG=0", _pins(ndig=0)),
    ("pins XHE_NDIG=00", _pins(ndig=0)),
    ("pins XHE_NDIG=01", _pins(ndig=0)),
    ("pins XHE_NDIG=", UNSET),
    ("pins XHE_NDIG=1", UNSET),
    ("pins XHE_NDIG=off", UNSET),
    ("pins XHE_NDIG_PUB=0", _pins(ndig_pub=0)),
    ("pins XHE_NODJN_PMD=0", _pins(nodjn_pmd=0)),
    ("pins XHE_ADD_WAVE=0", _pins(add_wave=0)),
    ("pins XHE_ADD_BAR=0", _pins(add_bar=0)),
    ("pins XHE_SUM_WORDS=0", _pins(sum_words=0)),
    ("pins XHE_MEXP_WAVE=0", _pins(mexp_wave=0)),
    ("pins XHE_DEC_PMDX=0", _pins(dec_pmdx=0)),
    ("pins XHE_DEC_RNS=0", _pins(dec_rns=0)),
    ("pins XHE_DEC_TPI=1", _pins(dec_tpi=1)),
    ("pins XHE_DEC_TPI=4", _pins(dec_tpi=4)),
    ("pins XHE_DEC_TPI=16", _pins(dec_tpi=16)),
    ("pins XHE_DEC_TPI=64", _pins(dec_tpi=64)),
    ("pins XHE_DEC_TPI=8", UNSET),
    ("pins XHE_PMD_SPLIT=1", _pins(pmd_split=1)),
    ("pins XHE_PMD_SPLIT=4", _pins(pmd_split=4)),
    ("pins XHE_PMD_SPLIT=16", _pins(pmd_split=16)),
    ("pins XHE_PMD_SPLIT=2", UNSET),
    ("pins XHE_PUB_TPI=4", _pins(pub_tpi=4)),
    ("pins XHE_PUB_TPI=64", _pins(pub_tpi=64)),
    ("pins XHE_PUB_TPI=16", UNSET),
    ("pins XHE_N2_TPI=4", _pins(n2_tpi=4)),
    ("pins XHE_N2_TPI=16", _pins(n2_tpi=16)),
    ("pins XHE_N2_TPI=8", UNSET),
    # $XHE_ENC_TPI: every value >= 0 is kept (16 = the row shape, anything else = not the row shape)
    ("pins XHE_ENC_TPI=16", _pins(enc_tpi=16)),
    ("pins XHE_ENC_TPI=0", _pins(enc_tpi=0)),
    ("pins XHE_ENC_TPI=4", _pins(enc_tpi=4)),
    ("pins XHE_ENC_TPI=", _pins(enc_tpi=0)),  # atoll("") = 0: set but empty pins "not the row shape"
    ("pins XHE_ENC_TPI=-1", UNSET),
    ("pins XHE_DEC_TPI=16 XHE_NDIG=0 XHE_DEC_RNS=0", _pins(dec_tpi=16, ndig=0, dec_rns=0)),
]

# private DJN encryption, per launch chunk of n elements
_D2 = "enc_djn K=2048 lanes=1 pmd=1 pmdx=0"
_P2 = "enc_djn K=2048 lanes=1 pmd=0 pmdx=0"
ROWS["enc_djn"] = [
    # k_djn_pmd's lanes per element: 16 up to 2048, 4 up to 16384, else 1
    (f"{_D2} n=1", "PMD/16"),
    (f"{_D2} n=2048", "PMD/16"),
    (f"{_D2} n=2049", "PMD/4"),
    (f"{_D2} n=16384", "PMD/4"),
    (f"{_D2} n=16385", "PMD/1"),
    (f"{_D2} n=1 XHE_PMD_SPLIT=1", "PMD/1"),
    (f"{_D2} n=1 XHE_PMD_SPLIT=4", "PMD/4"),
    (f"{_D2} n=16385 XHE_PMD_SPLIT=16", "PMD/16"),
    (f"{_D2} n=1 XHE_PMD_SPLIT=2", "PMD/16"),
    (f"{_D2} n=16385 XHE_PMD_SPLIT=2", "PMD/1"),
    (f"{_D2} n=1 XHE_ENC_TPI=0", "PMD/16"),  # the row-shape pin does not reach the digit kernels
    ("enc_djn K=3072 lanes=2 pmd=0 pmdx=1 n=1", "PMDX"),
    ("enc_djn K=3072 lanes=2 pmd=0 pmdx=1 n=20481", "PMDX"),
    ("enc_djn K=4096 lanes=4 pmd=0 pmdx=1 n=1", "PMDX"),
    ("enc_djn K=8192 lanes=16 pmd=0 pmdx=1 n=1", "PMDX"),
    ("enc_djn K=3072 lanes=2 pmd=0 pmdx=1 n=1 XHE_ENC_TPI=0", "PMDX"),
    # each key size reads its own flag only
    ("enc_djn K=2048 lanes=1 pmd=0 pmdx=1 n=1", "POW_X"),
    ("enc_djn K=3072 lanes=2 pmd=1 pmdx=0 n=1", "POW_X"),
    # keys without digit tables: the row shape up to 20480, then the batch shape (LDS staging in one lane)
    (f"{_P2} n=1", "POW_X"),
    (f"{_P2} n=20480", "POW_X"),
    (f"{_P2} n=20481", "POW_LDS"),
    ("enc_djn K=3072 lanes=2 pmd=0 pmdx=0 n=1", "POW_X"),
    ("enc_djn K=3072 lanes=2 pmd=0 pmdx=0 n=20480", "POW_X"),
    ("enc_djn K=3072 lanes=2 pmd=0 pmdx=0 n=20481", "POW"),
    ("enc_djn K=4096 lanes=4 pmd=0 pmdx=0 n=1", "POW_X"),
    ("enc_djn K=4096 lanes=4 pmd=0 pmdx=0 n=20480", "POW_X"),
    ("enc_djn K=4096 lanes=4 pmd=0 pmdx=0 n=20481", "POW"),
    ("enc_djn K=8192 lanes=16 pmd=0 pmdx=0 n=1", "POW_X"),
    ("enc_djn K=8192 lanes=16 pmd=0 pmdx=0 n=20480", "POW_X"),
    ("enc_djn K=8192 lanes=16 pmd=0 pmdx=0 n=20481", "POW"),
    (f"{_P2} n=20481 XHE_ENC_TPI=16", "POW_X"),
    (f"{_P2} n=1 XHE_ENC_TPI=0", "POW_LDS"),
    (f"{_P2} n=1 XHE_ENC_TPI=4", "POW_LDS"),
    (f"{_P2} n=1 XHE_ENC_TPI=-1", "POW_X"),
    (f"{_P2} n=20481 XHE_ENC_TPI=-1", "POW_LDS"),
    ("enc_djn K=3072 lanes=2 pmd=0 pmdx=0 n=1 XHE_ENC_TPI=0", "POW"),
    ("enc_djn K=3072 lanes=2 pmd=0 pmdx=0 n=1 XHE_ENC_TPI=4", "POW"),
    ("enc_djn K=4096 lanes=4 pmd=0 pmdx=0 n=20481 XHE_ENC_TPI=16", "POW_X"),
]

# public DJN encryption ($XHE_NDIG_PUB acts at key creation: a key made with it off has no pub_nd)
ROWS["enc_pub_djn"] = [
    ("enc_pub_djn K=2048 pub_nd=1", "PUB_ND"),
    ("enc_pub_djn K=2048 pub_nd=0", "PUB"),
    ("enc_pub_djn K=3072 pub_nd=0", "PUB"),
    ("enc_pub_djn K=3072 pub_nd=1", "PUB"),
    ("enc_pub_djn K=4096 pub_nd=0", "PUB"),
    ("enc_pub_djn K=8192 pub_nd=0", "PUB"),
]

# non-DJN encryption, by the whole call's count
_N2 = "enc_nodjn K=2048 priv=0 ndig=1"
ROWS["enc_nodjn"] = [
    ("enc_nodjn K=2048 priv=1 ndig=1 count=1", "PMD"),
    ("enc_nodjn K=2048 priv=1 ndig=1 count=2048", "PMD"),
    ("enc_nodjn K=2048 priv=1 ndig=1 count=2049", "PMD"),
    ("enc_nodjn K=2048 priv=1 ndig=1 count=1 XHE_NODJN_PMD=0", "CRT"),
    ("enc_nodjn K=2048 priv=1 ndig=1 count=1 XHE_PUB_TPI=64", "PMD"),
    ("enc_nodjn K=2048 priv=1 ndig=1 count=1 XHE_NODJN_PMD=0 XHE_PUB_TPI=64", "CRT"),
    ("enc_nodjn K=3072 priv=1 ndig=0 count=1", "CRT"),
    ("enc_nodjn K=4096 priv=1 ndig=0 count=1", "CRT"),
    ("enc_nodjn K=8192 priv=1 ndig=0 count=1", "CRT"),
    # public 2048-bit keys: one block per element up to 2048, the digit kernels beyond
    (f"{_N2} count=1", "PUB_WAVE"),
    (f"{_N2} count=2048", "PUB_WAVE"),
    (f"{_N2} count=2049", "NDIG"),
    (f"{_N2} count=2049 XHE_PUB_TPI=64", "PUB_WAVE"),
    (f"{_N2} count=1 XHE_PUB_TPI=4", "NDIG"),
    (f"{_N2} count=1 XHE_PUB_TPI=16", "PUB_WAVE"),
    (f"{_N2} count=2049 XHE_PUB_TPI=16", "NDIG"),
    (f"{_N2} count=2049 XHE_NDIG=0", "PUB"),
    (f"{_N2} count=1 XHE_NDIG=0", "PUB_WAVE"),
    (f"{_N2} count=1 XHE_NODJN_PMD=0", "PUB_WAVE"),
    ("enc_nodjn K=2048 priv=0 ndig=0 count=2049", "PUB"),
    ("enc_nodjn K=2048 priv=0 ndig=0 count=1 XHE_PUB_TPI=4", "PUB"),
    # the larger keys have neither
    ("enc_nodjn K=3072 priv=0 ndig=0 count=1", "PUB"),
    ("enc_nodjn K=3072 priv=0 ndig=0 count=2048", "PUB"),
    ("enc_nodjn K=3072 priv=0 ndig=0 count=2049", "PUB"),
    ("enc_nodjn K=3072 priv=0 ndig=1 count=2049", "PUB"),
    ("enc_nodjn K=3072 priv=0 ndig=0 count=1 XHE_PUB_TPI=64", "PUB"),
    ("enc_nodjn K=4096 priv=0 ndig=0 count=1", "PUB"),
    ("enc_nodjn K=4096 priv=0 ndig=0 count=2049", "PUB"),
    ("enc_nodjn K=8192 priv=0 ndig=0 count=1", "PUB"),
    ("enc_nodjn K=8192 priv=0 ndig=0 count=2049", "PUB"),
]

# lane shape of the n^2 ops (the same for every key size)
ROWS["n2"] = [
    ("n2 count=1", "ROW16"),
    ("n2 count=4096", "ROW16"),
    ("n2 count=4097", "LANES4"),
    ("n2 count=4097 XHE_N2_TPI=16", "ROW16"),
    ("n2 count=1 XHE_N2_TPI=4", "LANES4"),
    ("n2 count=1 XHE_N2_TPI=8", "ROW16"),
    ("n2 count=4097 XHE_N2_TPI=8", "LANES4"),
]

ROWS["add"] = [
    ("add K=2048 lanes=16 count=1 dmax=0", "WAVE"),
    ("add K=2048 lanes=16 count=256 dmax=0", "WAVE"),
    ("add K=2048 lanes=16 count=256 dmax=3", "WAVE"),
    ("add K=2048 lanes=16 count=257 dmax=0", "MONT"),  # 16 lanes: no Barrett kernel
    ("add K=2048 lanes=16 count=257 dmax=3", "MONT"),
    ("add K=2048 lanes=4 count=256 dmax=0", "WAVE"),  # ($XHE_N2_TPI=4) the block kernel is asked first
    ("add K=2048 lanes=4 count=257 dmax=0", "BARRETT"),
    ("add K=2048 lanes=4 count=4097 dmax=0", "BARRETT"),
    ("add K=2048 lanes=4 count=4097 dmax=1", "MONT"),
    ("add K=2048 lanes=16 count=1 dmax=0 XHE_ADD_WAVE=0", "MONT"),
    ("add K=2048 lanes=4 count=1 dmax=0 XHE_ADD_WAVE=0", "BARRETT"),
    ("add K=2048 lanes=4 count=4097 dmax=0 XHE_ADD_BAR=0", "MONT"),
    ("add K=2048 lanes=4 count=1 dmax=0 XHE_ADD_BAR=0", "WAVE"),
    ("add K=3072 lanes=16 count=1 dmax=0", "MONT"),
    ("add K=3072 lanes=16 count=256 dmax=0", "MONT"),
    ("add K=3072 lanes=16 count=257 dmax=0", "MONT"),
    ("add K=3072 lanes=4 count=4097 dmax=0", "MONT"),
    ("add K=4096 lanes=16 count=1 dmax=0", "MONT"),
    ("add K=4096 lanes=16 count=4097 dmax=0", "MONT"),
    ("add K=8192 lanes=16 count=1 dmax=0", "MONT"),
    ("add K=8192 lanes=16 count=4097 dmax=0", "MONT"),
]

ROWS["powmod"] = [
    ("powmod K=2048 lanes=4 ndig=1", "NDIG"),
    ("powmod K=2048 lanes=16 ndig=1", "MONT"),
    ("powmod K=2048 lanes=4 ndig=0", "MONT"),
    ("powmod K=2048 lanes=4 ndig=1 XHE_NDIG=0", "MONT"),
    ("powmod K=3072 lanes=4 ndig=0", "MONT"),
    ("powmod K=3072 lanes=4 ndig=1", "MONT"),
    ("powmod K=3072 lanes=16 ndig=0", "MONT"),
    ("powmod K=4096 lanes=16 ndig=0", "MONT"),
    ("powmod K=8192 lanes=16 ndig=0", "MONT"),
]

ROWS["invert"] = [
    ("invert K=2048 lanes=16 count=1", "WTREE"),
    ("invert K=2048 lanes=16 count=256", "WTREE"),
    ("invert K=2048 lanes=16 count=257", "TREE"),
    ("invert K=2048 lanes=4 count=1", "TREE"),
    ("invert K=2048 lanes=4 count=256", "TREE"),
    ("invert K=2048 lanes=4 count=4097", "TREE"),
    ("invert K=3072 lanes=16 count=1", "TREE"),
    ("invert K=3072 lanes=16 count=256", "TREE"),
    ("invert K=3072 lanes=16 count=257", "TREE"),
    ("invert K=4096 lanes=16 count=1", "TREE"),
    ("invert K=8192 lanes=16 count=1", "TREE"),
]

ROWS["segprod"] = [
    ("segprod count=1 dmax=0 has_d=1", "WORDS"),
    ("segprod count=1 dmax=0 has_d=0", "WORDS"),
    ("segprod count=1 dmax=3 has_d=0", "WORDS"),
    ("segprod count=1 dmax=3 has_d=1", "ALIGN"),
    ("segprod count=0 dmax=0 has_d=0", "ALIGN"),
    ("segprod count=1 dmax=0 has_d=1 XHE_SUM_WORDS=0", "ALIGN"),
]

ROWS["horner"] = [
    ("horner K=2048 lanes=16 ncols=1", "WAVE"),
    ("horner K=2048 lanes=16 ncols=4096", "WAVE"),
    ("horner K=2048 lanes=16 ncols=4097", "LANES"),
    ("horner K=2048 lanes=4 ncols=1", "LANES"),
    ("horner K=2048 lanes=16 ncols=1 XHE_MEXP_WAVE=0", "LANES"),
    ("horner K=3072 lanes=16 ncols=1", "LANES"),
    ("horner K=3072 lanes=16 ncols=4096", "LANES"),
    ("horner K=3072 lanes=16 ncols=4097", "LANES"),
    ("horner K=4096 lanes=16 ncols=1", "LANES"),
    ("horner K=8192 lanes=16 ncols=1", "LANES"),
]

# decrypt, by the whole call's count
_E2 = "decrypt K=2048 lanes=1 pmdx_dec=0 rns=1"
_E3 = "decrypt K=3072 lanes=2 pmdx_dec=1 rns=0"
_E3N = "decrypt K=3072 lanes=2 pmdx_dec=0 rns=0"
ROWS["decrypt"] = [
    (f"{_E2} count=1", "RNS"),
    (f"{_E2} count=1024", "RNS"),
    (f"{_E2} count=1025", "ROW16"),
    (f"{_E2} count=5120", "ROW16"),
    (f"{_E2} count=5121", "QUAD4"),
    (f"{_E2} count=28672", "QUAD4"),
    (f"{_E2} count=28673", "PMD1"),
    ("decrypt K=2048 lanes=1 pmdx_dec=0 rns=0 count=1", "WAVE"),
    ("decrypt K=2048 lanes=1 pmdx_dec=0 rns=0 count=1025", "ROW16"),
    (f"{_E2} count=1 XHE_DEC_RNS=0", "WAVE"),
    (f"{_E2} count=1 XHE_DEC_TPI=1", "PMD1"),
    (f"{_E2} count=1 XHE_DEC_TPI=4", "QUAD4"),
    (f"{_E2} count=1 XHE_DEC_TPI=16", "ROW16"),
    (f"{_E2} count=28673 XHE_DEC_TPI=64", "RNS"),
    (f"{_E2} count=28673 XHE_DEC_TPI=64 XHE_DEC_RNS=0", "WAVE"),
    (f"{_E2} count=1 XHE_DEC_TPI=8", "RNS"),
    (f"{_E2} count=28673 XHE_DEC_TPI=8", "PMD1"),
    ("decrypt K=2048 lanes=1 pmdx_dec=1 rns=1 count=5121", "QUAD4"),  # the digit decrypt is for the larger keys
    (f"{_E2} count=5121 XHE_DEC_PMDX=0", "QUAD4"),
    # 3072 bits: no block kernels; the digits where the batch size chooses 4 lanes,
    # which a multi-lane batch shape does for every larger batch
    (f"{_E3} count=1", "ROW16"),
    (f"{_E3} count=1024", "ROW16"),
    (f"{_E3} count=1025", "ROW16"),
    (f"{_E3} count=5120", "ROW16"),
    (f"{_E3} count=5121", "PMDX"),
    (f"{_E3} count=28672", "PMDX"),
    (f"{_E3} count=28673", "PMDX"),
    (f"{_E3N} count=5120", "ROW16"),
    (f"{_E3N} count=5121", "QUAD4"),
    (f"{_E3N} count=28673", "QUAD4"),
    (f"{_E3} count=5121 XHE_DEC_PMDX=0", "QUAD4"),
    (f"{_E3} count=1 XHE_DEC_TPI=64", "ROW16"),
    (f"{_E3N} count=1 XHE_DEC_TPI=64", "ROW16"),
    (f"{_E3} count=28673 XHE_DEC_TPI=64", "ROW16"),
    # pinned: the digits answer the one-lane pin, the 4-lane pin is the Montgomery shape
    (f"{_E3} count=1 XHE_DEC_TPI=1", "PMDX"),
    (f"{_E3N} count=1 XHE_DEC_TPI=1", "POW1"),
    (f"{_E3} count=1 XHE_DEC_TPI=1 XHE_DEC_PMDX=0", "POW1"),
    (f"{_E3} count=1 XHE_DEC_TPI=4", "QUAD4"),
    (f"{_E3} count=5121 XHE_DEC_TPI=4", "QUAD4"),
    (f"{_E3N} count=1 XHE_DEC_TPI=4", "QUAD4"),
    (f"{_E3} count=5121 XHE_DEC_TPI=16", "ROW16"),
    (f"{_E3} count=5121 XHE_DEC_TPI=8", "PMDX"),
    (f"{_E3} count=1 XHE_DEC_RNS=0", "ROW16"),
    ("decrypt K=4096 lanes=4 pmdx_dec=1 rns=0 count=1", "ROW16"),
    ("decrypt K=4096 lanes=4 pmdx_dec=1 rns=0 count=1024", "ROW16"),
    ("decrypt K=4096 lanes=4 pmdx_dec=1 rns=0 count=1025", "ROW16"),
    ("decrypt K=4096 lanes=4 pmdx_dec=1 rns=0 count=5120", "ROW16"),
    ("decrypt K=4096 lanes=4 pmdx_dec=1 rns=0 count=5121", "PMDX"),
    ("decrypt K=4096 lanes=4 pmdx_dec=1 rns=0 count=28672", "PMDX"),
    ("decrypt K=4096 lanes=4 pmdx_dec=1 rns=0 count=28673", "PMDX"),
    ("decrypt K=4096 lanes=4 pmdx_dec=0 rns=0 count=28673", "QUAD4"),
    ("decrypt K=4096 lanes=4 pmdx_dec=1 rns=0 count=1 XHE_DEC_TPI=1", "PMDX"),
    ("decrypt K=4096 lanes=4 pmdx_dec=0 rns=0 count=1 XHE_DEC_TPI=1", "POW1"),
    ("decrypt K=8192 lanes=16 pmdx_dec=1 rns=0 count=1", "ROW16"),
    ("decrypt K=8192 lanes=16 pmdx_dec=1 rns=0 count=1024", "ROW16"),
    ("decrypt K=8192 lanes=16 pmdx_dec=1 rns=0 count=1025", "ROW16"),
    ("decrypt K=8192 lanes=16 pmdx_dec=1 rns=0 count=5120", "ROW16"),
    ("decrypt K=8192 lanes=16 pmdx_dec=1 rns=0 count=5121", "PMDX"),
    ("decrypt K=8192 lanes=16 pmdx_dec=1 rns=0 count=28672", "PMDX"),
    ("decrypt K=8192 lanes=16 pmdx_dec=1 rns=0 count=28673", "PMDX"),
    ("decrypt K=8192 lanes=16 pmdx_dec=0 rns=0 count=28673", "QUAD4"),
    ("decrypt K=8192 lanes=16 pmdx_dec=1 rns=0 count=1 XHE_DEC_TPI=64", "ROW16"),
]


def build_paths_check(folder):
    """tests/native/paths_check.cpp compiled into `folder` -> the program's path
    (also used by tests/test_pinned_paths_host.py)"""
    exe = os.path.join(str(folder), "paths_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    os.path.join(HERE, "native", "paths_check.cpp"), "-o", exe], check=True)
    return exe


def ask_paths_check(exe, lines):
    """{input line: printed answer} of one run of the check program over `lines`"""
    assert len(set(lines)) == len(lines), "a row is listed twice"
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    out = r.stdout.splitlines()
    assert len(out) == len(lines), r.stdout
    return dict(zip(lines, out))


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """{input line: printed answer} of one run of the check program over every row"""
    exe = build_paths_check(tmp_path_factory.mktemp("paths"))
    return ask_paths_check(exe, [line for rows in ROWS.values() for line, _ in rows])


@pytest.mark.parametrize("op", sorted(ROWS))
def test_paths(answers, op):
    wrong = [(line, answers[line], want) for line, want in ROWS[op] if answers[line] != want]
    assert not wrong, "\n".join(f"{line}: chose {got}, expected {want}" for line, got, want in wrong)


def test_header_is_host_only():
    """paths.hpp: standard headers only, no environment and no HIP call of its own"""
    src = open(os.path.join(ROOT, "xfl_amd", "csrc", "paths.hpp")).read()
    assert re.findall(r'#include\s*"', src) == []
    code = re.sub(r"//[^\n]*", "", src)
    assert "getenv" not in code and not re.search(r"\bhip[A-Z_]", code)


def test_native_mirror(answers):
    """_native.PUB_WAVE_MAX (read from the source: no library is loaded) is paths.hpp's kPubWaveMax"""
    src = open(os.path.join(ROOT, "xfl_amd", "_native.py")).read()
    mirrored = re.findall(r"^PUB_WAVE_MAX = (\d+)\b", src, flags=re.M)
    assert len(mirrored) == 1
    printed = dict(kv.split("=") for kv in answers["const"].split())
    assert printed["kPubWaveMax"] == mirrored[0] == "2048"
