"""np.cumsum / Series.cumsum / cumsum_segments over ciphertext arrays on the
GPU: tests/cumsum_cases.py's checks on the real xhe_segscan (resident inputs
give resident results), and a histogram scanned, packed and unpacked."""
import numpy as np
import pytest

from oracle import paillier_oracle as O
from tests import cumsum_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture
def calls(monkeypatch):
    """the calls that reach the device scan, recorded around the real entry points"""
    from xfl_amd.paillier import ops
    seen = []
    real_dev, real_words = ops.segscan_dev, ops.segscan_words

    def segscan_dev(ctx, dk, cd, seg):
        seen.append(np.asarray(seg).tolist())
        return real_dev(ctx, dk, cd, seg)

    def segscan_words(ctx, cw, seg):
        seen.append(np.asarray(seg).tolist())
        return real_words(ctx, cw, seg)
    monkeypatch.setattr(ops, "segscan_dev", segscan_dev)
    monkeypatch.setattr(ops, "segscan_words", segscan_words)
    return seen


def test_scans(calls):
    priv, pub = CC.keys()
    assert CC.encrypt(pub, CC.plain(5)).is_resident  # what "resident when the input was" is checked on
    CC.scans(calls)


def test_pandas_columns(calls):
    CC.pandas_columns(calls)


def test_fallbacks(calls):
    CC.fallbacks(calls)


def test_lines_of_different_exponents(calls):
    CC.lines_of_different_exponents(calls)


def test_cumsum_segments(calls):
    CC.segments(calls)


def test_host_inputs_and_host_mode(calls, monkeypatch):
    """a host array is uploaded and its result resident; without a resident device the host entry point serves"""
    from xfl_amd.paillier import PaillierArray
    priv, pub = CC.keys()
    arr = CC.encrypt(pub, CC.plain(70, 11))
    host = PaillierArray.from_buffers(pub, np.array(arr.words), arr.exponents.copy())
    assert not host.is_resident
    on_dev = np.cumsum(host)
    assert on_dev.is_resident and CC.ints(on_dev) == CC.ints(np.cumsum(arr))
    monkeypatch.setenv("XHE_RESIDENT", "0")
    on_host = np.cumsum(PaillierArray.from_buffers(pub, np.array(arr.words), arr.exponents.copy()))
    assert not on_host.is_resident and CC.ints(on_host) == CC.ints(on_dev)


def test_histogram_scan_pack_unpack(calls):
    """two features' histograms (13 and 8 bins) concatenated, scanned in one call, packed and unpacked: the
    label trainer reads the cumulative grad / hess columns, equal to the reference's umbed of the exact
    cumulative integer bin sums"""
    import pandas as pd

    from xfl_amd.paillier import Paillier, PaillierArray
    from xfl_amd.paillier_acceleration import (cumsum_segments, decrypt_unpack, embed_packed, pack_ciphertexts,
                                               pack_factor)
    priv, pub = CC.keys()
    nsamples, lengths = 120, [13, 8]
    rng = np.random.default_rng(23)
    cols = [rng.random(nsamples) - 0.5, rng.random(nsamples) * 0.25]
    ints = O.embed_ref(cols)
    enc = Paillier.encrypt(pub, embed_packed(cols), precision=0, obfuscation=True)
    sums, exact = [], []
    for f, nb in enumerate(lengths):
        bins = rng.integers(0, nb, nsamples)
        bins[:nb] = np.arange(nb)  # no empty bin
        data = pd.DataFrame(enc, columns=["xfl_grad_hess"])
        data["bin"] = bins
        sums.append(data.groupby(["bin"])["xfl_grad_hess"].agg(["sum"])["sum"].array)
        exact += list(np.cumsum(np.array([sum(ints[i] for i in np.nonzero(bins == b)[0]) for b in range(nb)],
                                         dtype=object)))
    all_bins = PaillierArray._concat_same_type(sums)
    assert all_bins.shape == (sum(lengths),) and not all_bins.exponents.any()
    before = len(calls)
    cum = cumsum_segments(all_bins, lengths)
    assert len(calls) == before + 1 and cum.is_resident == all_bins.is_resident
    packed = pack_ciphertexts(cum)
    assert packed.shape == (-(-sum(lengths) // pack_factor(pub.n)),)
    back = Paillier.ciphertext_from(priv, Paillier.serialize(packed, compression=False), compression=False)
    got = decrypt_unpack(priv, back, sum(lengths))
    want = [np.array(c, dtype=np.float32).view(np.uint32) for c in O.umbed_ref(exact, 2)]
    for j in range(2):
        assert np.array_equal(got[j].view(np.uint32), want[j]), j
