"""CPU: embed_packed's PackedPlain is embed's object array wherever it is
looked at, raises what embed raises, and packed_geometry admits exactly the
geometries the device kernels handle (include/xhe.h)."""
import numpy as np
import pytest

from oracle import paillier_oracle as O
from tests.conftest import FIXTURES, hx, load_fixture
from xfl_amd.paillier_acceleration import PackedPlain, embed, embed_packed, packed_geometry


def _cols():
    rng = np.random.default_rng(5)
    g = np.concatenate([rng.random(40) - 0.5, [0.0, -0.0, 0.5, -0.5, 2.0 ** -70, -(2.0 ** -64), 1 - 2.0 ** -53]])
    h = np.concatenate([(rng.random(40) - 0.2) * 100, [0.0, 1.0, -1.0, 3.0, 2.0 ** -64, 0.25, 7.5]])
    return g, h


def test_packed_plain_is_embeds_array():
    g, h = _cols()
    want = embed([g, h])
    x = embed_packed([g, h])
    assert isinstance(x, PackedPlain)
    assert len(x) == len(want) and x.shape == want.shape == (len(g),) and x.ndim == 1 and x.dtype == object
    assert x.cols.dtype == np.float64 and x.cols.shape == (2, len(g)) and x.cols.flags.c_contiguous
    # element reads before the array exists, then the array, then reads from it
    assert all(type(x[i]) is int for i in (0, 5, -1))
    assert [x[i] for i in range(len(x))] == [int(v) for v in want] == O.embed_ref([g, h])
    assert x[-2] == int(want[-2])
    with pytest.raises(IndexError):
        x[len(x)]
    arr = np.asarray(x)
    assert arr.dtype == want.dtype and arr.shape == want.shape and list(arr) == list(want)
    assert np.asarray(x) is arr
    assert list(x) == list(want) and x[3] == int(want[3])
    for sl in (slice(3, 11), slice(None, None, 3), slice(-5, None), slice(7, 7)):
        s = x[sl]
        assert isinstance(s, PackedPlain) and len(s) == len(want[sl])
        assert list(np.asarray(s)) == list(want[sl])
        assert s.cols.flags.c_contiguous and (s.interval, s.precision) == (x.interval, x.precision)
    assert list(x[np.array([1, 4, 9])]) == list(want[[1, 4, 9]])


def test_three_way_and_other_geometry():
    g, h = _cols()
    three = [g[:30], h[:30], g[10:40] * 3]
    assert list(np.asarray(embed_packed(three))) == O.embed_ref(three)
    two = [g * 2.0 ** -10, h * 2.0 ** -10]
    got = embed_packed(two, interval=1 << 64, precision=32)
    assert list(np.asarray(got)) == O.embed_ref(two, 1 << 64, 32) == list(embed(two, 1 << 64, 32))
    assert got[:4].interval == 1 << 64 and got[:4].precision == 32


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_non_finite_raises_as_embed(bad):
    g, h = _cols()
    h = h.copy()
    h[7] = bad
    with pytest.raises(OverflowError) as want:
        embed([g, h])
    with pytest.raises(OverflowError) as got:
        embed_packed([g, h])
    assert str(got.value) == str(want.value)


def test_packed_geometry():
    assert packed_geometry(hx(load_fixture(FIXTURES[0])["key"]["n"]), 2, 1 << 128, 64) == 128
    n = (1 << 2047) | 1  # a 2048-bit n
    assert packed_geometry(1 << 1920, 15, 1 << 128, 64) == 128  # bitlen(n) - 1 = 1920 bits of slots
    assert packed_geometry((1 << 1920) - 1, 15, 1 << 128, 64) is None
    assert packed_geometry(n, 2, 1 << 128, 64) == 128
    assert packed_geometry(n, 10, 1 << 128, 64) == 128
    assert packed_geometry(n, 2, 1 << 64, 32) == 64
    assert packed_geometry(n, 15, 1 << 128, 126) == 128  # 1920 bits, precision = ib - 2
    assert packed_geometry(n, 7, 1 << 256, 0) == 256
    assert packed_geometry(n, 2, (1 << 128) - 1, 64) is None  # not a power of two
    assert packed_geometry(n, 2, 10 ** 38, 64) is None
    assert packed_geometry(n, 2, 1 << (96 + 8), 64) is None  # not whole words
    assert packed_geometry(n, 17, 1 << 128, 64) is None  # 2176 bits
    assert packed_geometry(n, 16, 1 << 128, 64) is None  # 2048 bits > bitlen(n) - 1
    assert packed_geometry(n, 2, 1 << 32, 8) is None and packed_geometry(n, 2, 1 << 288, 64) is None
    assert packed_geometry(n, 2, 1 << 128, 127) is None and packed_geometry(n, 2, 1 << 128, -1) is None
    assert packed_geometry(n, 0, 1 << 128, 64) is None
