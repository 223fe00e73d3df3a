"""CPU: the host half of the device decode of received payloads
(Paillier.ciphertext_from, paillier.py:260-271).

* xhe_wire_scan - the index of a payload in the library's own layout: value
  offsets, used lengths, exponents, shape - against wire.decode_words on the
  same bytes, whole and range by range; every other pickle form is refused.
* xhe_zstd_raw_probe / xhe_zstd_raw_extract_range against xhe_zstd_raw_extract.
* tests/native/wire_scan_fuzz.cpp under AddressSanitizer + UBSan: the scan on
  truncated, flipped and inflated payloads, and the per-quad unpack function
  of k_wire_unpack (wire_unpack.hpp) on the CPU, hostile indices included.
"""
import ctypes
import os
import pickle
import subprocess

import numpy as np
import pytest

from tests import wire_cases as wc
from tests.conftest import FIXTURES, ROOT, hx, load_fixture

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]

_payloads = {}


def payload(n2w, count):
    """(bytes, words, exps, shape) of a case, made once"""
    from xfl_amd.paillier import wire
    key = (n2w, count)
    if key not in _payloads:
        w, e, shape = wc.make(n2w, count)
        _payloads[key] = (wire.encode_words(w, e, shape), w, e, shape)
    return _payloads[key]


@pytest.mark.parametrize("n2w,count", wc.cases())
def test_scan_reproduces_decode(n2w, count):
    from xfl_amd import _native as nat
    from xfl_amd.paillier import wire
    data, w, e, shape = payload(n2w, count)
    dw, de, dshape = wire.decode_words(data, n2w)
    assert np.array_equal(dw, w) and np.array_equal(de, e) and dshape == shape
    for window in (None, 4096):
        rc, off, ln, ex, sshape = wc.scan(nat, data, n2w, window)
        assert rc == nat.XHE_OK
        assert sshape == dshape and np.array_equal(ex, de)
        assert np.array_equal(wc.rows_of(data, off, ln, n2w), dw), window
        # used length: the top zero bytes trimmed
        bw = dw.view(np.uint8)
        used = np.where(bw.any(axis=1), bw.shape[1] - np.argmax(bw[:, ::-1] != 0, axis=1), 0)
        assert np.array_equal(ln, used)


def test_scan_covers_the_element_forms():
    """the cases hold what they are meant to: LONG1 and LONG4 values, the
    extra sign byte, zero, both exponent forms"""
    data = b"".join(payload(n2w, count)[0] for n2w, count in wc.cases() if count in (1, 1001))
    assert b"\x8a\x00h\x03" in data                                  # a zero value
    assert b"\x8b\x01\x02\x00\x00" in data                           # nb = 4 * 128 + 1
    assert b"\x8a\xff" in data and b"\x8b\x00\x01\x00\x00" in data   # nb = 255 / 256
    for e in wc.EXPS:
        form = b"K" + bytes([e]) if 0 <= e < 256 else b"J" + int(e).to_bytes(4, "little", signed=True)
        assert b"h\x03" + form + b"ub" in data
    shapes = {payload(n2w, count)[3] for n2w, count in wc.cases()}
    assert any(len(s) == 1 for s in shapes) and any(len(s) == 2 and s[1] == 1 for s in shapes)
    assert any(len(s) == 2 and max(s) > 255 and s[1] != 1 for s in shapes)


def test_scan_reports_the_count_when_the_arrays_are_small():
    from xfl_amd import _native as nat
    data = payload(128, 1001)[0]
    rc, found, *_ = wc.scan(nat, data, 128, cap=10)
    assert rc == nat.XHE_EOVERFLOW and found == 1001


def test_scan_refuses_a_narrower_width():
    """a value above n2w words: the rejection of the host decode"""
    from xfl_amd import _native as nat
    rc, *_ = wc.scan(nat, payload(192, 999)[0], 128)
    assert rc == nat.XHE_ENOTSUP


def _foreign():
    """the reference's own bytes (gmpy2 values) and CPython's pickles of the
    same object graph"""
    from xfl_amd import compat
    from xfl_amd.paillier.paillier import RawCiphertext
    compat._register_alias()
    out = [(f"ref_{fx}", bytes.fromhex(load_fixture(fx)["ops"]["wire_a4"])) for fx in FIXTURES]
    g = load_fixture(FIXTURES[0])
    arr = np.empty(5, dtype=object)
    for i, (r, e) in enumerate(zip(g["ops"]["a"]["raw"][:5], g["ops"]["a"]["exp"][:5])):
        arr[i] = RawCiphertext(hx(r), e)
    return out + [(f"cpython_p{p}", pickle.dumps(arr.reshape(5, 1), protocol=p)) for p in (2, 3, 4, 5)]


def test_other_pickle_forms_are_refused():
    from xfl_amd import _native as nat
    from xfl_amd.paillier import wire
    for name, data in _foreign():
        assert wire.decode_words(data, 512)[0].shape[0] > 0, name  # the general machine reads it
        for window in (None, 4096):
            rc, *_ = wc.scan(nat, data, 512, window)
            assert rc == nat.XHE_ENOTSUP, (name, window)
        assert wire.peek_shape(wire._Source(data), 512) is None, name


def test_peek_shape():
    from xfl_amd.paillier import wire
    for n2w, count in wc.cases():
        data, _, _, shape = payload(n2w, count)
        assert wire.peek_shape(wire._Source(data), n2w) == shape


def test_range_extract_equals_the_slice():
    from xfl_amd import _native as nat
    from xfl_amd import compat
    L = nat.lib()
    blk = 128 << 10
    rng = np.random.default_rng(8)
    content = rng.integers(0, 256, size=8 * blk + 4321, dtype=np.uint8).tobytes()  # above compat.RAW_FRAME_MIN
    frame = compat.compress(content)
    assert compat.raw_frame_size(frame) == len(content)
    whole = compat.decompress(frame)
    assert whole == content
    n = len(content)
    ranges = [(0, 1), (0, n), (0, blk), (blk, 2 * blk), (blk - 1, blk + 1), (blk - 7, 2 * blk + 9), (5, blk - 5),
              (2 * blk + 3, n), (8 * blk, n), (8 * blk - 1, 8 * blk + 1), (n - 1, n), (blk, blk), (1, n - 1)]
    for lo, hi in ranges:
        dst = np.full(hi - lo + 2, 0xA5, dtype=np.uint8)
        assert L.xhe_zstd_raw_extract_range(frame, len(frame), lo, hi, dst[1:].ctypes.data) == nat.XHE_OK
        assert dst[1:1 + hi - lo].tobytes() == whole[lo:hi], (lo, hi)
        assert dst[0] == 0xA5 and dst[-1] == 0xA5
    assert L.xhe_zstd_raw_extract_range(frame, len(frame), 0, n + 1, dst.ctypes.data) == nat.XHE_EINVAL
    # a frame cut short, and one with a damaged block header in the range
    assert L.xhe_zstd_raw_extract_range(frame, len(frame) - 1, 8 * blk, n, dst.ctypes.data) == nat.XHE_ENOTSUP
    bad = bytearray(frame)
    bad[14 + blk + 3] ^= 2
    size = ctypes.c_int64()
    assert L.xhe_zstd_raw_probe(bytes(bad), len(bad), ctypes.byref(size)) == nat.XHE_ENOTSUP
    assert L.xhe_zstd_raw_extract_range(bytes(bad), len(bad), blk, blk + 1, dst.ctypes.data) == nat.XHE_ENOTSUP


def test_probe_refuses_a_compressed_frame():
    """libzstd level 3, what an unmodified peer sends"""
    from xfl_amd import _native as nat
    from xfl_amd import compat
    L = nat.lib()
    data = bytes(2 << 20)
    Z = compat._lib()
    cap = Z.ZSTD_compressBound(len(data))
    dst = ctypes.create_string_buffer(cap)
    n = Z.ZSTD_compress(dst, cap, data, len(data), 3)
    assert not Z.ZSTD_isError(n)
    frame = dst.raw[:n]
    size = ctypes.c_int64()
    assert L.xhe_zstd_raw_probe(frame, len(frame), ctypes.byref(size)) == nat.XHE_ENOTSUP
    small = compat.compress(payload(128, 999)[0])  # below RAW_FRAME_MIN: level 3 as well
    assert L.xhe_zstd_raw_probe(small, len(small), ctypes.byref(size)) == nat.XHE_ENOTSUP
    assert compat.raw_frame_size(small) is None


def test_wire_dev_defaults():
    from xfl_amd.paillier import wire
    assert wire.DEV_DECODE_MIN >= 1 and wire.DEV_CHUNK % 16 == 0


# ------------------------------------------------------------ under the sanitizers
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wirescan") / "wire_scan_fuzz")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread", *SAN,
                    os.path.join(HERE, "native", "wire_scan_fuzz.cpp"),
                    os.path.join(ROOT, "xfl_amd", "csrc", "wire_abi.cpp"), "-o", exe], check=True)
    return exe


def _env():
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    env.pop("LD_PRELOAD", None)  # the sanitizer runtime must come first in the child
    return env


def test_scan_fuzz_under_sanitizers(harness, tmp_path):
    """one run per width, side by side"""
    runs = []
    for n2w in wc.WIDTHS:
        seeds = []
        for count in wc.COUNTS:
            p = tmp_path / f"own_{n2w}_{count}.bin"
            p.write_bytes(payload(n2w, count)[0])
            seeds.append(str(p))
        for name, data in _foreign():
            p = tmp_path / f"foreign_{n2w}_{name}.bin"
            p.write_bytes(data)
            seeds.append(str(p))
        runs.append((n2w, len(seeds), subprocess.Popen([harness, "scan", str(n2w), *seeds], stdout=subprocess.PIPE,
                                                       stderr=subprocess.PIPE, text=True, env=_env())))
    for n2w, nseeds, p in runs:
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0, (n2w, err[-4000:])
        f = out.split()
        assert f[0] == "own" and int(f[1]) == len(wc.COUNTS) and int(f[3]) == nseeds - len(wc.COUNTS), out
        accepted, refused = int(f[5]), int(f[7])
        assert accepted > 100 and refused > 100000, out  # flips inside values decode; every truncation is refused


def test_unpack_quad_under_sanitizers(harness):
    r = subprocess.run([harness, "unpack"], capture_output=True, text=True, env=_env(), timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert int(r.stdout.split()[2]) > 4 * (16 * 10 * 2 + 5 * 13 * 9) - 1, r.stdout
