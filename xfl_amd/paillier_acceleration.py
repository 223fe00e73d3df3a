"""Drop-in for python/algorithm/core/paillier_acceleration.py: packing several
fixed-point values into one Paillier plaintext (SecureBoost grad/hess,
decision_tree_label_trainer.py:108-119) and unpacking decrypted sums.

Same functions, arguments and results as the reference:
  embed(p_list, interval=2^128, precision=64)   paillier_acceleration.py:21-32
      x = int(p0 * 2^precision) * interval^(k-1) + ... (int() truncates toward 0)
  umbed(a, num, interval=2^128, precison=64)    :35-59  centred base-`interval`
      digits, each / 2^precision (correctly rounded true division) -> float32
  unpack(x, num, ...)                           :62-81  one value, Python floats

embed is vectorised: for the reference's (interval, precision) the scaled
integers int(v * 2^precision) are formed exactly from each float's mantissa
and exponent (numpy, no per-element Python float arithmetic), then the packed
Python ints are assembled; umbed / unpack work on Python ints exactly as the
reference does (their inputs are decrypted Python ints).

Two additions move both ends onto the GPU, next to the encryption and
decryption they feed (xhe_embed_f64 / xhe_umbed, include/xhe.h):
  embed_packed(p_list, interval, precision) -> PackedPlain: embed's result
      kept as its float64 columns; Paillier.encrypt packs them on the device
  decrypt_umbed(context, data, num, interval, precison, num_cores): umbed of
      Paillier.decrypt(..., out_origin=True), unpacked behind the decryption

And one pair packs ciphertexts themselves (opt-in, both parties run this
library; xhe_pack): a grad/hess plaintext uses num * log2(interval) = 256
bits, so a party holding only the public key can fold k of them into one
  pack_factor(n, num, interval) -> k (7 at 2048 bits)
  pack_ciphertexts(arr, num, interval, k) -> ceil(count / k) ciphertexts
  decrypt_unpack(context, packed, count, num, interval, precison, k) ->
      decrypt_umbed's floats of the count ciphertexts that were packed
"""
from typing import List

import numpy as np


def _scaled_ints(v: np.ndarray, precision: int) -> List[int]:
    """[int(x * (1 << precision)) for x in v] for a float array, exactly:
    x * 2^p is exact in binary floating point (a power-of-two scale, no
    overflow for |x| < 2^(1024-p)), int() truncates toward zero."""
    v = np.asarray(v, dtype=np.float64)
    if not np.all(np.isfinite(v)):
        raise OverflowError("cannot convert float infinity to integer")
    mant, exp = np.frexp(v)  # v = mant * 2^exp, 0.5 <= |mant| < 1
    m53 = (mant * (1 << 53)).astype(np.int64)  # exact 53-bit signed mantissa
    sh = exp.astype(np.int64) - 53 + precision  # v * 2^p = m53 * 2^sh
    out = []
    for m, s in zip(m53.tolist(), sh.tolist()):
        if s >= 0:
            out.append(m << s)
        else:
            a = (-m if m < 0 else m) >> (-s)  # truncation toward zero
            out.append(-a if m < 0 else a)
    return out


def embed(p_list: List[np.ndarray], interval: int = (1 << 128), precision: int = 64):
    """paillier_acceleration.py:21-32"""
    cols = [_scaled_ints(p, precision) for p in p_list]
    out = [0] * len(cols[0])
    for i in range(len(out)):
        x = cols[0][i]
        for c in cols[1:]:
            x = x * interval + c[i]
        out[i] = x
    return np.array(out)


def packed_geometry(n: int, slots: int, interval: int, precision: int):
    """log2(interval) when the device packs / unpacks this geometry for the
    modulus n (include/xhe.h: whole-word slots of 64..256 bits, precision at
    most two bits below the slot, every slot below n's top bit), else None."""
    if not isinstance(interval, int) or not isinstance(precision, int) or interval <= 0:
        return None
    ib = interval.bit_length() - 1
    if interval != 1 << ib or ib % 32 or not 64 <= ib <= 256 or not 0 <= precision <= ib - 2:
        return None
    if slots < 1 or slots * ib > int(n).bit_length() - 1:
        return None
    return ib


class PackedPlain:
    """What embed(p_list, interval, precision) returns, kept as its float64
    columns so that Paillier.encrypt can pack on the GPU: 8 bytes per value go
    up and no Python integer is made. Wherever it is looked at it is the
    object array embed returns: len, shape, ndim, dtype, x[i] (a Python int),
    slices (a PackedPlain), iteration, and np.asarray(x) (embed's array,
    built on first use)."""
    __slots__ = ("cols", "interval", "precision", "_arr")

    def __init__(self, cols: np.ndarray, interval: int, precision: int):
        self.cols = cols  # [k, N] float64, C-contiguous, finite
        self.interval = interval
        self.precision = precision
        self._arr = None

    def __len__(self):
        return self.cols.shape[1]

    @property
    def shape(self):
        return (self.cols.shape[1],)

    ndim = 1
    dtype = np.dtype(object)

    def __array__(self, dtype=None, copy=None):
        if self._arr is None:
            self._arr = embed(list(self.cols), self.interval, self.precision)
        return self._arr if dtype is None else self._arr.astype(dtype)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return PackedPlain(np.ascontiguousarray(self.cols[:, i]), self.interval, self.precision)
        if isinstance(i, (int, np.integer)):
            if self._arr is not None:
                return int(self._arr[i])
            j = range(len(self))[i]  # IndexError and negative indices as a sequence's
            return int(embed(list(self.cols[:, j:j + 1]), self.interval, self.precision)[0])
        return self.__array__()[i]

    def __iter__(self):
        return iter(self.__array__())


def embed_packed(p_list: List[np.ndarray], interval: int = (1 << 128), precision: int = 64) -> PackedPlain:
    """embed for values on their way to Paillier.encrypt: the same packed
    integers (np.asarray of the result is embed's array), formed on the GPU by
    Paillier.encrypt instead of one Python int per sample here."""
    cols = np.ascontiguousarray([np.asarray(p, dtype=np.float64).reshape(-1) for p in p_list], dtype=np.float64)
    if not np.all(np.isfinite(cols)):
        raise OverflowError("cannot convert float infinity to integer")
    return PackedPlain(cols, interval, precision)


def decrypt_umbed(context, data, num: int, interval: int = (1 << 128), precison: int = 64, num_cores: int = -1):
    """umbed(Paillier.decrypt(context, data, num_cores=num_cores,
    out_origin=True), num, interval, precison) as `num` float32 arrays, bit for
    bit: for a ciphertext array the digits are taken and scaled on the GPU
    behind the decryption, and only the floats come back. Missing entries,
    nonzero exponents and geometries outside packed_geometry take the two
    steps on the host."""
    from .paillier import Paillier, PaillierCiphertext, ops, resident
    from .paillier.array import SMALL, PaillierArray
    if not context.is_private():
        raise TypeError("Try to decrypt a paillier ciphertext by a public key.")
    ib = packed_geometry(context.n, num, interval, precison)
    arr = data
    if ib is not None and isinstance(arr, np.ndarray) and arr.dtype == object and arr.ndim == 1 and arr.size and \
            all(isinstance(c, PaillierCiphertext) for c in arr):
        arr = PaillierArray(arr, context=context)
    if ib is not None and isinstance(arr, PaillierArray) and arr.ndim == 1 and arr.size and not arr._has_na() and \
            not arr.exponents.any():
        arr = arr._aligned_words(ops.n2w_of(context))
        dev = resident.device_for(context, num_cores)
        if arr._resident_on(dev) or (dev is not None and arr.size <= SMALL):
            f32, st = resident.decrypt_umbed(context.device_key(dev), arr._dw(dev), num, ib, precison)
        else:
            f32, st = ops.decrypt_umbed_words(context, arr.words, num, ib, precison, num_cores)
        if np.any(st != 0):
            raise OverflowError("Overflow detected during decoding encrypted number.")
        return [f32[j] for j in range(num)]
    vals = Paillier.decrypt(context, data, num_cores=num_cores, out_origin=True)
    return [np.array(col, dtype=np.float32) for col in umbed(vals, num, interval, precison)]


def pack_factor(n: int, num: int = 2, interval: int = (1 << 128)) -> int:
    """How many ciphertexts of `num` slots pack_ciphertexts folds into one
    under the modulus n: the largest k with k * num * log2(interval) <=
    bitlen(n) - 2 (one bit below xhe_umbed's geometry, so the packed value
    keeps the sign rule of a single one); 0 when the device does not unpack
    this slot width at all (packed_geometry refuses k = 1)."""
    if packed_geometry(n, num, interval, 0) is None:
        return 0
    return (int(n).bit_length() - 2) // (num * (interval.bit_length() - 1))


def _pack_k(n, num, interval, k):
    kmax = pack_factor(n, num, interval)
    if kmax < 1:
        raise ValueError("pack: this (num, interval) is not a device packing geometry for the key")
    if k is None:
        return kmax
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= k <= kmax:
        raise ValueError(f"pack: k must be in [1, {kmax}] for this key, num and interval")
    return int(k)


def pack_ciphertexts(arr, num: int = 2, interval: int = (1 << 128), k: int = None):
    """Fold every k consecutive ciphertexts of a 1-D array into one (cipher
    compressing): with s = num * log2(interval) plaintext bits per input,
    out[j] = ((c[jk]^(2^s) * c[jk+1])^(2^s) * ...) mod n^2, whose plaintext
    sum_t x[jk+t] * 2^(s (k-1-t)) is embed's layout with num * k slots; a short
    last group is filled with encryptions of 0. k defaults to
    pack_factor(n, num, interval). Needs only the public key; every input must
    be at exponent 0 (embed_packed's). Returns a PaillierArray of ceil(count /
    k) ciphertexts at exponent 0, in HBM when the input is; decrypt_unpack is
    the receiving side.

    One call walks (k - 1) * s dependent squarings per output whatever the
    batch: pack everything a message carries in one call."""
    from .paillier import PaillierCiphertext, ops, resident
    from .paillier.array import PaillierArray
    if isinstance(arr, np.ndarray) and arr.dtype == object and arr.ndim == 1 and \
            all(isinstance(c, PaillierCiphertext) for c in arr):
        arr = PaillierArray(arr)
    if not isinstance(arr, PaillierArray):
        raise TypeError("pack_ciphertexts takes a PaillierArray or an object array of PaillierCiphertext")
    if arr.ndim != 1:
        raise ValueError("pack_ciphertexts takes a 1-D array")
    context = arr.context
    if context is None:
        raise ValueError("ciphertext array without a context: pass one to Paillier.ciphertext_from")
    k = _pack_k(context.n, num, interval, k)
    if arr._has_na():
        raise ValueError("pack_ciphertexts: missing entries cannot be packed")
    if arr.exponents.any():
        raise ValueError("pack_ciphertexts: every ciphertext must be at exponent 0")
    shift = num * (interval.bit_length() - 1)
    ng = -(-arr.size // k)
    exps = np.zeros(ng, dtype=np.int32)
    arr = arr._aligned_words(ops.n2w_of(context))
    if not arr.size:
        return PaillierArray.from_buffers(context, np.zeros((0, ops.n2w_of(context)), dtype=np.uint32), exps)
    dev = resident.device_for(context)
    if arr._resident_on(dev):
        return PaillierArray.from_device(context, resident.pack(context.device_key(dev), arr._dw(dev), k, shift), exps)
    return PaillierArray.from_buffers(context, ops.pack_words(context, arr.words, k, shift), exps)


def cumsum_segments(arr, lengths):
    """Cumulative sums of consecutive runs of a 1-D ciphertext array: the run
    of lengths[i] elements after the runs before it is scanned on its own
    (np.cumsum of that slice), all runs in ONE device call - a message's
    per-feature histograms concatenated, with lengths the bin counts. Returns
    a PaillierArray of len(arr) ciphertexts with the inputs' exponents, in HBM
    when the scan ran there; cumulative bins at exponent 0 are what
    pack_ciphertexts takes. Needs only the public key.

    The device path serves arrays with a context, without missing entries and
    with one exponent per run; anything else is the reference's object left
    fold per run, concatenated. A call walks one chain of dependent products
    whatever the batch: scan everything a message carries in one call."""
    from .paillier import PaillierCiphertext
    from .paillier.array import PaillierArray, _Fallback, _scan_segments, _wrap
    if isinstance(arr, np.ndarray) and arr.dtype == object and arr.ndim == 1 and \
            all(isinstance(c, PaillierCiphertext) for c in arr):
        arr = PaillierArray(arr)
    if not isinstance(arr, PaillierArray):
        raise TypeError("cumsum_segments takes a PaillierArray or an object array of PaillierCiphertext")
    if arr.ndim != 1:
        raise ValueError("cumsum_segments takes a 1-D array")
    lens = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if lens.size and lens.min() < 0:
        raise ValueError("cumsum_segments: negative run length")
    if int(lens.sum()) != arr.size:
        raise ValueError(f"cumsum_segments: the run lengths add up to {int(lens.sum())}, the array has {arr.size}")
    seg = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=seg[1:])
    try:
        if lens.size == 0:
            raise _Fallback()
        return _scan_segments(arr, seg)
    except _Fallback:
        obj = np.asarray(arr)
        parts = [np.cumsum(obj[lo:hi]) for lo, hi in zip(seg[:-1], seg[1:]) if hi > lo]
        if not parts:
            return arr.copy()
        res = np.concatenate(parts)
        return PaillierArray._from_sequence(res) if arr._has_na() else _wrap(res)


def unpack_columns(cols, count: int, num: int, k: int):
    """decrypt_unpack's index mapping: cols[t * num + i][j] (the num * k digit
    columns of the packed plaintexts) -> out[i][j * k + t], cut to count."""
    cols = np.asarray(cols)
    ng = cols.shape[1]
    if cols.shape[0] != num * k or not (ng - 1) * k < count <= ng * k:
        raise ValueError("unpack: column count or element count does not match the packing")
    # [t, i, j] -> [i, j, t]
    return [np.ascontiguousarray(c.reshape(-1)[:count]) for c in cols.reshape(k, num, ng).transpose(1, 2, 0)]


def decrypt_unpack(context, packed, count: int, num: int = 2, interval: int = (1 << 128), precison: int = 64,
                   k: int = None, num_cores: int = -1):
    """The receiving side of pack_ciphertexts: `num` float32 arrays of length
    count, equal bit for bit to decrypt_umbed(context, original, num, interval,
    precison) of the ciphertexts that were packed whenever every original
    plaintext is the exact sum of its num centred digits - the condition under
    which the reference's umbed loses nothing. It is decrypt_umbed(context,
    packed, num * k, ...) with column t * num + i, row j moved to output i,
    element j * k + t: ceil(count / k) decryptions instead of count.

    Overflow: a bin sum that outgrows its slot is silently dropped by the
    reference's umbed; here it spills into the neighbouring element's slot.
    The slots must hold the sums (as SecureBoost's choice of interval
    assumes)."""
    k = _pack_k(context.n, num, interval, k)
    count = int(count)
    if count < 0 or len(packed) != -(-count // k):
        raise ValueError("decrypt_unpack: count does not match the packed array")
    if count == 0:
        return [np.zeros(0, dtype=np.float32) for _ in range(num)]
    cols = decrypt_umbed(context, packed, num * k, interval, precison, num_cores)
    return unpack_columns(cols, count, num, k)


def _centred_digits(x, num: int, interval: int):
    res = [0] * num
    b = x % interval
    if abs(b) > interval // 2:
        b = b - interval
    a = (x - b) // interval
    res[-1] = b
    for i in range(num - 1):
        b = a % interval
        if abs(b) > interval // 2:
            b = b - interval
        a = (a - b) // interval
        res[-i - 2] = b
    return res


def umbed(a: np.ndarray, num: int, interval: int = (1 << 128), precison: int = 64) -> List[list]:
    """paillier_acceleration.py:35-59 (argument name `precison` as in the reference)."""
    scale = 1 << precison
    out = [[0] * len(a) for _ in range(num)]
    for i in range(len(a)):
        digits = _centred_digits(a[i], num, interval)
        temp = np.array([d / scale for d in digits]).astype(np.float32)
        for j in range(num):
            out[j][i] = temp[j]
    return out


def unpack(x: float, num: int, interval: int = (1 << 128), precison: int = 64) -> List[list]:
    """paillier_acceleration.py:62-81"""
    scale = 1 << precison
    return [float(d / scale) for d in _centred_digits(x, num, interval)]
