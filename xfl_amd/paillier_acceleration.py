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


def _zero_bins(default_bin, nfeat, nbins):
    """default_bin as one uint16 zero bin per feature (0xFFFF: dense), or None when no feature has one"""
    if default_bin is None:
        return None
    db = np.asarray([-1 if d is None else d for d in np.asarray(default_bin, dtype=object).reshape(-1)],
                    dtype=np.int64)
    if db.size == 1:
        db = np.repeat(db, nfeat)
    if db.size != nfeat:
        raise ValueError("histograms: default_bin must be one bin or one per feature")
    zb = np.where((db < 0) | (db >= nbins), 0xFFFF, db).astype(np.uint16)
    return zb if (zb != 0xFFFF).any() else None


def _total_row(ctx, total, e0, n2w):
    """the [n2w] host words of `total` (a ciphertext or a one-element array) at exponent e0"""
    from .paillier import PaillierCiphertext
    from .paillier.array import PaillierArray
    if isinstance(total, PaillierCiphertext):
        total = PaillierArray(np.array([total], dtype=object))
    if not isinstance(total, PaillierArray) or total.size != 1 or total._has_na():
        raise ValueError("histograms: total must be a ciphertext or a one-element array")
    if int(total.exponents[0]) != e0:
        raise ValueError("histograms: total must be at the column's exponent")
    return np.array(total._aligned_words(n2w).words, dtype=np.uint32).reshape(n2w)  # (a copy: the words are read-only)


def histograms(arr, bins, nbins: int = None, rows=None, default_bin=None, total=None, sparse: bool = None):
    """Every feature's per-bin sums and counts of one ciphertext column in ONE
    device call (xhe_hist): what the per-column
    DataFrame.groupby(feature)[column].agg({'count', 'sum'}) loops of
    decision_tree_trainer.py:131-160 and binning_woe_iv/trainer.py:55-65 compute
    feature by feature. arr: a 1-D PaillierArray (or object array of
    PaillierCiphertext); bins: an [nfeat, len(arr)] integer array of bin ids, or
    a DataFrame of the feature columns (one row per element of arr); negative
    or NaN entries, ids >= nbins and missing ciphertexts are dropped rows.
    nbins defaults to the largest id + 1. rows: indices into arr (a tree
    node's samples, repeats allowed), default all. Returns (sums, counts):
    sums a PaillierArray of shape (nfeat, nbins) - sums[f][b] what
    groupby(bins[f]).sum() gives for group b, an empty bin the encryption of
    0 - at the inputs' common exponent (mixed exponents: each cell at the
    smallest of its own) and in HBM when the input is; counts an
    int64 array of the same shape. Needs only the public key.

    default_bin: an int, or one per feature - the bin that holds the feature's
    value 0 on one-hot, count or mostly-zero data; None or a negative entry
    marks the feature dense. The rows in it are then not multiplied: the bin is
    what is left of the product of all selected elements (xhe_hist_sparse), the
    same ciphertexts bit for bit. total: that product, a ciphertext or a
    one-element array at the column's exponent (the parent node's histogram has
    it in any feature's bins), else it is computed. sparse: None asks the
    planner with the entries outside the default bins counted from `bins`, True
    forces the sparse call, False never takes it. Raises ZeroDivisionError when
    a product that has to be inverted is no unit mod n^2 (never for
    ciphertexts of this key).

    The one-call path serves nbins <= 4096. A column of one exponent goes to
    xhe_hist (or xhe_hist_sparse). A column of mixed exponents - what
    Paillier.encrypt gives with precision=None - goes to xhe_hist_exp when it
    has no missing entries and its selected exponents spread over at most
    bitlen(n) - 2: every cell then comes back at its own smallest exponent,
    the ciphertext the groupby sum gives bit for bit. Anything else takes the
    drop-in's groupby sum feature by feature. Mixed exponents, missing entries
    and more than 4095 bins keep the dense path whatever default_bin says."""
    from .paillier import PaillierCiphertext, ops, resident
    from .paillier.array import NA_EXP, PaillierArray, _Fallback, _result
    if isinstance(arr, np.ndarray) and arr.dtype == object and arr.ndim == 1 and \
            all(isinstance(c, PaillierCiphertext) for c in arr):
        arr = PaillierArray(arr)
    if not isinstance(arr, PaillierArray):
        raise TypeError("histograms takes a PaillierArray or an object array of PaillierCiphertext")
    if arr.ndim != 1:
        raise ValueError("histograms takes a 1-D array")
    ctx = arr.context
    if ctx is None:
        raise ValueError("ciphertext array without a context: pass one to Paillier.ciphertext_from")
    b = bins.to_numpy().T if hasattr(bins, "columns") else np.asarray(bins)
    if b.ndim != 2 or b.shape[1] != arr.size or b.shape[0] < 1:
        raise ValueError(f"histograms: bins must be [nfeat, {arr.size}]")
    if b.dtype.kind not in "iu":
        bf = b.astype(np.float64)
        ok = np.isfinite(bf)
        b = np.where(ok, bf, -1).astype(np.int64)
    ids = b.astype(np.int64)
    if nbins is None:
        nbins = max(1, int(ids.max()) + 1) if ids.size else 1
    nbins = int(nbins)
    if nbins < 1:
        raise ValueError("histograms: nbins must be positive")
    ids = np.where((ids < 0) | (ids >= nbins), -1, ids)
    if arr._has_na():
        ids[:, arr.isna()] = -1
    nfeat = ids.shape[0]
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        if rows.size and (rows.min() < 0 or rows.max() >= arr.size):
            raise IndexError("histograms: row index out of range")
    sel = ids if rows is None else ids[:, rows]
    try:
        used = arr.exponents if rows is None else arr.exponents[rows]
        used = used[used != NA_EXP]
        spread = int(used.max()) - int(used.min()) if used.size else 0
        if nbins > 4096 or (spread and (arr._has_na() or spread > ops.hist_exp_spread_max(ctx))):
            raise _Fallback()
        e0 = int(used[0]) if used.size else 0
        n2w = ops.n2w_of(ctx)
        x = arr._aligned_words(n2w)
        u16 = np.where(ids < 0, 0xFFFF, ids).astype(np.uint16)
        if spread:  # mixed exponents: the dense call that aligns them (xhe_hist_exp), whatever default_bin says
            ev = np.ascontiguousarray(arr.exponents, dtype=np.int32)
            dev = resident.device_for(ctx, -1, x.size, 4 * n2w)
            if dev is None:
                w, eo, cnt = ops.hist_exp_words(ctx, x.words, ev, u16, nbins, rows)
                return _result(ctx, w, eo, (nfeat, nbins)), cnt.astype(np.int64).reshape(nfeat, nbins)
            rd = None if rows is None else resident.upload_async(rows.astype(np.int32), dev)
            out, eo, cnt = resident.hist_exp(ctx.device_key(dev), x._dw(dev), resident.upload_async(ev, dev), spread,
                                             resident.upload(u16.view(np.int16), dev), nbins, rd)
            counts = resident.download(cnt, np.int32).astype(np.int64).reshape(nfeat, nbins)
            return PaillierArray.from_device(ctx, out, resident.download(eo, np.int32), (nfeat, nbins)), counts
        exps = np.full(nfeat * nbins, e0, dtype=np.int32)
        dev = resident.device_for(ctx, -1, x.size, 4 * n2w)
        count = arr.size if rows is None else rows.size
        zb = None
        if sparse is not False and nbins <= 4095 and count and not arr._has_na():
            zb = _zero_bins(default_bin, nfeat, nbins)
        if zb is not None:
            picked = u16 if rows is None else u16[:, rows]
            nnz = int(((picked != zb[:, None]) | (zb[:, None] == 0xFFFF)).sum())
            if not sparse and not ops.hist_sparse_route(ctx, ctx.own_device() if dev is None else dev, count, nfeat,
                                                        nbins, nnz, total is not None):
                zb = None
        tw = _total_row(ctx, total, e0, n2w) if zb is not None and total is not None else None
        if dev is None:
            if zb is not None:
                w, cnt = ops.hist_sparse_words(ctx, x.words, u16, nbins, zb, rows, tw)
            else:
                w, cnt = ops.hist_words(ctx, x.words, u16, nbins, rows)
            return _result(ctx, w, exps, (nfeat, nbins)), cnt.astype(np.int64).reshape(nfeat, nbins)
        rd = None if rows is None else resident.upload_async(rows.astype(np.int32), dev)
        bd = resident.upload(u16.view(np.int16), dev)
        if zb is not None:
            out, cnt = resident.hist_sparse(ctx.device_key(dev), x._dw(dev), bd, nbins,
                                            resident.upload_async(zb.view(np.int16), dev), nnz, rd,
                                            None if tw is None else resident.upload_async(tw, dev))
        else:
            out, cnt = resident.hist(ctx.device_key(dev), x._dw(dev), bd, nbins, rd)
        counts = resident.download(cnt, np.int32).astype(np.int64).reshape(nfeat, nbins)
        return PaillierArray.from_device(ctx, out, exps, (nfeat, nbins)), counts
    except _Fallback:
        sub = arr if rows is None else arr.take(rows)
        parts = [sub._groupby_op(how="sum", has_dropped_na=True, min_count=0, ngroups=nbins, ids=sel[f])
                 for f in range(nfeat)]
        counts = np.stack([np.bincount(sel[f][sel[f] >= 0], minlength=nbins) for f in range(nfeat)]).astype(np.int64)
        return PaillierArray._concat_same_type(parts).reshape((nfeat, nbins)), counts


def _level_parent_ok(ctx, parent, subtract, shape, e0):
    """whether `parent` can serve a subtraction for a level of `shape` (the planner aside)"""
    from .paillier.array import PaillierArray
    nnodes, nfeat, nbins = shape
    if parent is None or subtract is False or nnodes % 2:
        return False
    sums, counts = parent
    pshape = (nnodes // 2, nfeat, nbins)
    if not isinstance(sums, PaillierArray) or sums.context is not ctx or sums.shape != pshape or \
            np.shape(counts) != pshape:
        return False
    pe = sums.exponents
    return int(pe.min()) == e0 and int(pe.max()) == e0


def _level_subtracts(ctx, dev, parent, subtract, n_rows, shape, e0):
    """whether level_histograms takes the subtraction path on device `dev`"""
    from .paillier import ops
    if not _level_parent_ok(ctx, parent, subtract, shape, e0):
        return False
    return True if subtract else ops.hist_level_sub_route(ctx, dev, n_rows, *shape)


def _total_rows(ctx, total, nnodes, e0, n2w):
    """the [nnodes, n2w] host words of `total` (a PaillierArray of nnodes ciphertexts) at exponent e0"""
    from .paillier.array import PaillierArray
    if not isinstance(total, PaillierArray) or total.size != nnodes or total._has_na():
        raise ValueError("level_histograms: total must be a PaillierArray of nnodes ciphertexts")
    if int(total.exponents.min()) != e0 or int(total.exponents.max()) != e0:
        raise ValueError("level_histograms: total must be at the column's exponent")
    return np.array(total.reshape(-1)._aligned_words(n2w).words, dtype=np.uint32).reshape(nnodes, n2w)


def level_histograms(arr, bins, nodes, nnodes: int = None, nbins: int = None, parent=None, subtract: bool = None,
                     default_bin=None, total=None, sparse: bool = None):
    """histograms() for every node of a tree level in ONE device call
    (xhe_hist_level): what a level-wise trainer's loop of
    histograms(arr, bins, rows=<the node's samples>) over the level's nodes
    computes (xgb_actor.py cal_hist_for_node, run for all nodes of a level).
    arr, bins, nbins: as histograms. nodes: one level-local node slot per
    element of arr; a negative or NaN slot, or one >= nnodes, leaves the row out
    of every node (a finished leaf, an unsampled row). nnodes defaults to the
    largest slot + 1. Returns (sums, counts): sums a PaillierArray of shape
    (nnodes, nfeat, nbins) at the column's exponent, in HBM when the input is;
    counts an int64 array of that shape. Needs only the public key.

    parent: the (sums, counts) a level_histograms call returned for the level
    above, whose slot v split into this level's slots 2v and 2v + 1 (every row
    of slot v, and no other, now sits in one of the two, under the same bins).
    With it the device builds only the smaller child of every pair from its
    rows and takes the sibling as parent / built per (feature, bin)
    (xhe_hist_level_sub: histogram subtraction, about half the products); the
    result is bit for bit the direct one. subtract: None = the library's planner
    decides, True = always, False = never. The subtraction needs a resident
    column, an even nnodes and a parent of shape (nnodes / 2, nfeat, nbins) at
    the column's exponent; in every other case the direct call runs. It
    synchronises the stream once.

    default_bin, sparse: as histograms - the rows in a feature's default bin
    are not multiplied; per node the bin is what is left of the node's product
    (xhe_hist_level_sparse), the same ciphertexts bit for bit. total: those
    per-node products, a PaillierArray of nnodes ciphertexts at the column's
    exponent (the level above has them in any feature's bins), else they are
    computed. sparse=None asks the planner with the entries outside the default
    bins counted from `bins`. With a parent that qualifies and a default bin
    the two savings combine in one call (xhe_hist_level_sub_sparse: only the
    smaller child's entries outside the default bins are multiplied) when
    subtract and sparse are both True, or when neither is False and the
    planner expects that call to beat both others; otherwise the subtraction,
    where it is taken, runs without the default bins. More than 4095 bins keep
    the dense path.
    Raises ZeroDivisionError when a product that has to be inverted is no unit
    mod n^2 (never for ciphertexts of this key).

    The device path serves one exponent, nbins <= 4096 and nnodes <= 4096;
    anything else is the loop of histograms(rows=...) per node."""
    from .paillier import PaillierCiphertext, ops, resident
    from .paillier.array import NA_EXP, PaillierArray, _Fallback, _result
    if isinstance(arr, np.ndarray) and arr.dtype == object and arr.ndim == 1 and \
            all(isinstance(c, PaillierCiphertext) for c in arr):
        arr = PaillierArray(arr)
    if not isinstance(arr, PaillierArray):
        raise TypeError("level_histograms takes a PaillierArray or an object array of PaillierCiphertext")
    if arr.ndim != 1:
        raise ValueError("level_histograms takes a 1-D array")
    ctx = arr.context
    if ctx is None:
        raise ValueError("ciphertext array without a context: pass one to Paillier.ciphertext_from")

    def ints(a):  # negative for NaN / non-finite
        a = np.asarray(a)
        if a.dtype.kind in "iu":
            return a.astype(np.int64)
        af = a.astype(np.float64)
        return np.where(np.isfinite(af), af, -1).astype(np.int64)
    ids = ints(bins.to_numpy().T if hasattr(bins, "columns") else bins)
    if ids.ndim != 2 or ids.shape[1] != arr.size or ids.shape[0] < 1:
        raise ValueError(f"level_histograms: bins must be [nfeat, {arr.size}]")
    nd = ints(nodes).reshape(-1)
    if nd.shape[0] != arr.size:
        raise ValueError(f"level_histograms: nodes must have {arr.size} entries")
    if nbins is None:
        nbins = max(1, int(ids.max()) + 1) if ids.size else 1
    if nnodes is None:
        nnodes = max(1, int(nd.max()) + 1) if nd.size else 1
    nbins, nnodes = int(nbins), int(nnodes)
    if nbins < 1 or nnodes < 1:
        raise ValueError("level_histograms: nbins and nnodes must be positive")
    ids = np.where((ids < 0) | (ids >= nbins), -1, ids)
    nd = np.where((nd < 0) | (nd >= nnodes), -1, nd)
    if arr._has_na():
        nd[arr.isna()] = -1
    nfeat = ids.shape[0]
    shape = (nnodes, nfeat, nbins)
    try:
        used = arr.exponents[nd >= 0]
        used = used[used != NA_EXP]
        if nbins > 4096 or nnodes > 4096 or (used.size and int(used.min()) != int(used.max())):
            raise _Fallback()
        e0 = int(used[0]) if used.size else 0
        n2w = ops.n2w_of(ctx)
        x = arr._aligned_words(n2w)
        b16 = np.where(ids < 0, 0xFFFF, ids).astype(np.uint16)
        n16 = np.where(nd < 0, 0xFFFF, nd).astype(np.uint16)
        exps = np.full(nnodes * nfeat * nbins, e0, dtype=np.int32)
        dev = resident.device_for(ctx, -1, x.size, 4 * n2w)
        # (the planner takes the combined call for 2 to 64 nodes only: no entry is counted for a level it cannot take)
        if dev is not None and sparse is not False and nbins <= 4095 and arr.size and default_bin is not None and \
                ((subtract and sparse) or nnodes <= 64) and _level_parent_ok(ctx, parent, subtract, shape, e0):
            zb = _zero_bins(default_bin, nfeat, nbins)
            if zb is not None:  # both savings in one call
                live = b16[:, n16 != 0xFFFF]
                nnz = int(((live != zb[:, None]) | (zb[:, None] == 0xFFFF)).sum())
                if (subtract and sparse) or ops.hist_level_sub_sparse_route(ctx, dev, arr.size, nnodes, nfeat, nbins,
                                                                            nnz, total is not None):
                    tw = None if total is None else resident.upload_async(_total_rows(ctx, total, nnodes, e0, n2w), dev)
                    out, cnt = resident.hist_level_sub_sparse(
                        ctx.device_key(dev), x._dw(dev), resident.upload(b16.view(np.int16), dev), nbins,
                        resident.upload(n16.view(np.int16), dev), nnodes, resident.upload_async(zb.view(np.int16), dev),
                        nnz, parent[0]._dw(dev),
                        resident.upload(np.ascontiguousarray(parent[1], np.int32).reshape(-1), dev), tw)
                    counts = resident.download(cnt, np.int32).astype(np.int64).reshape(shape)
                    return PaillierArray.from_device(ctx, out, exps, shape), counts
        subtracts = dev is not None and _level_subtracts(ctx, dev, parent, subtract, arr.size, shape, e0)
        zb = None
        if sparse is not False and nbins <= 4095 and arr.size and not subtracts:
            zb = _zero_bins(default_bin, nfeat, nbins)
        if zb is not None:
            live = b16[:, n16 != 0xFFFF]
            nnz = int(((live != zb[:, None]) | (zb[:, None] == 0xFFFF)).sum())
            if not sparse and not ops.hist_level_sparse_route(ctx, ctx.own_device() if dev is None else dev, arr.size,
                                                              nnodes, nfeat, nbins, nnz, total is not None):
                zb = None
        tw = _total_rows(ctx, total, nnodes, e0, n2w) if zb is not None and total is not None else None
        if dev is None:
            if zb is not None:
                w, cnt = ops.hist_level_sparse_words(ctx, x.words, b16, nbins, n16, nnodes, zb, tw)
            else:
                w, cnt = ops.hist_level_words(ctx, x.words, b16, nbins, n16, nnodes)
            return _result(ctx, w, exps, shape), cnt.astype(np.int64).reshape(shape)
        bd, ndv = resident.upload(b16.view(np.int16), dev), resident.upload(n16.view(np.int16), dev)
        if zb is not None:
            out, cnt = resident.hist_level_sparse(ctx.device_key(dev), x._dw(dev), bd, nbins, ndv, nnodes,
                                                  resident.upload_async(zb.view(np.int16), dev), nnz,
                                                  None if tw is None else resident.upload_async(tw, dev))
        elif subtracts:
            out, cnt = resident.hist_level_sub(ctx.device_key(dev), x._dw(dev), bd, nbins, ndv, nnodes,
                                               parent[0]._dw(dev),
                                               resident.upload(np.ascontiguousarray(parent[1], np.int32).reshape(-1),
                                                               dev))
        else:
            out, cnt = resident.hist_level(ctx.device_key(dev), x._dw(dev), bd, nbins, ndv, nnodes)
        counts = resident.download(cnt, np.int32).astype(np.int64).reshape(shape)
        return PaillierArray.from_device(ctx, out, exps, shape), counts
    except _Fallback:
        per = [histograms(arr, ids, nbins=nbins, rows=np.flatnonzero(nd == v)) for v in range(nnodes)]
        sums = PaillierArray._concat_same_type([s.reshape(-1) for s, _ in per]).reshape(shape)
        return sums, np.stack([c for _, c in per])


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
