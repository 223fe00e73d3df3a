"""Cumulative sums over ciphertext arrays on one GPU, through the drop-in API
(golden 2048-bit DJN key, public side; resident inputs):

  (a) histogram   config 5's histogram, `--runs` runs of `--bins` bins (64 x
                  256), scanned in one cumsum_segments call - against the
                  object left fold, which is what np.cumsum over a ciphertext
                  array ran before xhe_segscan (one PaillierCiphertext.__add__
                  per element on a downloaded array). The fold is timed on ONE
                  run of `--bins` elements, not on all of them, and the record
                  says so.
  (b) one segment np.cumsum of `--long` elements (1 M) in one segment, next to
                  the element-wise add of the same arrays in the same process
                  (add_per_s): the add is one product per element and the
                  yardstick a scan cannot beat.

Every timing is a pair of device events on the drop-in stream around one call
that is synchronised before and after; two warm-ups, then the median of
`--reps` (5). The kernels' own time comes from xhe_profile's "k_segscan".

    python tools/bench_cumsum.py [--runs 64] [--bins 256] [--long 1048576] [--reps 5] [--out DIR]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _stats(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "repeats_s": ts}


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "paillier_2048_djn.json")) as f:
        k = json.load(f)["key"]
    return int(k["p"], 16), int(k["q"], 16), int(k["h_pow_n"], 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=64)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--long", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="directory for the JSON record")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_cumsum: no GPU")
    torch.cuda.init()
    from xfl_amd import _native as nat
    from xfl_amd.paillier import PaillierArray, PaillierContext, resident
    from xfl_amd.paillier_acceleration import cumsum_segments
    p, q, h = _golden()
    pub = PaillierContext().init(p, q, djn_h_pow_n=h).to_public()
    dev = resident.device_for(pub)
    dk = pub.device_key(dev)
    L = nat.lib()
    rng = np.random.default_rng(9)

    def residues(count):
        """`count` resident ciphertext rows below n^2 at exponent 0 (the scan's time does not depend on the values)"""
        w = rng.integers(0, 1 << 32, size=(count, dk.n2w), dtype=np.uint64).astype(np.uint32)
        w[:, dk.n2w - 1] &= 0x0FFFFFFF
        return PaillierArray.from_device(pub, resident.upload(w, dev), np.zeros(count, dtype=np.int32))

    def timed(fn):
        """device events around synchronised calls: two warm-ups, then --reps"""
        ts = []
        s = resident.stream(dev)
        for r in range(args.reps + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(s)
            fn()
            b.record(s)
            torch.cuda.synchronize()
            if r >= 2:
                ts.append(a.elapsed_time(b) / 1e3)
        return ts

    def kernel_ms(fn):
        L.xhe_profile(1)
        fn()
        tot, cnt = ctypes.c_double(), ctypes.c_int64()
        nat.check(L.xhe_profile_read(b"k_segscan", ctypes.byref(tot), ctypes.byref(cnt)))
        L.xhe_profile(0)
        return tot.value, cnt.value

    # ---- (a)
    nb = args.runs * args.bins
    hist = residues(nb)
    lengths = [args.bins] * args.runs
    scan_a = lambda: cumsum_segments(hist, lengths)  # noqa: E731
    res = scan_a()
    assert res.is_resident and res.shape == (nb,)
    t_a = timed(scan_a)
    k_a, launches_a = kernel_ms(scan_a)
    one_run = hist[:args.bins]
    t0 = time.perf_counter()
    fold = np.cumsum(np.asarray(one_run))  # the object left fold: download, one __add__ per element
    fold_raw = [c.raw_ciphertext for c in fold]  # (the adds are deferred: reading the residues runs them)
    t_fold = time.perf_counter() - t0
    n2 = pub.n * pub.n
    same = [r % n2 for r in fold_raw] == [c.raw_ciphertext for c in res[:args.bins]]
    assert same, "the device scan differs from the object fold"
    case_a = {"runs": args.runs, "bins": args.bins, "elements": nb, "cumsum_segments": _stats(t_a),
              "k_segscan_ms": k_a, "k_segscan_labels": launches_a,
              "object_fold_one_run_s": t_fold, "object_fold_elements": args.bins,
              "object_fold_note": "timed once on ONE run of `bins` elements (wall clock; download and the residues' "
                                  "materialisation included); "
                                  "the whole histogram is `runs` such folds",
              "object_fold_whole_histogram_extrapolated_s": t_fold * args.runs, "bit_exact_first_run": bool(same)}
    del hist, res
    # ---- (b)
    n = args.long
    x, y = residues(n), residues(n)
    scan_b = lambda: np.cumsum(x)  # noqa: E731
    add_b = lambda: x + y  # noqa: E731
    assert scan_b().is_resident
    t_b, t_add = timed(scan_b), timed(add_b)
    k_b, _ = kernel_ms(scan_b)
    med = statistics.median
    case_b = {"elements": n, "cumsum": _stats(t_b), "k_segscan_ms": k_b, "cumsum_per_s": n / med(t_b),
              "add": _stats(t_add), "add_per_s": n / med(t_add), "cumsum_over_add": med(t_b) / med(t_add)}
    rec = {"key_bits": 2048, "reps": args.reps, "warmups": 2, "histogram": case_a, "one_segment": case_b}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "cumsum_2048.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
