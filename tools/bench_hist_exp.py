"""Histograms of a ciphertext column of mixed exponents on one GPU: xhe_hist_exp
next to its floor (xhe_hist on the same rows, which ignores the exponents:
spread 0 only) and next to the path such a column took before - the drop-in's
groupby sum feature by feature (a sort, a gather of the rows into bin order and
an xhe_segprod with a gap array, per feature).

Workload: `--rows` (100000) resident random residues of the 2048-bit golden
key x `--feat` (64) features x `--bins` (256) uniform bin ids, the rows'
exponents uniform in [0, spread] for every spread of `--spreads` (0,4,16,52).

Every timing is a host clock around one call plus torch.cuda.synchronize(),
the stream drained before it. hist_exp and hist alternate within a
repetition: two warm-ups, then the median of `--reps` (7). The groupby path
runs for seconds: one warm-up, then the median of `--groupby-reps` (3), and it
is checked once against the new call, words and exponents. histograms_s is the
drop-in end to end on the new route (uploads of the bin matrix and the
exponents and the download of the counts included).

    python tools/bench_hist_exp.py [--spreads 0,4,16,52] [--reps 7] [--out DIR]
"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--feat", type=int, default=64)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--spreads", default="0,4,16,52")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--groupby-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for the JSON record")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_hist_exp: no GPU")
    torch.cuda.init()
    from xfl_amd.paillier import PaillierArray, PaillierContext, resident
    from xfl_amd.paillier_acceleration import histograms
    with open(os.path.join(ROOT, "tests", "golden", "paillier_2048_djn.json")) as f:
        key = json.load(f)["key"]
    pub = PaillierContext().init(int(key["p"], 16), int(key["q"], 16), djn_h_pow_n=int(key["h_pow_n"], 16)).to_public()
    dev = resident.device_for(pub)
    dk = pub.device_key(dev)
    rng = np.random.default_rng(9)
    n, nfeat, nbins = args.rows, args.feat, args.bins
    w = rng.integers(0, 1 << 32, size=(n, dk.n2w), dtype=np.uint64).astype(np.uint32)
    w[:, dk.n2w - 1] &= 0x00FFFFFF  # below n^2
    cd = resident.upload(w, dev)
    ids = rng.integers(0, nbins, (nfeat, n))
    bd = resident.upload(ids.astype(np.uint16).view(np.int16), dev)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, res

    cases = []
    for spread in [int(s) for s in args.spreads.split(",")]:
        ev = rng.integers(0, spread + 1, n).astype(np.int32)
        if spread:
            ev[:2] = 0, spread
        ed = resident.upload(ev, dev)
        arr = PaillierArray.from_device(pub, cd, ev)

        def new():
            return resident.hist_exp(dk, cd, ed, spread, bd, nbins)

        def floor():
            return resident.hist(dk, cd, bd, nbins)

        def groupby():  # histograms()' path for such a column before xhe_hist_exp
            return PaillierArray._concat_same_type(
                [arr._groupby_op(how="sum", has_dropped_na=True, min_count=0, ngroups=nbins, ids=ids[f])
                 for f in range(nfeat)])

        tn, tf, th, tg = [], [], [], []
        for r in range(args.reps + 2):
            a, b = once(new)[0], once(floor)[0]
            c = once(lambda: histograms(arr, ids, nbins=nbins))[0]
            if r >= 2:
                tn.append(a)
                tf.append(b)
                th.append(c)
        rec = {"spread": spread, "xhe_hist_exp": _stats(tn), "xhe_hist": _stats(tf), "histograms": _stats(th)}
        if spread == 0:
            assert torch.equal(new()[0], floor()[0]), "xhe_hist_exp differs from xhe_hist at one exponent"
        else:
            for r in range(args.groupby_reps + 1):
                t, old = once(groupby)
                if r >= 1:
                    tg.append(t)
            out, eo, _ = new()
            assert np.array_equal(resident.download(out), np.asarray(old.words)) and \
                np.array_equal(resident.download(eo, np.int32), old.exponents), "xhe_hist_exp differs from the groupby"
            rec["groupby"] = _stats(tg)
            rec["groupby_over_hist_exp"] = rec["groupby"]["median_s"] / rec["xhe_hist_exp"]["median_s"]
        rec["bit_exact"] = True
        cases.append(rec)
    floor_s = next((c["xhe_hist"]["median_s"] for c in cases if c["spread"] == 0), None)
    for c in cases:
        c["hist_exp_over_floor"] = floor_s and c["xhe_hist_exp"]["median_s"] / floor_s
    rec = {"key_bits": 2048, "rows": n, "nfeat": nfeat, "nbins": nbins, "reps": args.reps, "warmups": 2,
           "groupby_reps": args.groupby_reps, "cases": cases}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "hist_exp.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
