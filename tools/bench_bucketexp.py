"""Bucket multi-exponentiation (xhe_bucketexp) next to the route it replaces
for tall dense products - the gather and xhe_invert of the bases some negative
scalar multiplies plus xhe_multiexp on bases and inverses, timed together, as a
caller pays them - on the 2048-bit key:

  pearson_100k   100 000 terms x 16 columns, signed 24-bit scalars
  pearson_1m   1 000 000 terms x 16 columns, signed 24-bit scalars
  lr_step            2 048 terms x 15 columns, signed 60-bit scalars
  floor_24 / _60     8 197 terms x 2 columns at 24 and 60 bits (the planner's
                     floor, paths.hpp kBucketMinTerms)

Both routes run on device buffers uploaded before the timer; the outputs are
compared word for word before anything is timed. Device events around
synchronised calls, one warm-up each, the two routes alternating, median /
fastest / slowest of --reps. One JSON file under --out.

    python tools/bench_bucketexp.py [--reps 5] [--shapes a,b] [--out profiles/r25/bucketexp]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"lr_step": (2048, 15, 60), "floor_24": (8197, 2, 24), "floor_60": (8197, 2, 60),
          "pearson_100k": (100_000, 16, 24), "pearson_1m": (1_000_000, 16, 24)}


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def alternate(fa, fb, reps):
    """device-event ms of fa() and fb(), alternating, after one warm-up of each"""
    import torch
    out = ([], [])
    for r in range(reps + 1):
        for which, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r:
                out[which].append(a.elapsed_time(b))
    return stats(out[0]), stats(out[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25", "bucketexp"))
    args = ap.parse_args()
    import torch

    from bench import make_key
    from xfl_amd import _native as nat
    L = nat.lib()
    p, q, n, h = make_key(2048, seed=2024)
    dk = nat.DeviceKey(2048, n, p, q, h, device=0, win_bits=16)
    s = torch.cuda.current_stream().cuda_stream
    S = 100_000
    rng = np.random.default_rng(25)
    mw = nat.ints_to_words([int(v) for v in rng.integers(0, 1 << 40, S)], dk.nw)
    mdev = torch.from_numpy(mw.view(np.int32)).cuda()
    rnd = torch.empty((S, dk.rand_words), dtype=torch.int32, device="cuda")
    ct = torch.empty((S, dk.n2w), dtype=torch.int32, device="cuda")
    nat.check(L.xhe_rand(dk.handle, b"\x19" * 32, 5, S, rnd.data_ptr(), None, s), "rand")
    nat.check(L.xhe_encrypt(dk.handle, mdev.data_ptr(), rnd.data_ptr(), S, ct.data_ptr(), s), "encrypt")
    torch.cuda.synchronize()
    del rnd, mdev
    rec = {"key_bits": 2048, "reps": args.reps, "shapes": {}}
    for name in args.shapes.split(","):
        nterms, ncols, kbits = SHAPES[name]
        bases = (ct.repeat(-(-nterms // S), 1) if nterms > S else ct)[:nterms].contiguous()
        kw = (kbits + 31) // 32
        k = rng.integers(1, 1 << kbits, (ncols, nterms), dtype=np.uint64)
        kwords = np.stack([(k >> np.uint64(32 * i)).astype(np.uint32) for i in range(kw)], axis=-1)
        neg = rng.integers(0, 2, (ncols, nterms)).astype(np.uint8)
        kd = torch.from_numpy(np.ascontiguousarray(kwords).view(np.int32)).cuda()
        nd = torch.from_numpy(neg).cuda()
        # the parent's plan (_matmul_plan): the bases some negative scalar multiplies are inverted and
        # appended; a term takes base t or that inverse
        need = np.nonzero(neg.any(axis=0))[0]
        slot = np.zeros(nterms, np.int64)
        slot[need] = nterms + np.arange(need.size)
        idx = np.where(neg != 0, slot[None, :], np.arange(nterms)[None, :]).astype(np.int32)
        idd = torch.from_numpy(np.ascontiguousarray(idx)).cuda()
        need_d = torch.from_numpy(need).cuda()
        ninv = int(need.size)
        both = torch.empty((nterms + ninv, dk.n2w), dtype=torch.int32, device="cuda")
        both[:nterms] = bases
        picked = torch.empty((ninv, dk.n2w), dtype=torch.int32, device="cuda")
        out_b = torch.empty((ncols, dk.n2w), dtype=torch.int32, device="cuda")
        out_s = torch.empty((ncols, dk.n2w), dtype=torch.int32, device="cuda")

        def buckets():
            nat.check(L.xhe_bucketexp(dk.handle, bases.data_ptr(), nterms, kd.data_ptr(), nd.data_ptr(), kw, kbits,
                                      ncols, 0, out_b.data_ptr(), s), "bucketexp")

        def straus():
            nat.check(L.xhe_gather_rows(bases.data_ptr(), need_d.data_ptr(), ninv, dk.n2w, picked.data_ptr(), s), "take")
            nat.check(L.xhe_invert(dk.handle, picked.data_ptr(), ninv, both[nterms:].data_ptr(), s), "invert")
            nat.check(L.xhe_multiexp(dk.handle, both.data_ptr(), nterms + ninv, idd.data_ptr(), kd.data_ptr(), kw,
                                     kbits, ncols, nterms, 0, out_s.data_ptr(), s), "multiexp")
        buckets()
        straus()
        torch.cuda.synchronize()
        r = {"nterms": nterms, "ncols": ncols, "kbits": kbits, "ninv": ninv,
             "equal_word_for_word": bool(torch.equal(out_b, out_s)),
             "planner_route": "buckets" if L.xhe_multiexp_route(dk.handle, nterms, ncols, kbits, ninv) == 1
             else "straus"}
        if r["equal_word_for_word"]:
            r["buckets"], r["invert_plus_multiexp"] = alternate(buckets, straus, args.reps if nterms < 500_000 else 3)
            # faster by more than the spread of either: the slowest bucket run under the fastest Straus run
            r["buckets_faster_beyond_spread"] = r["buckets"]["max_ms"] < r["invert_plus_multiexp"]["min_ms"]
            r["straus_faster_beyond_spread"] = r["invert_plus_multiexp"]["max_ms"] < r["buckets"]["min_ms"]
            L.xhe_profile(1)
            buckets()
            torch.cuda.synchronize()
            ms, cnt = ctypes.c_double(), ctypes.c_int64()
            for kn in ("k_bucketexp", "k_hist_tile", "k_bucket_fold", "k_mexp_horner"):
                L.xhe_profile_read(kn.encode(), ctypes.byref(ms), ctypes.byref(cnt))
                r[f"profile_{kn}_ms"] = ms.value
            L.xhe_profile(0)
        rec["shapes"][name] = r
        print(name, json.dumps(r), flush=True)
        del bases, both, kd, nd, idd, need_d, picked
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bucketexp_2048.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
