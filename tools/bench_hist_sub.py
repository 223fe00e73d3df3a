"""Histogram subtraction (xhe_hist_level_sub) next to the direct level call
(xhe_hist_level) in one process, on config 5's key and data (100 k samples x
64 features x 256 bins, 2048 bits, the seeded data of tools/bench_hist.py), at
nnodes = 2, 4, 8, 16, 32, 64, each with balanced children and with a 90 / 10
split of every pair. The parent histogram (the direct call on node >> 1) is
resident before the timed calls. The two are timed alternately: device events
around synchronised calls, two warm-ups, median / fastest / slowest of --reps
(tools/bench_hist.py's timed). Outputs and counts are compared bit for bit;
peak extra device memory of both; the stage times of one profiled call. One
JSON line per shape, all of them in --out/hist_sub_2048.jsonl.

    python tools/bench_hist_sub.py [--reps 5] [--nodes 2,4,8,16,32,64] [--out profiles/r27/hist_sub]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

STAGES = ("k_hist_level_sub", "k_sub_pick", "k_level_order", "k_level_tile", "k_level_fold", "k_sib_fwd", "k_sib_bwd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nodes", default="2,4,8,16,32,64")
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27", "hist_sub"))
    args = ap.parse_args()
    import torch

    from bench import make_key
    from bench_hist import peak_extra_bytes, timed
    from xfl_amd import _native as nat
    from xfl_amd.paillier_acceleration import embed
    L = nat.lib()
    p, q, n, h = make_key(2048, seed=2024)
    dk = nat.DeviceKey(2048, n, p, q, h, device=0, win_bits=16)
    S, F, NB = args.rows, 64, 256
    rng = np.random.default_rng(3)
    z = rng.standard_normal(S)
    y = (rng.random(S) < 0.5).astype(np.float64)
    pr = 1.0 / (1.0 + np.exp(-z))
    bins = np.stack([np.random.default_rng(4 + f).integers(0, NB, S) for f in range(F)]).astype(np.uint16)
    mw = nat.ints_to_words([int(v) % n for v in embed([pr - y, pr * (1.0 - pr)])], dk.nw)
    mdev = torch.from_numpy(mw.view(np.int32)).cuda()
    rnd = torch.empty((S, dk.rand_words), dtype=torch.int32, device="cuda")
    ct = torch.empty((S, dk.n2w), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    nat.check(L.xhe_rand(dk.handle, b"\x05" * 32, 3, S, rnd.data_ptr(), None, s), "rand")
    nat.check(L.xhe_encrypt(dk.handle, mdev.data_ptr(), rnd.data_ptr(), S, ct.data_ptr(), s), "encrypt")
    torch.cuda.synchronize()
    del rnd, mdev
    bd = torch.from_numpy(bins.view(np.int16)).cuda()

    def direct(nd, nn, out, cnt):
        nat.check(L.xhe_hist_level(dk.handle, ct.data_ptr(), S, bd.data_ptr(), S, F, NB, nd.data_ptr(), nn, 0,
                                   out.data_ptr(), cnt.data_ptr(), s), "hist_level")

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "hist_sub_2048.jsonl"), "w") as f:
        for nn in [int(v) for v in args.nodes.split(",")]:
            for kind, right in (("balanced", 0.5), ("split_90_10", 0.1)):
                g = np.random.default_rng(1000 + nn)
                node = 2 * g.integers(0, nn // 2, S) + (g.random(S) < right)
                nd = torch.from_numpy(node.astype(np.uint16).view(np.int16)).cuda()
                pnd = torch.from_numpy((node >> 1).astype(np.uint16).view(np.int16)).cuda()
                per = F * NB
                par = torch.empty((nn // 2 * per, dk.n2w), dtype=torch.int32, device="cuda")
                pcnt = torch.empty(nn // 2 * per, dtype=torch.int32, device="cuda")
                direct(pnd, nn // 2, par, pcnt)
                a_out = torch.empty((nn * per, dk.n2w), dtype=torch.int32, device="cuda")
                a_cnt = torch.empty(nn * per, dtype=torch.int32, device="cuda")
                b_out, b_cnt = torch.empty_like(a_out), torch.empty_like(a_cnt)

                def level():
                    direct(nd, nn, a_out, a_cnt)

                def sub():
                    nat.check(L.xhe_hist_level_sub(dk.handle, ct.data_ptr(), S, bd.data_ptr(), S, F, NB, nd.data_ptr(),
                                                   nn, par.data_ptr(), pcnt.data_ptr(), 0, b_out.data_ptr(),
                                                   b_cnt.data_ptr(), s), "hist_level_sub")
                # alternating: a drift of the machine falls on both
                a1, b1, a2, b2 = (timed(fn, args.reps) for fn in (level, sub, level, sub))
                rec = {"rows": S, "nfeat": F, "nbins": NB, "nnodes": nn, "node_ids": kind, "reps": args.reps,
                       "a_level": a1, "b_sub": b1, "a_level_again": a2, "b_sub_again": b2,
                       "routed": int(L.xhe_hist_level_sub_route(dk.handle, S, nn, F, NB))}
                rec["a_peak_extra_bytes"] = peak_extra_bytes(level)
                rec["b_peak_extra_bytes"] = peak_extra_bytes(sub)
                rec["b_equals_a_bit_for_bit"] = bool(torch.equal(a_out, b_out) and torch.equal(a_cnt, b_cnt))
                L.xhe_profile(1)
                sub()
                torch.cuda.synchronize()
                ms, k = ctypes.c_double(), ctypes.c_int64()
                for name in STAGES:
                    L.xhe_profile_read(name.encode(), ctypes.byref(ms), ctypes.byref(k))
                    rec[f"b_profile_{name}_ms"] = ms.value
                L.xhe_profile(0)
                rec["b_over_a"] = min(b1["median_ms"], b2["median_ms"]) / min(a1["median_ms"], a2["median_ms"])
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)
                del par, pcnt, a_out, a_cnt, b_out, b_cnt


if __name__ == "__main__":
    main()
