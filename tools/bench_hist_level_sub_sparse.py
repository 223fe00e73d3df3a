"""Subtraction on the sparse level histogram (xhe_hist_level_sub_sparse) next
to its two alternatives, xhe_hist_level_sparse and xhe_hist_level_sub, in one
process, on config 5's key and shape (100 k samples x 64 features x 256 bins,
2048 bits, resident column, the seeded ciphertexts of tools/bench_hist.py) at 2,
16 and 64 nodes. Bin 0 is every feature's zero bin; a fraction d of each
feature's rows is drawn into the other bins. The node of a row is drawn
uniformly (the two children of a pair about equal), or with --skew S the right
child of every pair gets the share S of the pair's rows. The parent is the dense
level call on node >> 1, the totals the dense call's products of feature 0's
bins, both resident before the timed calls. The three calls are timed
alternately: device events around synchronised calls, two warm-ups, median /
fastest / slowest of --reps (tools/bench_hist.py's timed). Every timed call's
outputs and counts are compared bit for bit with xhe_hist_level's; the stage
times of one profiled combined call. One JSON line per (nnodes, d, totals) in
--out/hist_level_sub_sparse_2048.jsonl, or ..._<tag>.jsonl with --tag.

    python tools/bench_hist_level_sub_sparse.py [--reps 5] [--nodes 2,16,64] [--density 0.05,0.2,0.5,0.8]
                                                [--skew 0.9] [--tag TAG] [--out profiles/r30/hist_level_sub_sparse]
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

STAGES = ("k_hist_level_sub_sparse", "k_sub_pick", "k_lsp_order", "k_sss_totals", "k_lsp_tile", "k_lsp_fold",
          "k_sss_mark", "k_sss_fwd", "k_sss_bwd", "k_sss_zero")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nodes", default="2,16,64")
    ap.add_argument("--density", default="0.05,0.2,0.5,0.8")
    ap.add_argument("--skew", type=float, default=0.0)
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30", "hist_level_sub_sparse"))
    args = ap.parse_args()
    import torch

    from bench import make_key
    from bench_hist import timed
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
    mw = nat.ints_to_words([int(v) % n for v in embed([pr - y, pr * (1.0 - pr)])], dk.nw)
    mdev = torch.from_numpy(mw.view(np.int32)).cuda()
    rnd = torch.empty((S, dk.rand_words), dtype=torch.int32, device="cuda")
    ct = torch.empty((S, dk.n2w), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    nat.check(L.xhe_rand(dk.handle, b"\x05" * 32, 3, S, rnd.data_ptr(), None, s), "rand")
    nat.check(L.xhe_encrypt(dk.handle, mdev.data_ptr(), rnd.data_ptr(), S, ct.data_ptr(), s), "encrypt")
    torch.cuda.synchronize()
    del rnd, mdev
    zd = torch.zeros(F, dtype=torch.int16, device="cuda")

    os.makedirs(args.out, exist_ok=True)
    fname = "hist_level_sub_sparse_2048" + ("_" + args.tag if args.tag else "") + ".jsonl"
    with open(os.path.join(args.out, fname), "w") as f:
        for NN in [int(v) for v in args.nodes.split(",")]:
            want = torch.empty((NN * F * NB, dk.n2w), dtype=torch.int32, device="cuda")
            want_cnt = torch.empty(NN * F * NB, dtype=torch.int32, device="cuda")
            outs = {k: (torch.empty_like(want), torch.empty_like(want_cnt)) for k in ("sparse", "sub", "both")}
            par = torch.empty((NN // 2 * F * NB, dk.n2w), dtype=torch.int32, device="cuda")
            par_cnt = torch.empty(NN // 2 * F * NB, dtype=torch.int32, device="cuda")
            tot = torch.empty((NN, dk.n2w), dtype=torch.int32, device="cuda")
            g = np.random.default_rng(NN)
            node = g.integers(0, NN, S)
            if args.skew:
                node = (node & ~1) | (g.random(S) < args.skew)
            nd = torch.from_numpy(node.astype(np.int16)).cuda()
            pd = torch.from_numpy((node >> 1).astype(np.int16)).cuda()
            for d in [float(v) for v in args.density.split(",")]:
                g = np.random.default_rng(2000 + int(d * 1000))
                bins = np.where(g.random((F, S)) < d, g.integers(1, NB, (F, S)), 0).astype(np.uint16)
                nnz = int((bins != 0).sum())
                bd = torch.from_numpy(bins.view(np.int16)).cuda()
                nat.check(L.xhe_hist_level(dk.handle, ct.data_ptr(), S, bd.data_ptr(), S, F, NB, nd.data_ptr(), NN, 0,
                                           want.data_ptr(), want_cnt.data_ptr(), s), "hist_level")
                nat.check(L.xhe_hist_level(dk.handle, ct.data_ptr(), S, bd.data_ptr(), S, F, NB, pd.data_ptr(), NN // 2, 0,
                                           par.data_ptr(), par_cnt.data_ptr(), s), "hist_level")
                # total[v]: the product of (v, feature 0)'s bins, as a trainer takes it from the level above
                torch.cuda.synchronize()
                src = want.view(NN, F * NB, dk.n2w)[:, :NB].contiguous()
                seg = np.arange(NN + 1, dtype=np.int64) * NB
                nat.check(L.xhe_segprod(dk.handle, src.data_ptr(), None, 0, NN * NB, seg.ctypes.data_as(ctypes.c_void_p),
                                        NN, tot.data_ptr(), s), "segprod")
                torch.cuda.synchronize()
                for have_total in (False, True):
                    tp = tot.data_ptr() if have_total else None

                    def sparse():
                        o, c = outs["sparse"]
                        nat.check(L.xhe_hist_level_sparse(dk.handle, ct.data_ptr(), S, bd.data_ptr(), S, F, NB,
                                                          zd.data_ptr(), nd.data_ptr(), NN, nnz, tp, 0, o.data_ptr(),
                                                          c.data_ptr(), s), "hist_level_sparse")

                    def sub():
                        o, c = outs["sub"]
                        nat.check(L.xhe_hist_level_sub(dk.handle, ct.data_ptr(), S, bd.data_ptr(), S, F, NB, nd.data_ptr(),
                                                       NN, par.data_ptr(), par_cnt.data_ptr(), 0, o.data_ptr(),
                                                       c.data_ptr(), s), "hist_level_sub")

                    def both():
                        o, c = outs["both"]
                        nat.check(L.xhe_hist_level_sub_sparse(dk.handle, ct.data_ptr(), S, bd.data_ptr(), S, F, NB,
                                                              zd.data_ptr(), nd.data_ptr(), NN, par.data_ptr(),
                                                              par_cnt.data_ptr(), nnz, tp, 0, o.data_ptr(), c.data_ptr(),
                                                              s), "hist_level_sub_sparse")
                    # alternating: a drift of the machine falls on all three
                    fns = (("sparse", sparse), ("sub", sub), ("both", both))
                    rec = {"rows": S, "nfeat": F, "nbins": NB, "nnodes": NN, "density": d, "nnz": nnz, "skew": args.skew,
                           "have_total": have_total, "reps": args.reps,
                           "routed": int(L.xhe_hist_level_sub_sparse_route(dk.handle, S, NN, F, NB, nnz,
                                                                           int(have_total)))}
                    for rnd_ in ("", "_again"):
                        for name, fn in fns:
                            rec[name + rnd_] = timed(fn, args.reps)
                    for name, (o, c) in outs.items():
                        rec[name + "_equals_level_bit_for_bit"] = bool(torch.equal(o, want) and torch.equal(c, want_cnt))
                    L.xhe_profile(1)
                    both()
                    torch.cuda.synchronize()
                    ms, k = ctypes.c_double(), ctypes.c_int64()
                    for name in STAGES:
                        L.xhe_profile_read(name.encode(), ctypes.byref(ms), ctypes.byref(k))
                        rec[f"profile_{name}_ms"] = ms.value
                    L.xhe_profile(0)
                    best = {name: min(rec[name]["median_ms"], rec[name + "_again"]["median_ms"]) for name, _ in fns}
                    rec["both_over_sparse"] = best["both"] / best["sparse"]
                    rec["both_over_sub"] = best["both"] / best["sub"]
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
