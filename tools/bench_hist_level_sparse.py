"""The level-wise sparse histogram (xhe_hist_level_sparse) next to the dense
level call (xhe_hist_level) in one process, on config 5's key and shape (100 k
samples x 64 features x 256 bins, 2048 bits, resident column, the seeded
ciphertexts of tools/bench_hist.py) at 2, 16 and 64 uniformly drawn nodes. Bin
0 is every feature's zero bin; a fraction d of each feature's rows is drawn
into the other bins, d = 0.05, 0.2, 0.5, each with and without the per-node
totals (the dense call's products of feature 0's bins, resident before the
timed calls). The two are timed alternately: device events around synchronised
calls, two warm-ups, median / fastest / slowest of --reps
(tools/bench_hist.py's timed). Outputs and counts are compared bit for bit; the
stage times of one profiled call. One JSON line per (nnodes, d, totals), all of
them in --out/hist_level_sparse_2048.jsonl, or hist_level_sparse_2048_<tag>.jsonl
with --tag, so that a further run does not overwrite the main table.

    python tools/bench_hist_level_sparse.py [--reps 5] [--nodes 2,16,64] [--density 0.05,0.2,0.5] [--tag TAG]
                                            [--out profiles/r29/hist_level_sparse]
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

STAGES = ("k_hist_level_sparse", "k_lsp_order", "k_lsp_totals", "k_lsp_tile", "k_lsp_fold", "k_lsp_zero")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nodes", default="2,16,64")
    ap.add_argument("--density", default="0.05,0.2,0.5")
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29", "hist_level_sparse"))
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
    fname = "hist_level_sparse_2048" + ("_" + args.tag if args.tag else "") + ".jsonl"
    with open(os.path.join(args.out, fname), "w") as f:
        for NN in [int(v) for v in args.nodes.split(",")]:
            a_out = torch.empty((NN * F * NB, dk.n2w), dtype=torch.int32, device="cuda")
            a_cnt = torch.empty(NN * F * NB, dtype=torch.int32, device="cuda")
            b_out, b_cnt = torch.empty_like(a_out), torch.empty_like(a_cnt)
            tot = torch.empty((NN, dk.n2w), dtype=torch.int32, device="cuda")
            nd = torch.from_numpy(np.random.default_rng(NN).integers(0, NN, S).astype(np.int16)).cuda()
            for d in [float(v) for v in args.density.split(",")]:
                g = np.random.default_rng(2000 + int(d * 1000))
                bins = np.where(g.random((F, S)) < d, g.integers(1, NB, (F, S)), 0).astype(np.uint16)
                nnz = int((bins != 0).sum())
                bd = torch.from_numpy(bins.view(np.int16)).cuda()

                def dense():
                    nat.check(L.xhe_hist_level(dk.handle, ct.data_ptr(), S, bd.data_ptr(), S, F, NB, nd.data_ptr(), NN, 0,
                                               a_out.data_ptr(), a_cnt.data_ptr(), s), "hist_level")
                dense()
                # total[v]: the product of (v, feature 0)'s bins, as a trainer takes it from the level above
                torch.cuda.synchronize()
                src = a_out.view(NN, F * NB, dk.n2w)[:, :NB].contiguous()
                seg = np.arange(NN + 1, dtype=np.int64) * NB
                nat.check(L.xhe_segprod(dk.handle, src.data_ptr(), None, 0, NN * NB, seg.ctypes.data_as(ctypes.c_void_p),
                                        NN, tot.data_ptr(), s), "segprod")
                torch.cuda.synchronize()
                for have_total in (False, True):
                    def sparse():
                        nat.check(L.xhe_hist_level_sparse(dk.handle, ct.data_ptr(), S, bd.data_ptr(), S, F, NB,
                                                          zd.data_ptr(), nd.data_ptr(), NN, nnz,
                                                          tot.data_ptr() if have_total else None, 0, b_out.data_ptr(),
                                                          b_cnt.data_ptr(), s), "hist_level_sparse")
                    # alternating: a drift of the machine falls on both
                    a1, b1, a2, b2 = (timed(fn, args.reps) for fn in (dense, sparse, dense, sparse))
                    rec = {"rows": S, "nfeat": F, "nbins": NB, "nnodes": NN, "density": d, "nnz": nnz,
                           "have_total": have_total, "reps": args.reps, "a_dense": a1, "b_sparse": b1,
                           "a_dense_again": a2, "b_sparse_again": b2,
                           "routed": int(L.xhe_hist_level_sparse_route(dk.handle, S, NN, F, NB, nnz, int(have_total)))}
                    rec["b_equals_a_bit_for_bit"] = bool(torch.equal(a_out, b_out) and torch.equal(a_cnt, b_cnt))
                    L.xhe_profile(1)
                    sparse()
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


if __name__ == "__main__":
    main()
