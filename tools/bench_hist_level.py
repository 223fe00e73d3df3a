"""The level-wise histogram (xhe_hist_level) next to the loop it replaces, on
config 5's key and data (100 k samples x 64 features x 256 bins, 2048 bits,
the seeded data of tools/bench_hist.py):

  (a) the per-node loop: one row-id list and one xhe_hist call per node, with
      and without building the lists (torch.nonzero per node + int32 cast)
  (b) one xhe_hist_level call on the same rows

at nnodes = 1, 2, 8, 32, 64 with balanced random node ids and at 32 nodes with
one node holding 90 % of the rows; peak extra device memory of both. Device
events around synchronised calls, two warm-ups, median / fastest / slowest of
--reps (tools/bench_hist.py's timed). (b) is compared with (a) word for word.
One JSON line per shape, all of them in --out/hist_level_2048.jsonl.

    python tools/bench_hist_level.py [--reps 5] [--nodes 1,2,8,32,64] [--out profiles/r26/hist_level]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nodes", default="1,2,8,32,64")
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26", "hist_level"))
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

    shapes = [(int(v), "balanced") for v in args.nodes.split(",")] + [(32, "skewed_90")]
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "hist_level_2048.jsonl"), "w") as f:
        for nn, kind in shapes:
            g = np.random.default_rng(1000 + nn)
            node = g.integers(0, nn, S)
            if kind == "skewed_90":
                node = np.where(g.random(S) < 0.9, 0, g.integers(1, nn, S))
            nd = torch.from_numpy(node.astype(np.uint16).view(np.int16)).cuda()
            per = F * NB
            loop_out = torch.empty((nn * per, dk.n2w), dtype=torch.int32, device="cuda")
            loop_cnt = torch.empty(nn * per, dtype=torch.int32, device="cuda")
            out, cnt = torch.empty_like(loop_out), torch.empty_like(loop_cnt)
            st = {}

            def lists():
                st["rows"] = [torch.nonzero(nd == v).reshape(-1).to(torch.int32) for v in range(nn)]

            def loop():
                for v, r in enumerate(st["rows"]):
                    nat.check(L.xhe_hist(dk.handle, ct.data_ptr(), S, bd.data_ptr(), S, F, NB, r.data_ptr(),
                                         r.shape[0], 0, loop_out[v * per:].data_ptr(), loop_cnt[v * per:].data_ptr(),
                                         s), "hist")

            def lists_loop():
                lists()
                loop()

            def level():
                nat.check(L.xhe_hist_level(dk.handle, ct.data_ptr(), S, bd.data_ptr(), S, F, NB, nd.data_ptr(), nn, 0,
                                           out.data_ptr(), cnt.data_ptr(), s), "hist_level")
            lists()
            rec = {"rows": S, "nfeat": F, "nbins": NB, "nnodes": nn, "node_ids": kind, "reps": args.reps,
                   "a_loop": timed(loop, args.reps), "a_loop_with_lists": timed(lists_loop, args.reps),
                   "b_level": timed(level, args.reps)}
            rec["a_peak_extra_bytes"] = peak_extra_bytes(loop)
            rec["b_peak_extra_bytes"] = peak_extra_bytes(level)
            rec["b_equals_a_bit_for_bit"] = bool(torch.equal(out, loop_out) and torch.equal(cnt, loop_cnt))
            L.xhe_profile(1)
            level()
            torch.cuda.synchronize()
            ms, k = ctypes.c_double(), ctypes.c_int64()
            for name in ("k_hist_level", "k_level_order", "k_level_tile", "k_level_fold"):
                L.xhe_profile_read(name.encode(), ctypes.byref(ms), ctypes.byref(k))
                rec[f"b_profile_{name}_ms"] = ms.value
            L.xhe_profile(0)
            rec["b_over_a"] = rec["b_level"]["median_ms"] / rec["a_loop"]["median_ms"]
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)
            del loop_out, loop_cnt, out, cnt, st


if __name__ == "__main__":
    main()
