"""The fused histogram (xhe_hist) next to the paths it replaces, on config 5:
100 k samples x 64 features x 256 bins, the 2048-bit key and the seeded data of
tools/bench_configs.py::cfg5.

  (a) cfg5's build(): ct.index_select(bin order) + xhe_segprod, with and
      without the argsort / bincount / offsets preparation cfg5 leaves outside
      its timer
  (b) one xhe_hist call on the rows where they lie
  (c) the drop-in: the 64-call groupby loop of bench.py's
      measure_dropin_histogram against one histograms() call (wall clock, host
      work included)
  (d) peak extra device memory of (a) and (b) (free memory polled from a
      second thread while the call runs)
  (e) --shapes: nbins 2, 16 and 4096; a 10 k-row subset through row ids; one
      feature whose rows all fall into one bin; 1 M rows x 8 features

Device events around synchronised calls, two warm-ups, median / fastest /
slowest of --reps. A sample of bins is checked against Python integers. One JSON
file under --out.

    python tools/bench_hist.py [--shapes] [--reps 5] [--out profiles/r24/hist]
"""
import argparse
import ctypes
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, reps):
    """median / min / max ms of fn() by device events, after two warm-ups"""
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def wall(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    ts.sort()
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}


def trim_pool():
    """give the blocks the device's stream-ordered pool keeps after a call back to the device (the library's
    workspaces come from it), through the HIP runtime this process has loaded; False when that fails"""
    try:
        with open("/proc/self/maps") as f:
            path = next(line.split()[-1] for line in f if "libamdhip64" in line)
        hip = ctypes.CDLL(path)
        pool = ctypes.c_void_p()
        ok = hip.hipDeviceGetDefaultMemPool(ctypes.byref(pool), 0) == 0
        return bool(ok and hip.hipMemPoolTrimTo(pool, ctypes.c_size_t(0)) == 0)
    except (OSError, StopIteration, AttributeError):
        return False


def peak_extra_bytes(fn):
    """free memory before minus the least free memory seen while fn() runs, with the caches of the warm-up
    released first (torch's and the stream-ordered pool's), so that the call's own allocations show"""
    import torch
    fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    trim_pool()
    free0 = torch.cuda.mem_get_info()[0]
    low, stop = [free0], threading.Event()

    def poll():
        while not stop.is_set():
            low[0] = min(low[0], torch.cuda.mem_get_info()[0])
    th = threading.Thread(target=poll)
    th.start()
    fn()
    torch.cuda.synchronize()
    stop.set()
    th.join()
    return int(free0 - low[0])


class Hist:
    """device buffers of one xhe_hist problem over the ciphertext rows ct"""

    def __init__(self, nat, dk, ct, bins, nbins, rows=None):
        import torch
        self.nat, self.dk, self.ct, self.nbins, self.bins = nat, dk, ct, nbins, bins
        self.F = bins.shape[0]
        self.bd = torch.from_numpy(np.ascontiguousarray(bins, dtype=np.uint16).view(np.int16)).cuda()
        self.rows = rows
        self.rd = None if rows is None else torch.from_numpy(rows.astype(np.int32)).cuda()
        self.out = torch.empty((self.F * nbins, dk.n2w), dtype=torch.int32, device="cuda")
        self.cnt = torch.empty(self.F * nbins, dtype=torch.int32, device="cuda")
        self.s = torch.cuda.current_stream().cuda_stream

    def __call__(self):
        n = self.ct.shape[0]
        self.nat.check(self.nat.lib().xhe_hist(
            self.dk.handle, self.ct.data_ptr(), n, self.bd.data_ptr(), self.bins.shape[1], self.F, self.nbins,
            None if self.rd is None else self.rd.data_ptr(), n if self.rd is None else self.rd.shape[0], 0,
            self.out.data_ptr(), self.cnt.data_ptr(), self.s), "hist")

    def check(self, n2, sample):
        """the (feature, bin) pairs of `sample` against Python integers, every count against np.bincount"""
        import torch
        torch.cuda.synchronize()
        sel = np.arange(self.ct.shape[0]) if self.rows is None else self.rows
        ids = self.bins[:, sel].astype(np.int64)
        want = np.stack([np.bincount(r[r < self.nbins], minlength=self.nbins) for r in ids]).reshape(-1)
        ok = bool(np.array_equal(self.cnt.cpu().numpy(), want))
        for f, b in sample:
            rows = sel[ids[f] == b]
            cs = self.nat.words_to_ints(self.ct[torch.from_numpy(rows).cuda()].cpu().numpy().view(np.uint32)) \
                if rows.size else []
            acc = 1
            for c in cs:
                acc = acc * c % n2
            got = self.nat.words_to_ints(self.out[f * self.nbins + b:f * self.nbins + b + 1].cpu().numpy().view(np.uint32))
            ok &= got[0] == acc
        return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-dropin", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24", "hist"))
    args = ap.parse_args()
    import torch

    from bench import make_key
    from xfl_amd import _native as nat
    from xfl_amd.paillier_acceleration import embed
    L = nat.lib()
    p, q, n, h = make_key(2048, seed=2024)
    dk = nat.DeviceKey(2048, n, p, q, h, device=0, win_bits=16)
    n2 = n * n
    S, F, NB = 100_000, 64, 256
    rng = np.random.default_rng(3)
    z = rng.standard_normal(S)
    y = (rng.random(S) < 0.5).astype(np.float64)
    pr = 1.0 / (1.0 + np.exp(-z))
    gr, he = pr - y, pr * (1.0 - pr)
    bins = np.stack([np.random.default_rng(4 + f).integers(0, NB, S) for f in range(F)])
    mw = nat.ints_to_words([int(v) % n for v in embed([gr, he])], dk.nw)
    mdev = torch.from_numpy(mw.view(np.int32)).cuda()
    rnd = torch.empty((S, dk.rand_words), dtype=torch.int32, device="cuda")
    ct = torch.empty((S, dk.n2w), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    nat.check(L.xhe_rand(dk.handle, b"\x05" * 32, 3, S, rnd.data_ptr(), None, s), "rand")
    nat.check(L.xhe_encrypt(dk.handle, mdev.data_ptr(), rnd.data_ptr(), S, ct.data_ptr(), s), "encrypt")
    torch.cuda.synchronize()
    del rnd, mdev
    rec = {"config": f"{S} samples x {F} features x {NB} bins, 2048-bit", "reps": args.reps,
           "pool_trimmed_before_memory_poll": trim_pool()}

    # (a) cfg5's path
    local = torch.empty((F * NB, dk.n2w), dtype=torch.int32, device="cuda")
    bins_d = torch.from_numpy(np.ascontiguousarray(bins)).cuda()
    st = {}

    def prep():
        st["order"] = torch.argsort(bins_d, dim=1, stable=True)
        counts = np.stack([np.bincount(bins[f], minlength=NB) for f in range(F)]).reshape(-1)
        st["seg"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)

    def build():
        gathered = ct.index_select(0, st["order"].reshape(-1))
        nat.check(L.xhe_segprod(dk.handle, gathered.data_ptr(), None, 0, F * S, st["seg"].ctypes.data_as(
            ctypes.c_void_p), F * NB, local.data_ptr(), s), "segprod")

    def prep_build():
        prep()
        build()
    prep()
    rec["a_gather_segprod"] = timed(build, args.reps)
    rec["a_with_preparation"] = timed(prep_build, args.reps)
    rec["a_peak_extra_bytes"] = peak_extra_bytes(build)
    want = local.clone()

    # (b) one xhe_hist call
    hb = Hist(nat, dk, ct, bins, NB)
    rec["b_hist"] = timed(hb, args.reps)
    rec["b_peak_extra_bytes"] = peak_extra_bytes(hb)
    rec["b_equals_a_bit_for_bit"] = bool(torch.equal(hb.out, want))
    rec["b_sample_bins_exact"] = hb.check(n2, [(0, 0), (17, 255), (63, 101)])
    L.xhe_profile(1)
    hb()
    torch.cuda.synchronize()
    ms, cnt = ctypes.c_double(), ctypes.c_int64()
    for name in ("k_hist", "k_hist_tile"):
        L.xhe_profile_read(name.encode(), ctypes.byref(ms), ctypes.byref(cnt))
        rec[f"b_profile_{name}_ms"] = ms.value
    L.xhe_profile(0)
    rec["b_at_most_a"] = rec["b_hist"]["median_ms"] <= rec["a_gather_segprod"]["max_ms"]
    del want, local

    # (c) the drop-in
    if not args.no_dropin:
        import pandas as pd

        from xfl_amd.paillier import Paillier, PaillierContext
        from xfl_amd.paillier_acceleration import embed_packed, histograms
        ctx = PaillierContext().init(p, q, djn_h_pow_n=h)
        enc = Paillier.encrypt(ctx, embed_packed([gr, he]), precision=0)
        values = pd.DataFrame({f"x{f}": bins[f].astype(np.uint8) for f in range(F)})
        data = pd.concat([pd.DataFrame(enc, columns=["xfl_grad_hess"]), values], axis=1)
        res = {}

        def loop():
            res["loop"] = [data.groupby([c])["xfl_grad_hess"].agg({"count", "sum"}) for c in values.columns]

        def fused():
            res["fused"] = histograms(enc, values, nbins=NB)
        rec["c_groupby_loop_64_calls"] = wall(loop, 3)
        rec["c_histograms_one_call"] = wall(fused, 3)
        sums, counts = res["fused"]
        rec["c_equal_bit_for_bit"] = all(
            np.array_equal(np.asarray(sums[f].words), np.asarray(res["loop"][f]["sum"].array.words))
            and np.array_equal(counts[f], res["loop"][f]["count"].to_numpy()) for f in (0, 31, 63))
        del enc, data, res, sums

    # (e) other shapes
    if args.shapes:
        shapes = {}
        for nb in (2, 16, 4096):
            b2 = np.stack([np.random.default_rng(90 + f).integers(0, nb, S) for f in range(F)])
            hs = Hist(nat, dk, ct, b2, nb)
            shapes[f"nbins_{nb}"] = dict(timed(hs, args.reps), exact=hs.check(n2, [(1, 0), (F - 1, nb - 1)] if nb < 4096
                                                                             else [(1, 7), (F - 1, nb - 1)]))
        rows = np.random.default_rng(77).permutation(S)[:10_000]
        hs = Hist(nat, dk, ct, bins, NB, rows=rows)
        shapes["subset_10k_rows"] = dict(timed(hs, args.reps), exact=hs.check(n2, [(0, 3), (63, 200)]))
        one = bins.copy()
        one[5, :] = 9
        hs = Hist(nat, dk, ct, one[5:6], NB)
        shapes["one_feature_one_bin"] = dict(timed(hs, args.reps), exact=hs.check(n2, [(0, 8), (0, 9)]))
        hs = Hist(nat, dk, ct, bins[5:6], NB)
        shapes["one_feature_balanced"] = dict(timed(hs, args.reps), exact=hs.check(n2, [(0, 8)]))
        shapes["one_bin_over_balanced"] = shapes["one_feature_one_bin"]["median_ms"] / \
            shapes["one_feature_balanced"]["median_ms"]
        M = 1_000_000
        big = ct.repeat(M // S, 1)
        b8 = np.stack([np.random.default_rng(300 + f).integers(0, NB, M) for f in range(8)])
        hs = Hist(nat, dk, big, b8, NB)
        shapes["1M_x_8"] = dict(timed(hs, max(2, args.reps // 2)), exact=hs.check(n2, [(7, 255)]))
        rec["shapes"] = shapes

    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "hist_2048.json"), "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
