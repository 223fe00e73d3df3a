"""Batch inversion mod n^2 on one GPU: xhe_invert (the product tree's root
inverted on the host, two stream synchronisations inside the call) next to
xhe_invert_dev (the root inverted by k_modinv, nothing on the host), for the
2048- and 4096-bit golden keys at `--counts` (1, 15, 256, 65536) resident
random residues.

Every timing is a host clock around one call plus torch.cuda.synchronize(),
the stream drained before it; the two entry points alternate within a
repetition; two warm-ups, then the median of `--reps` (9). k_modinv's own time
is xhe_profile's "k_modinv" (one launch per call, a run of its own). The host
inverse is not timed directly: host_modinv_est_s is xhe_invert minus
xhe_invert_dev at count 1 - what the host root costs over the device root, its
copies and synchronisations included and k_modinv's time taken off.

    python tools/bench_invert_dev.py [--counts 1,15,256,65536] [--reps 9] [--out DIR]
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

KEYS = {2048: "paillier_2048_djn.json", 4096: "paillier_4096_djn.json"}


def _stats(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "repeats_s": ts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,15,256,65536")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None, help="directory for the JSON record")
    args = ap.parse_args()
    counts = [int(c) for c in args.counts.split(",")]
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_invert_dev: no GPU")
    torch.cuda.init()
    from xfl_amd import _native as nat
    L = nat.lib()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(5)
    recs = []
    for bits, fixture in KEYS.items():
        with open(os.path.join(ROOT, "tests", "golden", fixture)) as f:
            n = int(json.load(f)["key"]["n"], 16)
        dk = nat.DeviceKey(bits, n, None, None, None, device=0)
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        cases = []
        for count in counts:
            w = rng.integers(0, 1 << 32, size=(count, dk.n2w), dtype=np.uint64).astype(np.uint32)
            w[:, dk.n2w - 1] &= 0x00FFFFFF  # below n^2; a random residue is a unit
            dc = torch.from_numpy(w.view(np.int32)).cuda()
            out_h, out_d = torch.empty_like(dc), torch.empty_like(dc)
            dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

            def host():
                nat.check(L.xhe_invert(dk.handle, dp(dc), count, dp(out_h), s), "invert")

            def dev():
                nat.check(L.xhe_invert_dev(dk.handle, dp(dc), count, dp(out_d), dp(status), s), "invert_dev")

            def once(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            th, td = [], []
            for r in range(args.reps + 2):
                a, b = once(host), once(dev)
                if r >= 2:
                    th.append(a)
                    td.append(b)
            assert int(status.item()) == 0 and torch.equal(out_h, out_d), "the two entry points differ"
            L.xhe_profile(1)
            once(dev)
            tot, cnt = ctypes.c_double(), ctypes.c_int64()
            nat.check(L.xhe_profile_read(b"k_modinv", ctypes.byref(tot), ctypes.byref(cnt)))
            L.xhe_profile(0)
            cases.append({"count": count, "xhe_invert": _stats(th), "xhe_invert_dev": _stats(td),
                          "k_modinv_ms": tot.value, "k_modinv_launches": cnt.value, "bit_exact": True})
        one = next((c for c in cases if c["count"] == 1), None)
        recs.append({"key_bits": bits, "cases": cases,
                     "host_modinv_est_s": one and one["xhe_invert"]["median_s"] - one["xhe_invert_dev"]["median_s"]})
    rec = {"reps": args.reps, "warmups": 2, "keys": recs}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "invert_dev.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
