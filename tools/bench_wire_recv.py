"""Paillier.ciphertext_from into HBM: the device decode against the host decode + upload.

    python tools/bench_wire_recv.py [--sizes N,N,...] [--reps R] [--out FILE.jsonl]

One process, the 2048-bit fixture key (tests/golden). Per payload size
(default 64 k, 256 k and 1 M elements) and compression (False, True), after
one untimed call of each leg, the legs alternate rep by rep:
    host    $XHE_WIRE_DEV=0's behaviour: ciphertext_from (host decode into a
            [count, n2w] host buffer), then .to_device() (the blocking upload
            the first device operation does), then a stream synchronize
    device  wire.decode_device behind ciphertext_from, then a stream synchronize
Wall time around each, the median of R (default 5) with the fastest and the
slowest rep. One more device call runs with the pipeline's trace on: its
per-chunk stage / scan / issue times go into the result. The payloads hold
seeded random residues (the decode does not look at the values). One JSON line
per case on stdout (and appended to --out).

The kernel's own time per chunk comes from a run of this tool under
rocprofv3 --kernel-trace --stats (k_wire_unpack), in a run of its own.
"""
import argparse
import contextlib
import io
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,262144,1048576")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch  # noqa: F401  (before the library: one HIP runtime per process)

    from xfl_amd.paillier import Paillier, PaillierContext, resident, wire
    with open(os.path.join(ROOT, "tests", "golden", "paillier_2048_djn.json")) as f:
        k = json.load(f)["key"]
    pub = PaillierContext().init(int(k["p"], 16), int(k["q"], 16), djn_h_pow_n=int(k["h_pow_n"], 16)).to_public()
    dev = resident.device_for(pub)
    n2w = 128
    wire.DEV_DECODE_MIN = 1  # the device leg at every size: the threshold is what this run is for

    def host(blob, comp):
        wire.WIRE_DEV = False
        a = Paillier.ciphertext_from(pub, blob, compression=comp)
        assert not a.is_resident
        a.to_device()
        resident.stream(dev).synchronize()
        return a

    def device(blob, comp):
        wire.WIRE_DEV = True
        a = Paillier.ciphertext_from(pub, blob, compression=comp)
        assert a.is_resident and a._st.h is None
        resident.stream(dev).synchronize()
        return a

    for count in [int(s) for s in args.sizes.split(",")]:
        rng = np.random.default_rng(count)
        w = rng.integers(0, 1 << 32, size=(count, n2w), dtype=np.uint64).astype(np.uint32)
        w[:, -1] >>= 1
        e = rng.integers(-60, 0, size=count).astype(np.int32)
        for comp in (False, True):
            blob = wire.encode_words(w, e, (count,), compression=comp)
            ref = host(blob, comp)
            got = device(blob, comp)
            same = bool(torch.equal(ref._st.d, got._st.d)) and bool(np.array_equal(ref.exponents, got.exponents))
            del ref, got
            t = {"host": [], "device": []}
            for _ in range(args.reps):
                for name, leg in (("host", host), ("device", device)):
                    t0 = time.perf_counter()
                    a = leg(blob, comp)
                    t[name].append((time.perf_counter() - t0) * 1e3)
                    del a
            err = io.StringIO()
            wire._TRACE = True
            with contextlib.redirect_stderr(err):
                device(blob, comp)
            wire._TRACE = False
            m = re.search(r"\[(\(.*\))\]", err.getvalue())
            chunks = [[float(x) for x in c.split(",")] for c in re.findall(r"\(([^()]*)\)", m.group(1))] if m else []
            res = {"bench": "wire_recv", "count": count, "compression": comp, "payload_mb": round(len(blob) / 1e6, 1),
                   "reps": args.reps, "bit_equal": same}
            for name in ("host", "device"):
                res[name + "_ms"] = {"median": round(statistics.median(t[name]), 2), "min": round(min(t[name]), 2),
                                     "max": round(max(t[name]), 2)}
            res["device_wins"] = bool(res["device_ms"]["median"] < res["host_ms"]["median"] and
                                      res["device_ms"]["max"] < res["host_ms"]["min"])
            res["trace_chunk_elements_ready_stage_scan_issue_ms"] = chunks
            res["trace_sum_ms"] = {n: round(sum(c[i] for c in chunks), 2)
                                   for i, n in ((2, "ready"), (3, "stage"), (4, "scan"), (5, "issue"))}
            line = json.dumps(res)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")
            del blob


if __name__ == "__main__":
    main()
