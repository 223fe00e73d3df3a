"""Prime search and key generation: host GMP against the device Fermat search,
in one process on one GPU (profiles/r12/keygen/).

Per prime width, seeded starts (random.Random(bits), top bit set), the same
ones for both paths, which alternate start by start after one untimed device
call per width (runtime initialisation, code object load). One JSON line per
start: host `_gmp.next_prime` seconds, device `primes.next_primes` seconds
(sieve, launches and GMP confirmation included), the candidates of each
launch and the kernel time xhe_profile recorded; then a summary line per
width with the `auto` verdict, and `generate(8192, djn_on=True)` on both paths
from the same seeded rng (both must find the same key).

    python tools/bench_keygen.py [--bits 1024,1536,2048,4096] [--starts 5] [--key-bits 8192] > keygen.jsonl
    python tools/bench_keygen.py --starts 2 --key-bits 0     # short form for a kernel trace
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _profile_read(nat):
    import ctypes
    ms, n = ctypes.c_double(0), ctypes.c_int64(0)
    nat.check(nat.lib().xhe_profile_read(b"k_fermat2", ctypes.byref(ms), ctypes.byref(n)), "profile_read")
    return ms.value, n.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", default="1024,1536,2048,4096")
    ap.add_argument("--starts", type=int, default=5)
    ap.add_argument("--key-bits", type=int, default=8192, help="0 skips the key generation timing")
    a = ap.parse_args()
    from xfl_amd import _native as nat
    from xfl_amd.paillier import PaillierContext, _gmp, primes
    if not _gmp.available():
        sys.exit("bench_keygen: the yardstick is GMP's mpz_nextprime; no libgmp here")
    if not primes.device_ready():
        sys.exit("bench_keygen: no library or no GPU")
    real = nat.fermat2
    counts = []

    def counted(bits, starts, which, offs, device=0):
        counts.append(len(offs))
        return real(bits, starts, which, offs, device=device)

    nat.fermat2 = counted
    for bits in [int(b) for b in a.bits.split(",") if b]:
        r = random.Random(bits)
        xs = [r.getrandbits(bits) | 1 << (bits - 1) for _ in range(a.starts)]
        primes.next_primes([xs[0] ^ 2], device=0)  # untimed: another start of this width
        host_s, dev_s = [], []
        for i, x in enumerate(xs):
            t0 = time.perf_counter()
            want = _gmp.next_prime(x)
            th = time.perf_counter() - t0
            del counts[:]
            nat.check(nat.lib().xhe_profile(1), "profile")
            t0 = time.perf_counter()
            got = primes.next_primes([x], device=0)[0]  # returns after the verdicts are on the host
            td = time.perf_counter() - t0
            kms, launches = _profile_read(nat)
            nat.check(nat.lib().xhe_profile(0), "profile")
            if got != want:
                sys.exit(f"bench_keygen: device search differs from mpz_nextprime at {bits} bits, start {i}")
            host_s.append(th)
            dev_s.append(td)
            print(json.dumps({"bits": bits, "start": i, "gap": want - x, "host_s": round(th, 5),
                              "device_s": round(td, 5), "candidates": list(counts), "launches": launches,
                              "kernel_ms": round(kms, 3)}), flush=True)
        hm, dm = statistics.median(host_s), statistics.median(dev_s)
        print(json.dumps({"bits": bits, "summary": True, "starts": a.starts, "host_median_s": round(hm, 5),
                          "device_median_s": round(dm, 5), "host_min_s": round(min(host_s), 5),
                          "device_max_s": round(max(dev_s), 5),
                          "device_ahead": bool(dm < hm and max(dev_s) < min(host_s))}), flush=True)
    if a.key_bits:
        keys = {}
        for mode in ("device", "host"):
            os.environ["XHE_KEYGEN"] = mode
            del counts[:]
            t0 = time.perf_counter()
            c = PaillierContext.generate(a.key_bits, djn_on=True, rng=random.Random(a.key_bits))
            t = time.perf_counter() - t0
            keys[mode] = (c.p, c.q)
            print(json.dumps({"generate_bits": a.key_bits, "djn": True, "path": mode, "seconds": round(t, 3),
                              "launches": len(counts), "candidates": list(counts)}), flush=True)
        if keys["device"] != keys["host"]:
            sys.exit("bench_keygen: the two paths generated different keys")


if __name__ == "__main__":
    main()
