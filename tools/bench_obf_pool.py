"""Online encryption on reserved obfuscators against the direct path.

    python tools/bench_obf_pool.py [--legs both|direct] [--large N] [--win W] [--out FILE.jsonl]

One process, through the C ABI on device buffers. Per configuration the two
legs alternate call by call:
    direct  xhe_rand + xhe_encrypt                      (what every call costs without a pool)
    online  xhe_encrypt_obf(wipe=1) on obfuscators that xhe_obf_fill made
            before the timed region (refilled, untimed, before every call)
Device events around synchronised calls, two warm-up calls, then the median of
9 (min and max kept). The fill itself is timed separately: it runs the direct
path's kernels on m = 0, so its rate is the direct rate.

  large   2048-bit private DJN key (tests/golden), N elements (default 1 M),
          fixed-base window --win (default 22, the drop-in's steady window):
          elements/s of both legs, the online leg's bytes per element and its
          share of the HBM bandwidth.
  small   1, 15, 64 and 2,048 elements on a public non-DJN and a public DJN
          2048-bit key and a private DJN 4096-bit key: ms per call.

--legs direct runs the direct legs alone: an older library loaded through
$XHE_LIB has no obfuscator entry points, and its direct legs next to this
library's show that the direct path did not move. One JSON line per
measurement on stdout (and appended to --out).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak
WARMUP, REPS = 2, 9
SMALL = (1, 15, 64, 2048)


def fixture_key(name):
    with open(os.path.join(ROOT, "tests", "golden", name)) as f:
        k = json.load(f)["key"]
    hx = lambda s: int(s, 16)  # noqa: E731
    return hx(k["n"]), hx(k["p"]), hx(k["q"]), hx(k["h_pow_n"]) if k["djn_on"] else None


class Bench:
    def __init__(self, dk, count, legs, out):
        import torch
        from xfl_amd import _native as nat
        self.torch, self.nat, self.L, self.dk, self.n, self.legs, self.out = torch, nat, nat.lib(), dk, count, legs, out
        z = lambda cols: torch.empty((count, cols), dtype=torch.int32, device="cuda")  # noqa: E731
        self.m, self.rnd, self.ct = z(dk.nw), z(dk.rand_words), z(dk.n2w)
        self.obf = z(dk.n2w) if legs == "both" else None
        x = torch.randn(count, dtype=torch.float64, device="cuda")
        ex, st = torch.empty(count, dtype=torch.int32, device="cuda"), torch.empty(count, dtype=torch.int32, device="cuda")
        self.s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        nat.check(self.L.xhe_encode_f64(dk.handle, x.data_ptr(), count, 7, 0, 0, self.m.data_ptr(), ex.data_ptr(),
                                        st.data_ptr(), self.s), "encode")
        self.nonce = 0

    def draw(self):
        self.nonce += 1
        self.nat.check(self.L.xhe_rand(self.dk.handle, os.urandom(32), self.nonce, self.n, self.rnd.data_ptr(), None,
                                       self.s), "rand")

    def direct(self):
        self.draw()
        self.nat.check(self.L.xhe_encrypt(self.dk.handle, self.m.data_ptr(), self.rnd.data_ptr(), self.n,
                                          self.ct.data_ptr(), self.s), "encrypt")

    def fill(self):
        self.draw()
        self.nat.check(self.L.xhe_obf_fill(self.dk.handle, self.rnd.data_ptr(), self.n, self.obf.data_ptr(), self.s),
                       "obf_fill")

    def online(self):
        self.nat.check(self.L.xhe_encrypt_obf(self.dk.handle, self.m.data_ptr(), self.obf.data_ptr(), self.n, 1,
                                              self.ct.data_ptr(), self.s), "encrypt_obf")

    def timed(self, fn):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def run(self, tag, extra):
        ms = {"direct": [], "fill": [], "online": []}
        for i in range(WARMUP + REPS):
            t = {"direct": self.timed(self.direct)}
            if self.legs == "both":
                t["fill"] = self.timed(self.fill)  # outside the online leg's timed region
                t["online"] = self.timed(self.online)
            if i >= WARMUP:
                for k, v in t.items():
                    ms[k].append(v)
        rec = {"config": tag, "elements": self.n, "key_bits": self.dk.key_bits, "private": self.dk.private,
               "djn": self.dk.djn, "lib": os.path.basename(self.nat.LIB_PATH), "warmup": WARMUP, "reps": REPS}
        rec.update(extra)
        for k, v in ms.items():
            if v:
                med = statistics.median(v)
                rec[f"{k}_ms"] = {"median": med, "min": min(v), "max": max(v)}
                rec[f"{k}_per_s"] = self.n / med * 1e3
        if ms["online"]:
            rec["direct_over_online"] = rec["direct_ms"]["median"] / rec["online_ms"]["median"]
            row = 4 * self.dk.n2w
            rec["online_bytes_per_element"] = {"m + X + ct": 4 * self.dk.nw + 2 * row, "with the wipe": 4 * self.dk.nw + 3 * row}
            rec["online_hbm_frac"] = rec["online_per_s"] * (4 * self.dk.nw + 3 * row) / HBM_BYTES_PER_S
        line = json.dumps(rec)
        print(line, flush=True)
        if self.out:
            with open(self.out, "a") as f:
                f.write(line + "\n")
        return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", choices=("both", "direct"), default="both")
    ap.add_argument("--large", type=int, default=1_000_000, help="elements of the large configuration (0: skip it)")
    ap.add_argument("--win", default="22", help="fixed-base window of the large configuration's key")
    ap.add_argument("--no-small", action="store_true")
    ap.add_argument("--out", help="append the JSON lines to this file")
    args = ap.parse_args()
    import torch
    from xfl_amd import _native as nat
    torch.cuda.init()
    ok = True
    if not args.no_small:
        n2, p2, q2, h2 = fixture_key("paillier_2048_djn.json")
        n4, p4, q4, h4 = fixture_key("paillier_4096_djn.json")
        for tag, make in (("small public non-DJN 2048", lambda: nat.DeviceKey(2048, n2)),
                          ("small public DJN 2048", lambda: nat.DeviceKey(2048, n2, None, None, h2)),
                          ("small private DJN 4096", lambda: nat.DeviceKey(4096, n4, p4, q4, h4))):
            dk = make()
            for count in SMALL:
                rec = Bench(dk, count, args.legs, args.out).run(tag, {})
                ok &= rec.get("direct_over_online", 2.0) > 1.0  # online faster than direct at every size
            del dk
    if args.large:
        n2, p2, q2, h2 = fixture_key("paillier_2048_djn.json")
        win = nat.parse_win(args.win)
        dk = nat.DeviceKey(2048, n2, p2, q2, h2, win_bits=win)
        rec = Bench(dk, args.large, args.legs, args.out).run("large private DJN 2048", {"window": nat.win_spec(win)})
        ok &= rec.get("direct_over_online", 2.0) >= 2.0  # the floor: a fused path that does not wait on the host
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
