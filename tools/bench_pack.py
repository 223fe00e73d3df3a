"""Ciphertext packing of a SecureBoost histogram against what the label trainer
does today, through the drop-in API on one GPU (golden 2048-bit DJN key, and
3072 bits with --bits 3072):

  today    decrypt_umbed of the `--bins` resident bin ciphertexts
  packed   pack_ciphertexts of the bins (the trainer, public key only), then
           decrypt_unpack of the ceil(bins / k) packed ciphertexts

with the serialize sizes of both forms. Each call is warmed up once, then
timed `--reps` times; the record holds every repeat and the median, and the
floats of both ways are compared bit for bit.

    python tools/bench_pack.py [--bits 2048] [--bins 16384] [--reps 5] [--out DIR]

--shapes measures xhe_pack alone (k = 7, 256-bit shifts, 2048 bits) in both
lane shapes at 512, 2,341, 4,096 and 16,384 outputs: one child process per
$XHE_N2_TPI setting (the switches are read once per process), kernel time from
xhe_profile's "k_pack" and wall time of the whole call. This is what
paths.hpp's kPackRowMax is set from; --outputs A,B,.. measures other counts
(written as pack_shapes_sweep.json).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPE_OUTPUTS = (512, 2341, 4096, 16384)
FIXTURE = {2048: "paillier_2048_djn.json", 3072: "paillier_3072_djn.json", 4096: "paillier_4096_djn.json",
           8192: "paillier_8192_djn.json"}


def _stats(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "repeats_s": ts}


def _golden(bits):
    with open(os.path.join(ROOT, "tests", "golden", FIXTURE[bits])) as f:
        k = json.load(f)["key"]
    return int(k["p"], 16), int(k["q"], 16), int(k["h_pow_n"], 16)


def _timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return ts


def shape_child(reps, outputs):
    """xhe_pack at `outputs` outputs under this process's switches -> one JSON line"""
    import torch
    torch.cuda.init()
    from xfl_amd import _native as nat
    from xfl_amd.paillier import resident
    p, q, _ = _golden(2048)
    n = p * q
    dk = nat.DeviceKey(2048, n, None, None, None)
    L = nat.lib()
    k, s = 7, 256
    rng = np.random.default_rng(5)
    rows = []
    for groups in outputs:
        count = groups * k
        w = rng.integers(0, 1 << 32, size=(count, dk.n2w), dtype=np.uint64).astype(np.uint32)
        w[:, dk.n2w - 1] &= 0x0FFFFFFF  # below n^2
        c = resident.upload(w, dk.device)
        wall, kern = [], []
        for r in range(reps + 1):
            torch.cuda.synchronize()
            L.xhe_profile(1)
            t = time.perf_counter()
            resident.pack(dk, c, k, s)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            tot, cnt = ctypes.c_double(), ctypes.c_int64()
            nat.check(L.xhe_profile_read(b"k_pack", ctypes.byref(tot), ctypes.byref(cnt)))
            L.xhe_profile(0)
            if r:  # the first run warms up
                wall.append(dt)
                kern.append(tot.value / 1e3)
        rows.append({"outputs": groups, "k": k, "shift_bits": s, "k_pack": _stats(kern), "call": _stats(wall)})
    print(json.dumps({"XHE_N2_TPI": os.environ.get("XHE_N2_TPI"), "XHE_NDIG": os.environ.get("XHE_NDIG"),
                      "rows": rows}), flush=True)


def shapes(args):
    rec = {"key_bits": 2048, "reps": args.reps, "shapes": []}
    for env in ({"XHE_N2_TPI": "16"}, {"XHE_N2_TPI": "4"}, {"XHE_N2_TPI": "4", "XHE_NDIG": "0"}):
        e = {k: v for k, v in os.environ.items() if k not in ("XHE_N2_TPI", "XHE_NDIG")}
        e.update(env)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape-child", "--reps", str(args.reps),
                            "--outputs", args.outputs], env=e, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"bench_pack: the child of {env} ended with status {r.returncode}\n{r.stderr[-3000:]}")
        rec["shapes"].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    default = args.outputs == ",".join(map(str, SHAPE_OUTPUTS))
    _emit(rec, args.out, "pack_shapes.json" if default else "pack_shapes_sweep.json")


def _emit(rec, out, name):
    line = json.dumps(rec)
    print(line)
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, name), "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=2048, choices=sorted(FIXTURE))
    ap.add_argument("--bins", type=int, default=16_384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="directory for the JSON record")
    ap.add_argument("--shapes", action="store_true", help="xhe_pack in both lane shapes (kPackRowMax)")
    ap.add_argument("--outputs", default=",".join(map(str, SHAPE_OUTPUTS)), help="--shapes: the output counts")
    ap.add_argument("--shape-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.shape_child:
        return shape_child(args.reps, [int(v) for v in args.outputs.split(",")])
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pack: no GPU")
    torch.cuda.init()
    if args.shapes:
        return shapes(args)
    from xfl_amd import _native as nat
    from xfl_amd.paillier import Paillier, PaillierContext
    from xfl_amd.paillier_acceleration import decrypt_umbed, decrypt_unpack, pack_ciphertexts, pack_factor
    p, q, h = _golden(args.bits)
    priv = PaillierContext().init(p, q, djn_h_pow_n=h)
    pub = priv.to_public()
    NB = args.bins
    k = pack_factor(priv.n)
    # bins as a histogram holds them: (sum of grads, sum of hessians) of ~6 samples, 64 fractional bits
    rng = np.random.default_rng(3)
    g = np.rint((rng.random(NB) - 0.5) * 6 * 2.0 ** 64).astype(object)
    hs = np.rint(rng.random(NB) * 1.5 * 2.0 ** 64).astype(object)
    sums = np.empty(NB, dtype=object)
    sums[:] = [int(a) * (1 << 128) + int(b) for a, b in zip(g, hs)]
    hist = Paillier.encrypt(pub, sums, precision=0).to_device()
    assert hist.is_resident
    L = nat.lib()

    def profiled(fn, label):
        L.xhe_profile(1)
        fn()
        tot, cnt = ctypes.c_double(), ctypes.c_int64()
        nat.check(L.xhe_profile_read(label, ctypes.byref(tot), ctypes.byref(cnt)))
        L.xhe_profile(0)
        return tot.value, cnt.value

    def today():
        return decrypt_umbed(priv, hist, 2)

    def pack():
        out = pack_ciphertexts(hist)
        torch.cuda.synchronize()
        return out

    packed = pack()
    assert packed.is_resident and len(packed) == -(-NB // k)

    def unpack():
        return decrypt_unpack(priv, packed, NB)

    want, got = today(), unpack()
    exact = all(np.array_equal(want[j].view(np.uint32), got[j].view(np.uint32)) for j in range(2))
    assert exact, "decrypt_unpack differs from decrypt_umbed"
    t_today, t_pack, t_unpack = _timed(today, args.reps), _timed(pack, args.reps), _timed(unpack, args.reps)
    k_pack_ms, k_pack_launches = profiled(pack, b"k_pack")
    wire_bins = len(Paillier.serialize(hist, compression=False))
    wire_packed = len(Paillier.serialize(packed, compression=False))
    med = statistics.median
    rec = {"key_bits": args.bits, "bins": NB, "k": k, "packed_ciphertexts": len(packed), "geometry": [2, 128, 64],
           "reps": args.reps, "decrypt_umbed_bins": _stats(t_today), "pack_ciphertexts": _stats(t_pack),
           "decrypt_unpack": _stats(t_unpack), "k_pack_ms": k_pack_ms, "k_pack_launches": k_pack_launches,
           "pack_plus_unpack_median_s": med(t_pack) + med(t_unpack),
           "serialize_bytes_bins": wire_bins, "serialize_bytes_packed": wire_packed, "bit_exact": bool(exact)}
    _emit(rec, args.out, f"pack_{args.bits}.json")


if __name__ == "__main__":
    main()
