"""Label-side packed pipeline of SecureBoost, host packing against device
packing, through the drop-in API on one GPU (2048-bit DJN key):

  encrypt side  embed        -> Paillier.encrypt(precision=0) -> Paillier.serialize(compression=False)
                embed_packed -> the same two calls
  decrypt side  Paillier.decrypt(out_origin=True) + umbed   of 16,384 resident bins
                decrypt_umbed                               of the same bins

Each sequence is warmed up once, then the two of a side alternate for
`--reps` rounds; the record holds every repeat, the median and the spread,
and the results are compared bit for bit (the obfuscated encryptions through
their decryption).

    python tools/bench_packed.py [--samples 100000] [--bins 16384] [--reps 5] [--out DIR]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _stats(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "repeats_s": ts}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100_000)
    ap.add_argument("--bins", type=int, default=16_384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="directory for packed.json")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_packed: no GPU")
    from bench import make_key
    from xfl_amd.paillier import Paillier, PaillierContext
    from xfl_amd.paillier_acceleration import decrypt_umbed, embed, embed_packed, umbed
    p, q, n, h = make_key(2048, seed=2024)
    priv = PaillierContext().init(p, q, djn_h_pow_n=h)
    S, NB = args.samples, args.bins
    rng = np.random.default_rng(3)
    z = rng.standard_normal(S)
    y = (rng.random(S) < 0.5).astype(np.float64)
    pr = 1.0 / (1.0 + np.exp(-z))
    cols = [pr - y, pr * (1.0 - pr)]

    def enc_host():
        return Paillier.serialize(Paillier.encrypt(priv, embed(cols), precision=0), compression=False)

    def enc_device():
        return Paillier.serialize(Paillier.encrypt(priv, embed_packed(cols), precision=0), compression=False)

    ints = [int(v) for v in embed(cols)]
    for fn in (enc_host, enc_device):  # warm-up, and the plaintexts behind both payloads
        back = Paillier.ciphertext_from(priv, fn(), compression=False)
        assert [int(v) for v in Paillier.decrypt(priv, back, out_origin=True)] == ints, fn.__name__
    t_enc = {"host": [], "device": []}
    for _ in range(args.reps):
        for name, fn in (("host", enc_host), ("device", enc_device)):
            t = time.perf_counter()
            fn()
            t_enc[name].append(time.perf_counter() - t)

    # the bins: sums of consecutive samples' packed values, resident as a histogram is
    seg = np.linspace(0, S, NB + 1).astype(np.int64)
    sums = np.empty(NB, dtype=object)
    sums[:] = [sum(ints[a:b]) for a, b in zip(seg[:-1], seg[1:])]
    hist = Paillier.encrypt(priv, sums, precision=0).to_device()

    def dec_host():
        return umbed(Paillier.decrypt(priv, hist, out_origin=True), 2)

    def dec_device():
        return decrypt_umbed(priv, hist, 2)

    want, got = dec_host(), dec_device()
    exact = all(np.array_equal(np.array(want[j], np.float32).view(np.uint32), got[j].view(np.uint32)) for j in range(2))
    assert exact, "decrypt_umbed differs from decrypt + umbed"
    t_dec = {"host": [], "device": []}
    for _ in range(args.reps):
        for name, fn in (("host", dec_host), ("device", dec_device)):
            t = time.perf_counter()
            fn()
            t_dec[name].append(time.perf_counter() - t)
    rec = {"samples": S, "bins": NB, "geometry": [2, 128, 64], "key_bits": 2048, "reps": args.reps,
           "embed_encrypt_serialize_host": _stats(t_enc["host"]),
           "embed_packed_encrypt_serialize_device": _stats(t_enc["device"]),
           "decrypt_umbed_host": _stats(t_dec["host"]), "decrypt_umbed_device": _stats(t_dec["device"]),
           "encrypt_plaintexts_equal": True, "decrypt_bit_exact": bool(exact)}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "packed.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
