"""Decrypt (or, with --enc, DJN private encrypt) latency/throughput per batch
size for one lane shape: XHE_DEC_TPI = 1, 4 or 16 pins the decrypt shape,
XHE_ENC_TPI = 16 or 0 the encrypt one; unset = the library's choice by size.
Device-resident operands, wall time of the call + synchronize, median of 5.
Prints one JSON line.

    XHE_DEC_TPI=16 python tools/dec_shapes.py [sizes...]
    XHE_ENC_TPI=0 python tools/dec_shapes.py --enc [--short] [sizes...]

--enc encrypts plaintexts with random 30-bit words in every word: general
plaintexts for k_djn_pmd. --short makes them what the float encodings produce,
+-s with s below 2^27 (a negative one stored as n - s), signs alternating: every
wave takes the kernel's short-plaintext entry.

--pub: xhe_encrypt on a PUBLIC non-DJN 2048-bit key (the obfuscator r^n of a
party that received the key, Paillier.encrypt(public_context, ...) of the
regression operators) at 1 .. 8 k elements, device events around synchronised
calls, warmed up, median of --reps (default 9). XHE_PUB_TPI = 64 or 4 pins
the block-per-element or the 4-lane path.
--matmul: np.matmul(enc.reshape(1, B), X) of the drop-in API at (B, D) =
(64, 15) and (2048, 15), wall time of the call + synchronize.

    python tools/dec_shapes.py --pub [sizes...]
    python tools/dec_shapes.py --matmul

A/B against another commit's build: --ab ROOT runs the sweep alternately from
this tree and from ROOT (a checkout of the other commit, its library built
with `python -m xfl_amd.build --out ROOT/libxhe_ab.so -D XHE_ONLY_2048`
and loaded through XHE_LIB), --rounds times each, every run a fresh process,
and writes the table (per size: both medians and their ratio) to --out.

    python tools/dec_shapes.py --pub --ab ../parent --out profiles/r9/pub_small/pub_encrypt.json
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ("--enc", "--pub", "--matmul", "--short")
OPTS = ("--ab", "--out", "--root", "--reps", "--rounds")


def _args():
    flags, opts, sizes = set(), {}, []
    it = iter(sys.argv[1:])
    for a in it:
        if a in FLAGS:
            flags.add(a)
        elif a in OPTS:
            opts[a] = next(it)
        else:
            sizes.append(int(a))
    return flags, opts, sizes


def _median(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2]


def sweep_pub(sizes, reps):
    import torch

    from bench import make_key
    from xfl_amd import _native as nat
    _, _, n, _ = make_key(2048, seed=2024)
    dk = nat.DeviceKey(2048, n, None, None, None)
    assert not dk.private and not dk.djn
    L = nat.lib()
    sizes = sizes or [1, 15, 64, 256, 1024, 2048, 4096, 8192]
    N = max(sizes)
    m = torch.randint(0, 1 << 30, (N, dk.nw), dtype=torch.int32, device="cuda")
    m[:, -1] = 0  # below n
    r = torch.randint(0, 1 << 30, (N, dk.rand_words), dtype=torch.int32, device="cuda")
    r[:, -1] = 1
    c = torch.empty((N, dk.n2w), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    out = {"op": "encrypt_pub_nodjn", "tpi": os.environ.get("XHE_PUB_TPI", "auto"), "lib": os.path.relpath(nat.LIB_PATH, HERE_ROOT)}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for k in sizes:
        ts = []
        for it in range(reps + 2):  # two warm-up calls
            torch.cuda.synchronize()
            a.record()
            nat.check(L.xhe_encrypt(dk.handle, m.data_ptr(), r.data_ptr(), k, c.data_ptr(), s))
            b.record()
            torch.cuda.synchronize()
            if it >= 2:
                ts.append(a.elapsed_time(b))
        out[str(k)] = {"ms": round(_median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}
    return out


def sweep_matmul(sizes, reps):
    import torch

    from bench import make_key
    from xfl_amd.paillier import Paillier, PaillierContext
    p, q, _, _ = make_key(2048, seed=2024)
    pub = PaillierContext().init(p, q).to_public()
    rng = np.random.default_rng(3)
    out = {"op": "matmul_row_matrix"}
    for B, D in ((64, 15), (2048, 15)):
        enc = Paillier.encrypt(pub, rng.standard_normal(B).astype(np.float32), precision=7, obfuscation=False)
        X = rng.standard_normal((B, D)).astype(np.float32)
        ts = []
        budget = time.perf_counter() + 60.0  # the object loop of the large shape takes its time
        for it in range(reps + 1):  # one warm-up call
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = np.matmul(enc.reshape(1, B), X)
            res.words  # the result on the host, whichever path made it
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            if it >= 1 or dt > 5.0:
                ts.append(dt * 1e3)
            if time.perf_counter() > budget or dt > 5.0:
                break
        assert res.shape == (1, D)
        out[f"{B}x{D}"] = {"ms": round(_median(ts), 3), "calls": len(ts)}
    return out


def sweep_dec_enc(enc, sizes, short=False):
    import torch

    from bench import make_key
    from xfl_amd import _native as nat
    p, q, n, h = make_key(2048, seed=2024)
    dk = nat.DeviceKey(2048, n, p, q, h, win_bits=16)
    L = nat.lib()
    sizes = sizes or [1, 15, 64, 256, 1024, 2048, 4096, 16384, 65536]
    N = max(sizes)
    rng = np.random.default_rng(1)
    c = torch.from_numpy(rng.integers(0, 2 ** 32, (N, dk.n2w), dtype=np.uint64).astype(np.uint32).view(np.int32))
    c[:, -1] = c[:, -1] & 0x0FFFFFFF  # below n^2's top word range
    c = c.cuda()
    m = torch.empty((N, dk.nw), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    out = {"op": "encrypt" if enc else "decrypt",
           "tpi": os.environ.get("XHE_ENC_TPI" if enc else "XHE_DEC_TPI", "auto")}
    if enc:
        if short:
            srng = np.random.default_rng(2)
            mags = srng.integers(1, 1 << 27, N)
            vals = [int(v) if i & 1 == 0 else n - int(v) for i, v in enumerate(mags)]
            m = torch.from_numpy(nat.ints_to_words(vals, dk.nw).view(np.int32)).cuda()
            out["plaintexts"] = "short"
        else:
            m.random_(0, 1 << 30)
            m[:, -1] = 0
        r = torch.randint(0, 1 << 30, (N, dk.rand_words), dtype=torch.int32, device="cuda")
    for k in sizes:
        ts = []
        for _ in range(5):
            torch.cuda.synchronize()
            t = time.perf_counter()
            if enc:
                nat.check(L.xhe_encrypt(dk.handle, m.data_ptr(), r.data_ptr(), k, c.data_ptr(), s))
            else:
                nat.check(L.xhe_decrypt(dk.handle, c.data_ptr(), k, m.data_ptr(), s))
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        ts.sort()
        out[str(k)] = {"ms": round(ts[2] * 1e3, 3), "per_s": round(k / ts[2])}
    return out


def run_ab(flags, opts, sizes):
    """this tree and the --ab checkout alternately, a fresh process each"""
    other = os.path.abspath(opts["--ab"])
    rounds = int(opts.get("--rounds", 3))
    mode = "--pub" if "--pub" in flags else "--matmul"
    base = [sys.executable, os.path.abspath(__file__), mode] + [str(k) for k in sizes]
    if "--reps" in opts:
        base += ["--reps", opts["--reps"]]
    runs = {"branch": [], "other": []}
    for _ in range(rounds):
        for side in ("other", "branch"):
            env = dict(os.environ)
            cmd = list(base)
            if side == "other":
                env["XHE_LIB"] = os.path.join(other, "libxhe_ab.so")
                cmd += ["--root", other]
            else:
                env.pop("XHE_LIB", None)
            p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=360)
            if p.returncode != 0:  # nothing more on the GPU after a failed run
                raise SystemExit(f"{side} run failed ({p.returncode})")
            rec = json.loads(p.stdout.strip().splitlines()[-1])
            runs[side].append(rec)
            print(side, json.dumps(rec), flush=True)
    table = {"op": runs["branch"][0]["op"], "rounds": rounds, "other": os.path.relpath(other, HERE_ROOT), "rows": {}}
    for key, v in runs["branch"][0].items():
        if not isinstance(v, dict):
            continue
        mb = _median([r[key]["ms"] for r in runs["branch"]])
        mo = _median([r[key]["ms"] for r in runs["other"]])
        table["rows"][key] = {"other_ms": mo, "branch_ms": mb, "speedup": round(mo / mb, 3)}
    table["runs"] = runs
    if "--out" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["--out"])), exist_ok=True)
        with open(opts["--out"], "w") as f:
            json.dump(table, f, indent=1)
            f.write("\n")
    print(json.dumps(table["rows"]))


def main():
    flags, opts, sizes = _args()
    if "--ab" in opts:
        if not flags & {"--pub", "--matmul"}:
            raise SystemExit("--ab goes with --pub or --matmul")
        run_ab(flags, opts, sizes)
        return
    sys.path.insert(0, os.path.abspath(opts.get("--root", HERE_ROOT)))
    reps = int(opts.get("--reps", 9))
    if "--pub" in flags:
        out = sweep_pub(sizes, reps)
    elif "--matmul" in flags:
        out = sweep_matmul(sizes, min(reps, 5))
    else:
        out = sweep_dec_enc("--enc" in flags, sizes, "--short" in flags)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
