"""CPU: bench.py --dump-outputs writes float64 .npy files that hold the
ciphertext words exactly, every row of a small shard and the same seeded
sample of a large one on every call, within the size budget. GPU: two
bench.py --dump-outputs runs with the same arguments write the same files,
and what they hold is the last timed step's output for the seeded plaintexts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from tests.conftest import ROOT


def _shard(rows, words, seed):
    g = torch.Generator().manual_seed(seed)
    ct = torch.randint(-(1 << 31), (1 << 31) - 1, (rows, words), dtype=torch.int64, generator=g).to(torch.int32)
    ex = torch.randint(-40, 0, (rows,), dtype=torch.int64, generator=g).to(torch.int32)
    return ct, ex


def _load(path, tag=""):
    return [np.load(os.path.join(path, f"{name}{tag}.npy")) for name in ("ciphertexts", "exponents", "sample_rows")]


def test_small_shard_is_dumped_whole(tmp_path):
    ct, ex = _shard(37, 128, 1)
    bench.dump_outputs(str(tmp_path / "d"), ct, ex, rank=0, world=1)
    c, e, r = _load(tmp_path / "d")
    assert c.dtype == e.dtype == r.dtype == np.float64
    assert np.array_equal(r, np.arange(37))
    assert np.array_equal(c.astype(np.uint32), ct.numpy().view(np.uint32))  # the unsigned words, exactly
    assert np.array_equal(e, ex.numpy())


def test_large_shard_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 * 128 * 8)  # room for 64 rows of 128 words
    ct, ex = _shard(1000, 128, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), ct, ex, rank=0, world=1)
    (ca, ea, ra), (cb, eb, rb) = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert np.array_equal(ra, rb) and np.array_equal(ca, cb) and np.array_equal(ea, eb)
    rows = ra.astype(np.int64)
    assert len(rows) == 64 and np.all(np.diff(rows) > 0) and rows[-1] < 1000
    assert np.array_equal(ca.astype(np.uint32), ct.numpy().view(np.uint32)[rows])
    assert np.array_equal(ea, ex.numpy()[rows])
    assert ca.nbytes <= bench.DUMP_BYTES


def test_ranks_share_the_budget_and_name_their_files(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 * 128 * 8)
    ct, ex = _shard(100, 128, 3)
    bench.dump_outputs(str(tmp_path), ct, ex, rank=1, world=2)
    c, _, r = _load(tmp_path, "_rank1")
    assert c.shape == (32, 128) and len(r) == 32


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_and_decrypt(tmp_path):
    """Two plain runs side by side (--n 1000, window 12, 3 steps): equal result
    keys, equal dumps; the dumped ciphertexts decrypt on the CPU oracle to the
    encoding of the run's seeded plaintexts at the dumped exponents."""
    from oracle import paillier_oracle as O
    from xfl_amd import _native as nat
    n = 1000
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", str(n), "--steps", "3", "--warmup", "1",
           "--win", "12", "--dump-outputs"]
    procs = [subprocess.Popen(cmd + [str(tmp_path / d)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              cwd=ROOT) for d in ("a", "b")]
    for p in procs:
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, out[-2000:] + err[-3000:]
        rec = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["value"] > 0
        assert "ops" not in rec and "cpu_baseline" not in rec and "parity_sample_ok" not in rec  # a plain run
    (ca, ea, ra), (cb, eb, rb) = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert ca.dtype == ea.dtype == np.float64 and ca.shape == (n, 128)
    assert np.array_equal(ra, np.arange(n)) and np.array_equal(ra, rb)
    assert np.array_equal(ca, cb) and np.array_equal(ea, eb)
    p_, q_, _, h_ = bench.make_key(2048, seed=2024)
    okey = O.derive_private(p_, q_, h_)
    x = np.random.default_rng(0).standard_normal(n)  # rank 0's plaintexts
    rows = [0, 1, n // 2, n - 1]
    for i, c in zip(rows, nat.words_to_ints(ca[rows].astype(np.uint32))):
        m, e = O.encode_element(okey, float(x[i]), 7)
        assert O.decrypt_raw(okey, c) == m and int(ea[i]) == e, i
