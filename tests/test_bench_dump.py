"""bench.py --dump-outputs helpers (CPU tensors): float files with the device
arrays' unsigned values, a fixed seeded sample of a large array, 64-bit hashes
as two exact halves, row bytes gathered from a padded arena, and the plain /
--full split of the command line."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D0 = argparse.Namespace(rank=0)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_values_dtypes_and_hash_halves(tmp_path):
    h = np.array([0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF, 0], np.uint64)
    arrays = {"key_len": torch.tensor([1, -1, 300], dtype=torch.int16),      # u16 on the device
              "val_len": torch.tensor([5, -2], dtype=torch.int32),           # u32
              "key_off": torch.tensor([0, 1 << 40], dtype=torch.int64),
              "status": torch.tensor([0, -3], dtype=torch.int32),            # signed
              "seg": torch.arange(256, dtype=torch.uint8),
              "hash": torch.from_numpy(h.view(np.int64))}
    bench.dump_outputs(D0, torch, str(tmp_path / "a"), arrays, hashes=("hash",))
    got = _load(tmp_path / "a")
    assert sorted(got) == ["hash_hi", "hash_lo", "key_len", "key_off", "seg", "status", "val_len"]
    assert got["key_len"].dtype == np.float32 and got["key_len"].tolist() == [1, 65535, 300]
    assert got["val_len"].dtype == np.float64 and got["val_len"].tolist() == [5, 2**32 - 2]
    assert got["key_off"].dtype == np.float64 and got["key_off"].tolist() == [0, 2**40]
    assert got["status"].tolist() == [0, -3]
    assert got["seg"].dtype == np.float32 and got["seg"].tolist() == list(range(256))
    back = (got["hash_hi"].astype(np.uint64) << np.uint64(32)) | got["hash_lo"].astype(np.uint64)
    assert np.array_equal(back, h)


def test_dump_large_array_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP", 1000)
    big = torch.arange(50_000, dtype=torch.int64) * 3
    for name in ("a", "b"):
        bench.dump_outputs(D0, torch, str(tmp_path / name), {"x": big.reshape(-1, 4)})
    a, b = _load(tmp_path / "a")["x"], _load(tmp_path / "b")["x"]
    assert a.shape == (1000,) and np.array_equal(a, b)           # same positions every run
    assert np.all(np.diff(a) >= 0) and np.all(a % 3 == 0) and a.max() < 150_000
    bench.dump_outputs(argparse.Namespace(rank=1), torch, str(tmp_path / "r1"), {"x": big})
    assert not (tmp_path / "r1").exists()                         # rank 0 alone writes


def test_arena_rows_skips_padding():
    arena = torch.tensor([9, 9, 1, 2, 3, 9, 9, 4, 9, 5, 6], dtype=torch.uint8)
    off = torch.tensor([2, 7, 5, 9], dtype=torch.int64)
    ln = torch.tensor([3, 1, 0, 2], dtype=torch.int16)
    got = bench._arena_rows(torch, arena, off, ln, torch.tensor([0, 1, 2, 3]))
    assert got.tolist() == [1, 2, 3, 4, 5, 6]
    assert bench._arena_rows(torch, arena, off, ln, torch.tensor([2])).size == 0
    long = torch.tensor([-1], dtype=torch.int16)  # 65535 as the device holds it
    a2 = torch.zeros(70000, dtype=torch.uint8)
    assert bench._arena_rows(torch, a2, torch.tensor([3]), long, torch.tensor([0])).size == 65535


def test_decode_dump_arrays_index_only_has_no_arenas():
    o = dict(status=torch.zeros(2, dtype=torch.int32), key_base=torch.zeros(2, dtype=torch.int64),
             val_base=torch.zeros(2, dtype=torch.int64),
             row_start=torch.tensor([0, 1, 3], dtype=torch.int64),
             key_off=torch.zeros(3, dtype=torch.int64), key_len=torch.ones(3, dtype=torch.int16),
             val_off=torch.zeros(3, dtype=torch.int64), val_len=torch.ones(3, dtype=torch.int32),
             key_arena=torch.arange(16, dtype=torch.uint8),
             val_arena=torch.arange(16, dtype=torch.uint8))
    assert sorted(bench.decode_dump_arrays(torch, o, 3, 2, True)) == [
        "key_len", "key_off", "row_start", "status", "val_len", "val_off"]
    full = bench.decode_dump_arrays(torch, o, 3, 2, False)
    assert full["key_arena_rows"].tolist() == [0, 0, 0] and "key_base" in full


@pytest.mark.parametrize("argv, msg", [(["--e2e"], "--full"), (["--steps", "0"], "--steps")])
def test_command_line_rejects(argv, msg):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and msg in r.stderr
