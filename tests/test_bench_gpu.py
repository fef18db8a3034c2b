"""bench.py on the GPU (small configurations): the JSON line's contract fields,
the oracle check of the bench's own outputs, and the decodes-in-flight path
(two contexts, streams and output sets; outputs compared before timing)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args],
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("inflight", ["1", "2"])
def test_bench_c2_line(inflight):
    d = _bench("--config", "c2", "--steps", "3", "--warmup", "1", "--full", "--no-cpu",
               "--decode-inflight", inflight)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["value"] > 0
    assert d["decodes_in_flight"] == int(inflight)
    assert d["latency_ms_per_step"] > 0
    assert d["verify"]["verified"].startswith("all output arrays == oracle")
    r = d["roofline"]
    assert r["bound"] == "hbm" and 0 < r["frac"] < 1 and r["peak"] == 8000.0


@pytest.mark.gpu
def test_bench_plain_run_and_dump(tmp_path):
    """A plain run carries the headline fields alone (what --full adds is
    absent, not null), and --dump-outputs writes the last timed step's decode
    as float arrays equal to the oracle's decode of the same segment."""
    import numpy as np

    import bench
    import objectkv_amd as okv
    from oracle import coracle

    d = _bench("--config", "c2", "--steps", "3", "--warmup", "1", "--dump-outputs",
               str(tmp_path / "dump"))
    assert d["metric"] == bench.METRIC and d["unit"] == "GiB/s" and d["dtype"] == "u8"
    assert d["higher_is_better"] is True and d["steps"] == 3 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    in_bytes = d["config"]["block_bytes_per_gpu"]
    # value = input bytes over the same step time (the line rounds ms_per_step to 1e-4 ms)
    assert abs(d["value"] - in_bytes / (d["ms_per_step"] * 1e-3) / 2**30) <= \
        d["value"] * 5e-5 / (d["ms_per_step"] - 5e-5) + 1e-3
    for k in ("cpu_baseline", "verify", "roofline", "kernel_ms", "latency_ms_per_step"):
        assert k not in d, k

    kind, seed, nblk, th, bs, _ = bench.CONFIGS["c2"]
    w = okv.synth_segment(kind, seed, nblocks=nblk, threshold=th, block_size=bs)
    descs = w.descs()[:nblk]
    ref = coracle.decode_soa(w.data(), coracle.descs_array([tuple(int(x) for x in r)
                                                            for r in descs]))
    got = {f[:-4]: np.load(tmp_path / "dump" / f) for f in os.listdir(tmp_path / "dump")}
    assert sum(a.nbytes for a in got.values()) <= 64e6
    for k in ("status", "row_start", "key_base", "val_base", "key_off", "key_len", "val_off",
              "val_len"):
        assert got[k].dtype in (np.float32, np.float64), (k, got[k].dtype)
        assert np.array_equal(got[k], ref[k].astype(got[k].dtype)), k
    rows = int(ref["row_start"][-1])
    assert rows > bench.DUMP_ROWS  # the arenas are dumped as a seeded sample of rows
    pick = np.sort(np.random.default_rng(0x0B5E).integers(0, rows, bench.DUMP_ROWS))
    for a in ("key", "val"):
        want = np.concatenate([ref[a + "_arena"][int(o):int(o) + int(n)] for o, n in
                               zip(ref[a + "_off"][pick], ref[a + "_len"][pick])])
        assert got[a + "_arena_rows"].dtype == np.float32
        assert np.array_equal(got[a + "_arena_rows"], want.astype(np.float32)), a


@pytest.mark.gpu
def test_rccl_control_plane_world1():
    """The nccl (RCCL) control plane executes on the GPU: process group init with
    device_id, barriers and the all_gather of the ranks' times, at world size 1
    under torch.distributed.run (two ranks cannot share one GPU under RCCL).
    The default control plane is gloo (no data-path collective exists)."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", "29631", os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--config", "c2", "--steps", "3", "--warmup", "1", "--full",
                        "--no-cpu", "--dist-backend", "nccl", "--dist-always"],
                       capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["dist"] == {"world_size": 1, "dist_backend": "nccl"}, d["dist"]
    assert d["n_gpus"] == 1 and d["value"] > 0
    assert d["verify"]["verified"].startswith("all output arrays == oracle")
