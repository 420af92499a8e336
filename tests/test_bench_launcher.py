"""bench.py's multi-rank contract without a GPU: `--gpus 2` with no launcher in the environment makes bench.py start its own two ranks
(torch.distributed.run on 127.0.0.1), the ranks form ONE process group of exactly N members (gloo here, RCCL on the GPU node), rank 0 prints
one JSON line with n_gpus = N and the number of ranks a collective actually saw; a launcher that started a different number of ranks than
--gpus is refused.  `--stub-engine` swaps the workload for a few CPU flops -- this tests the launcher, not the kernels."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return env


def _json_line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_gpus_2_without_a_launcher_starts_two_ranks():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "3", "--warmup", "1", "--stub-engine"], env=_env(), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["ranks_in_collective"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["launcher"] == "self"
    assert d["data"] == "stub" and d["scaling"] == "weak" and d["higher_is_better"] is True


def test_external_launcher_is_honoured_and_checked():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    base = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH]
    r = subprocess.run(base + ["--gpus", "2", "--steps", "2", "--warmup", "0", "--stub-engine"], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["ranks_in_collective"] == 2 and d["launcher"] == "external"
    # two ranks started, --gpus 4 claimed: no number may be printed
    r = subprocess.run(base + ["--gpus", "4", "--steps", "2", "--warmup", "0", "--stub-engine"], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "refusing" in (r.stderr + r.stdout)
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]


def test_single_process_default():
    r = subprocess.run([sys.executable, BENCH, "--steps", "2", "--warmup", "0", "--stub-engine"], env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 1 and d["ranks_in_collective"] == 1


def test_named_workloads_cover_the_baseline_configs():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse([])
    assert a.gpus == 1 and a.config == "sdxl-b8-euler20"
    assert set(bench.CONFIGS) == {"sdxl-b8-euler20", "sd15-b4-eulera", "sdxl-b8-dpmpp2m30-vae", "flux-b2-bf16"}
    assert bench.CONFIGS["sd15-b4-eulera"]["sampler"] == "Euler a" and bench.CONFIGS["sd15-b4-eulera"]["batch"] == 4
    assert bench.CONFIGS["sdxl-b8-dpmpp2m30-vae"]["sampler"] == "DPM++ 2M" and bench.CONFIGS["sdxl-b8-dpmpp2m30-vae"]["nominal_steps"] == 30
    assert bench.CONFIGS["flux-b2-bf16"]["dtype"] == "bf16"


def test_plain_run_is_the_default_and_extra_tables_need_full():
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert a.steps == 4 and a.warmup == 2 and not a.full and a.dump_outputs == ""
    assert bench.parse(["--full", "--breakdown", "b.jsonl", "--vae-breakdown", "v.jsonl"]).full
    for bad in (["--breakdown", "b.jsonl"], ["--vae-breakdown", "v.jsonl"], ["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)


def test_dump_outputs_writes_the_last_timed_step(tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--steps", "3", "--warmup", "1", "--stub-engine", "--dump-outputs", str(out)], env=_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    x = np.load(out / "stub.npy")
    assert x.dtype == np.float32 and x.shape == (64, 64) and (x == 64).all()


def test_dump_outputs_keeps_float_type_and_samples_a_fixed_subset_above_the_budget(tmp_path, monkeypatch):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    small = {"h": torch.arange(12, dtype=torch.float16).reshape(3, 4), "d": torch.linspace(0, 1, 5, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "small"), small)
    h, d = np.load(tmp_path / "small" / "h.npy"), np.load(tmp_path / "small" / "d.npy")
    assert h.dtype == np.float32 and h.shape == (3, 4) and np.array_equal(h, np.arange(12, dtype=np.float32).reshape(3, 4))
    assert d.dtype == np.float64 and np.array_equal(d, small["d"].numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    big = {"x": torch.arange(10000, dtype=torch.float32)}
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), big)
    xa, xb = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert xa.nbytes <= 4096 and xa.size == 1024 and np.array_equal(xa, xb)                # same seed, same sample
    assert len(np.unique(xa)) == xa.size and (np.diff(xa) > 0).all()                       # distinct elements, in their original order


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_reproducible_latents(tmp_path):
    """A plain run (no --full) carries the headline only, times exactly --steps steps, and --dump-outputs writes the same latents on every run."""
    got = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--config", "sd15-b4-eulera", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(tmp_path / run)], env=_env(), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        d = _json_line(r.stdout)
        assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "it/s" and d["higher_is_better"] is True and d["dtype"] == "f16"
        assert abs(d["value"] * d["ms_per_step"] - 1e3) < 1.0                                  # value = steps / T, ms_per_step = T / steps
        for key in ("roofline", "clocks_during_timed_steps", "vae_decode_ms_per_batch", "cpu_baseline", "torch_rocm_baseline", "rccl_world1", "other_configs"):
            assert key not in d, key
        x = np.load(tmp_path / run / "latents.npy")
        assert x.dtype == np.float32 and x.shape == (4, 4, 64, 64) and np.isfinite(x).all()
        got.append(x)
    assert np.array_equal(got[0], got[1])
