"""CPU: ``python bench.py --gpus 2`` without a launcher starts its two ranks itself (child processes through
torch.distributed.run, rendezvous on 127.0.0.1) and rank 0 prints the one JSON line with n_gpus = 2.  Runs the dry mode
(MCDSEG_BENCH_DRY=1: gloo, a stand-in step, the real barriers / MAX-over-ranks protocol) -- no GPU work."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(argv, extra_env):
    env = dict(os.environ, MCDSEG_BENCH_DRY="1", OMP_NUM_THREADS="1", **extra_env)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True, text=True, timeout=600)


def test_bench_spawns_its_ranks():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "0"], {})
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["scaling"] == "weak"
    # MAX over ranks: rank 1's stand-in step is twice as long as rank 0's
    assert rec["ms_per_step"] >= 19.0


def test_bench_rejects_world_size_mismatch():
    env = dict(os.environ, MCDSEG_BENCH_DRY="1", WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_for_dump_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_writes_the_losses_and_the_state(tmp_path, monkeypatch):
    """``--dump-outputs DIR``: the two losses (float64) and each model's floating-point state flattened in state_dict order (float32);
    a model over DUMP_MAX_ELEMS elements is written at a fixed sample of its positions, the same in every run."""
    import numpy as np
    import torch
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    torch.manual_seed(0)
    g, f1, f2 = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.BatchNorm1d(32)), torch.nn.Linear(4, 3), torch.nn.Linear(4, 3)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), 1.25, -0.5, (g, f1, f2))
    out = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("c_loss", "d_loss", "g_state", "f1_state", "f2_state")}
    assert out["c_loss"].dtype == np.float64 and out["c_loss"].tolist() == [1.25] and out["d_loss"].tolist() == [-0.5]
    whole = torch.cat([t.detach().reshape(-1).float() for t in g.state_dict().values() if t.dtype.is_floating_point]).numpy()
    assert whole.size > 1000 and out["g_state"].dtype == np.float32 and out["g_state"].size == 1000
    assert np.isin(out["g_state"], whole).all()
    want = torch.cat([f1.weight.detach().reshape(-1), f1.bias.detach()]).numpy()
    assert np.array_equal(out["f1_state"], want)
    for n in out:
        assert np.array_equal(out[n], np.load(str(tmp_path / "b" / (n + ".npy"))))


def test_bench_refuses_zero_steps():
    r = _run(["--gpus", "1", "--steps", "0"], {})
    assert r.returncode != 0 and "--steps" in r.stderr
