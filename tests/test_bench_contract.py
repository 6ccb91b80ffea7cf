"""bench.py driver contract: one JSON line from rank 0 with the BASELINE
metric/config keys — the round driver parses exactly this (BENCH_rNN /
SCALE_rNN)."""
import json
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]


def _run(args, timeout=420):
    r = subprocess.run([sys.executable, str(REPO / "bench.py"), *args],
                       capture_output=True, text=True, timeout=timeout,
                       cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_json_contract_cpu():
    d = _run(["--steps", "2", "--warmup", "1", "--n-envs", "32",
              "--rollout", "8"])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "phases_ms"):
        assert key in d, key
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["dtype"] == "bf16" and d["data"] == "synthetic"
    cfg = d["config"]
    for key in ("model", "global_batch", "seq_len", "parallelism",
                "n_envs_per_gpu", "rollout_steps", "obs_dim", "preprocessor",
                "reward", "strategy", "pairs"):
        assert key in cfg, key
    assert cfg["parallelism"] == "dp1"
    assert d["value"] > 0 and d["ms_per_step"] > 0


DUMP_NAMES = ("params", "adam_m", "adam_v", "bootstrap_value",
              "actions", "logp", "values", "rewards", "dones", "advantages",
              "returns", "obs")


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last timed update's arrays as float32
    .npy; the same arguments give the same arrays, and --steps sets how
    many updates were timed (Adam has taken steps+warmup updates' worth of
    minibatch steps, visible in the parameters)."""
    import numpy as np

    base = ["--warmup", "1", "--n-envs", "32", "--rollout", "8"]
    dirs = [tmp_path / "a", tmp_path / "b", tmp_path / "c"]
    da = _run([*base, "--steps", "2", "--dump-outputs", str(dirs[0])])
    _run([*base, "--steps", "2", "--full", "--dump-outputs", str(dirs[1])])
    _run([*base, "--steps", "3", "--dump-outputs", str(dirs[2])])
    assert da["steps"] == 2
    total = 0
    for name in DUMP_NAMES:
        a = np.load(dirs[0] / f"{name}.npy")
        b = np.load(dirs[1] / f"{name}.npy")
        assert a.dtype == np.float32, name
        assert np.isfinite(a).all(), name
        assert np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 * 1000 * 1000
    assert np.load(dirs[0] / "obs.npy").shape == (8 * 32, da["config"]["obs_dim"])
    assert np.load(dirs[0] / "actions.npy").shape == (8 * 32,)
    # one more timed update moves the parameters
    assert not np.array_equal(np.load(dirs[0] / "params.npy"),
                              np.load(dirs[2] / "params.npy"))


def test_bench_dump_outputs_sampling(tmp_path, monkeypatch):
    """Past the byte budget the rollout arrays become a fixed seeded sample
    of (t, env) rows: same rows for every array, indices written alongside,
    total size within the budget, values equal to the trainer's buffers."""
    import importlib.util

    import numpy as np
    import torch

    from gymfx_amd import build_vec_environment
    from gymfx_amd.algo.ppo import PPOConfig, PPOTrainer
    from gymfx_amd.config import DEFAULT_VALUES

    spec = importlib.util.spec_from_file_location("_bench_mod", REPO / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    env = build_vec_environment({
        **DEFAULT_VALUES, "data_feed_plugin": "synthetic_data_feed",
        "synthetic_rows": 600, "n_envs": 16, "device": "cpu",
        "autoreset": True, "env_start_mode": "spread", "seed": 3})
    env.reset(seed=3)
    tr = PPOTrainer(env, PPOConfig(rollout_steps=8, minibatches=2,
                                   ppo_epochs=1, seed=3))
    tr.train_update(with_stats=False)
    n_state = 3 * tr.model.params.numel() + tr.N
    budget = 4 * n_state + 6000
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", budget)
    for d in ("a", "b"):
        bench.dump_outputs(tr, str(tmp_path / d))
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert "rows_small.npy" in files and "rows_obs.npy" in files
    assert sum(np.load(tmp_path / "a" / f).nbytes for f in files) <= budget
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f),
                              np.load(tmp_path / "b" / f)), f
    rows = np.load(tmp_path / "a" / "rows_small.npy").astype(np.int64)
    assert 0 < len(rows) < tr.T * tr.N and (np.diff(rows) > 0).all()
    adv = tr.adv_buf.reshape(-1).numpy()
    assert np.array_equal(np.load(tmp_path / "a" / "advantages.npy"), adv[rows])
    rows_o = np.load(tmp_path / "a" / "rows_obs.npy").astype(np.int64)
    obs = tr.obs_flat.to(torch.float32).numpy()
    assert np.array_equal(np.load(tmp_path / "a" / "obs.npy"), obs[rows_o])


def test_bench_lstm_variant_contract():
    d = _run(["--steps", "1", "--warmup", "0", "--n-envs", "16",
              "--rollout", "16", "--policy", "lstm"])
    assert "LSTM" in d["config"]["model"]
    assert d["config"]["reward"] == "dd_penalized_reward"
    assert d["config"]["strategy"] == "direct_atr_sltp"


def test_bench_torchrun_ws2_contract():
    """The driver's exact SCALE invocation shape (torch.distributed.run,
    nnodes=1, nproc-per-node N, 127.0.0.1 rendezvous): rank 0 prints ONE
    JSON line, parallelism reflects the world size, and the run exits 0
    on the gloo fallback here (nccl=RCCL path on a GPU box).  With GPUs
    present but fewer than the two ranks need, rank 1 has no device of its
    own, so the ranks are pinned to the CPU/gloo path instead."""
    import socket

    import torch

    n_gpu = torch.cuda.device_count() if torch.cuda.is_available() else 0
    device_args = ["--device", "cpu"] if n_gpu == 1 else []
    for attempt in range(2):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        r = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
             "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
             "--master-port", str(port), str(REPO / "bench.py"),
             "--gpus", "2", "--steps", "2", "--warmup", "1",
             "--n-envs", "32", "--rollout", "8", *device_args],
            capture_output=True, text=True, timeout=420, cwd=REPO)
        if r.returncode == 0:
            break
        # the freed port can be re-taken before torchrun binds it — one
        # retry on a fresh port removes that flake from the CI path
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["config"]["parallelism"] == "dp2"
    assert d["value"] > 0
