"""GPU: the seeded probabilistic fill model inside the fused HIP env_step
kernel vs the torch oracle (envs/reference_step.py), plus the properties the
stateless draw buys: off-means-off, determinism, split stepping and hipGraph
replay.  CPU-side semantics live in tests/test_fill_model.py."""
import numpy as np
import pytest
import torch

from gymfx_amd import build_vec_environment
from gymfx_amd.data.feed import synthetic_ohlcv

pytestmark = pytest.mark.gpu

N = 64
STEPS = 220


def _market(pairs=1):
    if pairs == 1:
        return synthetic_ohlcv(2000, seed=5, vol=4e-4, extra_feature_columns=3)
    from gymfx_amd.data.feed import concat_markets
    return concat_markets([
        synthetic_ohlcv(700 + 100 * i, seed=5 + i, vol=4e-4,
                        extra_feature_columns=3, instrument=f"PAIR_{i}")
        for i in range(pairs)
    ])


BASE = {
    "n_envs": N,
    "window_size": 16,
    "initial_cash": 10000.0,
    "position_size": 1000.0,
    "commission": 2e-5,
    "slippage": 1e-5,
    "env_start_mode": "spread",
    "strategy_plugin": "direct_fixed_sltp",
    "autoreset": True,
}

HALF = {"prob_fill_on_limit": 0.5, "prob_fill_on_stop": 0.5,
        "prob_slippage": 0.5, "fill_slip_rate": 2e-5, "fill_random_seed": 11}

CONFIGS = {
    "worst_case": {"intrabar_collision_policy": "worst_case",
                   "sl_pips": 6.0, "tp_pips": 6.0},
    "adaptive_cross": {"intrabar_collision_policy": "adaptive",
                       "limit_fill_policy": "cross",
                       "sl_pips": 6.0, "tp_pips": 6.0},
    "multipair": {"_pairs": 3, "sl_pips": 6.0, "tp_pips": 9.0},
}

_SL, _TP = 15, 16  # exec_diag columns: bracket_sl_fills, bracket_tp_fills


def _actions(rng):
    return torch.from_numpy(rng.integers(0, 3, N))


def oracle_exercises_the_model(name):
    """CPU oracle alone: which fill_diag columns and bracket fill counters
    ever went positive over the run (autoreset zeroes them per episode)."""
    cfg = {**BASE, **HALF, **CONFIGS[name]}
    md = _market(cfg.pop("_pairs", 1))
    env = build_vec_environment({**cfg, "device": "cpu"}, md)
    env.reset(seed=0)
    rng = np.random.default_rng(9)
    seen_fill = torch.zeros(3, dtype=torch.bool)
    seen_br = torch.zeros(2, dtype=torch.bool)
    for _ in range(STEPS):
        env.step(_actions(rng))
        seen_fill |= (env.st.fill_diag > 0).any(dim=0)
        seen_br |= (env.st.exec_diag[:, [_SL, _TP]] > 0).any(dim=0)
    return seen_fill, seen_br


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_kernel_matches_torch_oracle_with_fill_model(name):
    seen_fill, seen_br = oracle_exercises_the_model(name)
    assert bool(seen_fill.all()), (name, seen_fill)
    assert bool(seen_br.all()), (name, seen_br)

    cfg = {**BASE, **HALF, **CONFIGS[name]}
    md = _market(cfg.pop("_pairs", 1))
    env_g = build_vec_environment({**cfg, "device": "cuda"}, md, use_native=True)
    env_c = build_vec_environment({**cfg, "device": "cuda"}, md, use_native=False)
    assert env_g.params.fill_model_on
    env_g.reset(seed=0)
    env_c.reset(seed=0)
    rng = np.random.default_rng(9)
    for k in range(STEPS):
        a = _actions(rng).cuda()
        out_g = env_g.step(a)
        out_c = env_c.step(a)
        torch.cuda.synchronize()
        for fld in ("equity", "cash", "pos", "avg_entry", "commission_paid"):
            g = getattr(env_g.st, fld).cpu().numpy()
            c = getattr(env_c.st, fld).cpu().numpy()
            np.testing.assert_allclose(g, c, rtol=1e-9, atol=1e-9,
                                       err_msg=f"{name} step {k} field {fld}")
        np.testing.assert_array_equal(
            env_g.st.cursor.cpu().numpy(), env_c.st.cursor.cpu().numpy())
        np.testing.assert_array_equal(
            env_g.st.terminated.cpu().numpy(), env_c.st.terminated.cpu().numpy())
        np.testing.assert_allclose(
            out_g["reward"].cpu().numpy(),
            out_c["reward"].cpu().float().numpy(),
            rtol=5e-4, atol=1e-6, err_msg=f"{name} step {k} reward")
        np.testing.assert_allclose(
            out_g["obs"].cpu().numpy(), out_c["obs"].cpu().numpy(),
            rtol=3e-5, atol=3e-5, err_msg=f"{name} step {k} obs")
        np.testing.assert_array_equal(
            env_g.st.exec_diag.cpu().numpy(), env_c.st.exec_diag.cpu().numpy(),
            err_msg=f"{name} step {k} exec_diag")
        np.testing.assert_array_equal(
            env_g.st.fill_diag.cpu().numpy(), env_c.st.fill_diag.cpu().numpy(),
            err_msg=f"{name} step {k} fill_diag")


def _trajectory(extra, steps=150, split=False):
    cfg = {**BASE, "sl_pips": 6.0, "tp_pips": 6.0, "device": "cuda", **extra}
    env = build_vec_environment(cfg, _market(), use_native=True)
    env.reset(seed=0)
    rng = np.random.default_rng(3)
    eq = []
    for _ in range(steps):
        a = _actions(rng).cuda()
        if split:
            env.step(a, env_lo=0, env_hi=N // 2)
            env.step(a, env_lo=N // 2, env_hi=N)
        else:
            env.step(a)
        eq.append(env.st.equity.clone())
    return env, torch.stack(eq)


def test_off_means_off():
    """Defaults spelled out == a config that never mentions the keys."""
    plain, eq_p = _trajectory({})
    spelled, eq_s = _trajectory({"prob_fill_on_limit": 1.0,
                                 "prob_fill_on_stop": 1.0,
                                 "prob_slippage": 0.0,
                                 "fill_slip_rate": 2e-5,
                                 "fill_random_seed": 5})
    assert torch.equal(eq_p, eq_s)
    assert torch.equal(plain.st.exec_diag, spelled.st.exec_diag)
    assert int(spelled.st.fill_diag.abs().sum()) == 0


def test_deterministic_and_seed_sensitive():
    e1, eq1 = _trajectory(HALF)
    e2, eq2 = _trajectory(HALF)
    assert torch.equal(eq1, eq2)
    assert torch.equal(e1.st.fill_diag, e2.st.fill_diag)
    assert int(e1.st.fill_diag.sum()) > 0
    e3, _ = _trajectory({**HALF, "fill_random_seed": 12})
    assert not torch.equal(e1.st.fill_diag, e3.st.fill_diag)


def test_split_stepping_uses_the_global_env_index():
    full, eq_f = _trajectory(HALF, steps=100)
    halves, eq_h = _trajectory(HALF, steps=100, split=True)
    assert torch.equal(eq_f, eq_h)
    for fld in ("cash", "pos", "cursor", "exec_diag", "fill_diag"):
        assert torch.equal(getattr(full.st, fld), getattr(halves.st, fld)), fld
    assert int(full.st.fill_diag.sum()) > 0


def _make_trainer(use_graphs):
    from gymfx_amd.algo.ppo import PPOConfig, PPOTrainer

    cfg = {**BASE, **HALF, "sl_pips": 6.0, "tp_pips": 6.0, "device": "cuda",
           "preprocessor_plugin": "feature_window_preprocessor",
           "feature_columns": ["OPEN", "HIGH", "LOW", "CLOSE",
                               "FEAT_0", "FEAT_1", "FEAT_2"],
           "seed": 3}
    env = build_vec_environment(cfg, _market())
    env.reset(seed=3)
    pc = PPOConfig(rollout_steps=8, minibatches=2, ppo_epochs=2, seed=3,
                   hidden=256, use_graphs=use_graphs)
    return PPOTrainer(env, pc)


def test_graph_replay_equals_eager_with_fill_model():
    tg = _make_trainer(use_graphs=True)
    te = _make_trainer(use_graphs=False)
    for _ in range(2):
        tg.train_update(with_stats=False)
        te.train_update(with_stats=False)
    torch.cuda.synchronize()
    assert tg._graphs_ready
    assert torch.equal(tg.model.params, te.model.params)
    assert torch.equal(tg.env.st.equity, te.env.st.equity)
    assert torch.equal(tg.env.st.fill_diag, te.env.st.fill_diag)
    assert int(tg.env.st.fill_diag.sum()) > 0
