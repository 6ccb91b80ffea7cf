"""Seeded probabilistic fill model (prob_fill_on_limit / prob_fill_on_stop /
prob_slippage) in the vectorized engine: the stateless draw hash, its
semantics on the torch oracle, reconciliation against the independent
ScalarLedger at p < 1, the profile/config path and checkpoint
compatibility.  GPU parity for the same model lives in
tests/test_gpu_fill_model.py."""
import json
import math

import numpy as np
import pytest
import torch

from gymfx_amd import build_vec_environment
from gymfx_amd import replay
from gymfx_amd.data.feed import MarketData, synthetic_ohlcv
from gymfx_amd.envs import reference_step
from gymfx_amd.envs.params import EnvParams
from gymfx_amd.replay import ReplayAdapter

M64 = (1 << 64) - 1

# (seed, n, t, ch) -> (key, u53), computed with Python integers
KNOWN = [
    ((0, 0, 0, 0), 0xA706DD2F4D197E6F, 5876733520225071),
    ((3, 0, 2, 1), 0x22B89286290766A2, 1221636082966764),
    ((3, 5, 1234, 2), 0xA11897A7C24B1815, 5668063860509027),
    ((2147483647, 4095, 70000, 3), 0x384FF2456F7DCE19, 1981312582676409),
]


def _oracle_key(seed, n, t, ch):
    k = reference_step.fill_key(seed, torch.tensor([n]), torch.tensor([t]), ch)
    return int(k.item()) & M64


def _oracle_u53(seed, n, t, ch):
    return int(reference_step.fill_u53(
        seed, torch.tensor([n]), torch.tensor([t]), ch).item())


@pytest.mark.parametrize("args,key,u53", KNOWN)
def test_known_answers_oracle_and_ledger(args, key, u53):
    assert _oracle_key(*args) == key
    assert _oracle_u53(*args) == u53
    assert replay.fill_key(*args) == key
    assert replay.fill_u53(*args) == u53


def _grid_draws(seed, ch, n_envs=4096, n_bars=64):
    n = torch.arange(n_envs).repeat_interleave(n_bars)
    t = torch.arange(n_bars).repeat(n_envs)
    return reference_step.fill_u53(seed, n, t, ch)


def test_oracle_hash_equals_python_integers_on_a_grid():
    u = _grid_draws(7, 1, n_envs=64, n_bars=64).tolist()
    want = [replay.fill_u53(7, n, t, 1) for n in range(64) for t in range(64)]
    assert u == want


def test_threshold_edges():
    from gymfx_amd.envs.params import fill_threshold

    u = _grid_draws(11, 0, n_envs=64, n_bars=64)  # 4096 draws
    assert u.numel() == 4096
    assert bool((u < fill_threshold(1.0, "p")).all())
    assert not bool((u < fill_threshold(0.0, "p")).any())
    assert bool((u >= 0).all())


def test_frequency_and_channel_independence():
    p = 0.3
    thr = int(p * 2 ** 53)
    draws = 4096 * 64
    bound = 5.0 * math.sqrt(p * (1 - p) / draws)
    fired = []
    for ch in range(4):
        f = (_grid_draws(5, ch) < thr).to(torch.float64)
        assert f.numel() == draws
        assert abs(float(f.mean()) - p) <= bound, (ch, float(f.mean()))
        fired.append(f)
    for i in range(4):
        for j in range(i + 1, 4):
            corr = float(torch.corrcoef(torch.stack([fired[i], fired[j]]))[0, 1])
            assert abs(corr) < 5.0 / math.sqrt(draws), (i, j, corr)


# ---------------------------------------------------------------------------
# behaviour on the collision fixture of test_execution_realism.py
# ---------------------------------------------------------------------------

def _md(bars):
    arr = np.asarray(bars, dtype=np.float64)
    return MarketData(
        columns={
            "OPEN": arr[:, 0].copy(),
            "HIGH": arr[:, 1].copy(),
            "LOW": arr[:, 2].copy(),
            "CLOSE": arr[:, 3].copy(),
            "VOLUME": np.zeros(len(arr)),
        },
        timestamps=1700000000 + np.arange(len(arr), dtype=np.int64) * 60,
    )


BASE = {
    "n_envs": 1,
    "device": "cpu",
    "window_size": 2,
    "initial_cash": 10000.0,
    "position_size": 100.0,
    "commission": 0.0,
    "slippage": 0.0,
    "strategy_plugin": "direct_fixed_sltp",
    "sl_pips": 50.0,
    "tp_pips": 50.0,
    "pip_size": 0.0001,
}

# entry decided at bar1 (close 1.0, SL 0.995 / TP 1.005), parent fills at
# bar2 open, bar3 touches BOTH children
COLLISION_BARS = [
    (1.0, 1.001, 0.999, 1.0),
    (1.0, 1.001, 0.999, 1.0),
    (1.0, 1.006, 0.994, 1.002),
    (1.0, 1.001, 0.999, 1.0),
    (1.0, 1.001, 0.999, 1.0),
]


def _run(md, actions, **kw):
    cfg = dict(BASE)
    cfg.update(kw)
    env = build_vec_environment(cfg, md)
    env.reset()
    for a in actions:
        env.step(torch.tensor([a]))
    return env


def test_worst_case_with_stop_off_fills_take_profit():
    env = _run(_md(COLLISION_BARS), [1, 0, 0, 0],
               intrabar_collision_policy="worst_case", prob_fill_on_stop=0.0)
    d = env.execution_diagnostics(0)
    f = env.fill_model_diagnostics(0)
    assert d["bracket_tp_fills"] == 1 and d["bracket_sl_fills"] == 0
    assert f["bracket_sl_fill_misses"] >= 1


def test_both_legs_off_never_fill_and_stay_armed():
    env = _run(_md(COLLISION_BARS), [1, 0, 0, 0],
               prob_fill_on_stop=0.0, prob_fill_on_limit=0.0)
    d = env.execution_diagnostics(0)
    f = env.fill_model_diagnostics(0)
    assert d["bracket_tp_fills"] == 0 and d["bracket_sl_fills"] == 0
    assert float(env.st.pos[0]) == 100.0
    assert bool(env.st.br_active[0])
    assert f["bracket_sl_fill_misses"] > 0 and f["bracket_tp_fill_misses"] > 0


def test_certain_slippage_moves_the_entry_fill():
    slip, r = 1e-5, 3e-5
    env = _run(_md(COLLISION_BARS), [1, 0], slippage=slip,
               prob_slippage=1.0, fill_slip_rate=r)
    want = np.float32(1.0) * (np.float32(1.0) + (np.float32(slip) + np.float32(r)))
    assert float(env.st.avg_entry[0]) == float(want)
    assert float(env.st.avg_entry[0]) > 1.0 * (1.0 + slip)
    assert env.fill_model_diagnostics(0)["market_fill_slips"] == 1


def test_preflight_denied_open_does_not_count_as_slip():
    env = _run(_md(COLLISION_BARS), [1, 0], prob_slippage=1.0,
               fill_slip_rate=3e-5, enforce_margin_preflight=True,
               position_size=50000.0, leverage=1.0)
    assert env.execution_diagnostics(0)["margin_preflight_denied"] == 1
    assert env.fill_model_diagnostics(0)["market_fill_slips"] == 0


# ---------------------------------------------------------------------------
# defaults leave the engine untouched
# ---------------------------------------------------------------------------

def _random_run(extra, steps=200, n=8):
    md = synthetic_ohlcv(600, seed=5, vol=4e-4)
    cfg = {"n_envs": n, "device": "cpu", "window_size": 8,
           "initial_cash": 10000.0, "position_size": 1000.0,
           "commission": 2e-5, "slippage": 1e-5, "env_start_mode": "spread",
           "autoreset": True, "strategy_plugin": "direct_fixed_sltp",
           "sl_pips": 6.0, "tp_pips": 6.0, **extra}
    env = build_vec_environment(cfg, md)
    env.reset(seed=0)
    rng = np.random.default_rng(9)
    trail = []
    for _ in range(steps):
        env.step(torch.from_numpy(rng.integers(0, 3, n)))
        trail.append(env.st.equity.clone())
    return env, torch.stack(trail)


def test_defaults_are_bit_identical_and_count_nothing():
    absent, eq_a = _random_run({})
    explicit, eq_e = _random_run({"prob_fill_on_limit": 1.0,
                                  "prob_fill_on_stop": 1.0,
                                  "prob_slippage": 0.0,
                                  "fill_slip_rate": 2e-5,
                                  "fill_random_seed": 17})
    assert not absent.params.fill_model_on
    assert not explicit.params.fill_model_on
    assert torch.equal(eq_a, eq_e)
    for fld in ("equity", "cash", "pos", "exec_diag"):
        assert torch.equal(getattr(absent.st, fld), getattr(explicit.st, fld)), fld
    assert int(absent.st.exec_diag[:, 15:17].sum()) > 0  # brackets did fill
    assert int(absent.st.fill_diag.abs().sum()) == 0
    assert int(explicit.st.fill_diag.abs().sum()) == 0


def test_model_on_changes_the_run_and_counters_reset_with_the_episode():
    off, _ = _random_run({})
    on, _ = _random_run({"prob_fill_on_limit": 0.5, "prob_fill_on_stop": 0.5,
                         "prob_slippage": 0.5, "fill_slip_rate": 2e-5})
    assert on.params.fill_model_on
    assert not torch.equal(off.st.equity, on.st.equity)
    assert bool((on.st.fill_diag.sum(dim=0) > 0).all())
    mask = torch.zeros(on.n_envs, dtype=torch.bool)
    mask[0] = True
    from gymfx_amd.envs.state import reset_state_

    reset_state_(on.st, on.params, mask)
    assert int(on.st.fill_diag[0].abs().sum()) == 0


# ---------------------------------------------------------------------------
# ledger reconciliation at p < 1
# ---------------------------------------------------------------------------

def _walk(seed, n):
    rng = np.random.default_rng(seed)
    o = 1.0 + np.cumsum(rng.normal(0, 8e-4, size=n))
    h = o + np.abs(rng.normal(0, 6e-4, size=n))
    lo = o - np.abs(rng.normal(0, 6e-4, size=n))
    c = np.clip(o + rng.normal(0, 4e-4, size=n), lo, h)
    return _md(list(zip(o, h, lo, c)))


HALF = {"prob_fill_on_limit": 0.5, "prob_fill_on_stop": 0.5,
        "prob_slippage": 0.5, "fill_slip_rate": 2e-5, "fill_random_seed": 3}


def _fixed_case(policy):
    md = _walk(21, 160)
    rng = np.random.default_rng(4)
    actions = [int(a) for a in rng.integers(0, 3, size=150)]
    cfg = {**BASE, **HALF, "intrabar_collision_policy": policy,
           "sl_pips": 8.0, "tp_pips": 8.0, "commission": 2e-5,
           "slippage": 1e-5, "leverage": 20.0}
    return ReplayAdapter().run(cfg, md, actions)


@pytest.fixture(scope="module")
def fixed_results():
    return {pol: _fixed_case(pol) for pol in ("worst_case", "ohlc", "adaptive")}


@pytest.mark.parametrize("policy", ["worst_case", "ohlc", "adaptive"])
def test_ledger_reconciles_at_half_probabilities(fixed_results, policy):
    res = fixed_results[policy]
    assert res["reconciled"], res["reconciliation"]
    assert res["fill_model"]["engine"] == res["fill_model"]["oracle"]


def test_fixed_cases_exercise_the_model(fixed_results):
    misses = [r["fill_model"]["engine"]["bracket_sl_fill_misses"]
              + r["fill_model"]["engine"]["bracket_tp_fill_misses"]
              for r in fixed_results.values()]
    slips = [r["fill_model"]["engine"]["market_fill_slips"]
             for r in fixed_results.values()]
    assert any(m > 0 and s > 0 for m, s in zip(misses, slips)), (misses, slips)


def test_fill_model_cross_product_reconciles_property():
    from hypothesis import given, settings
    from hypothesis import strategies as st

    probs = st.sampled_from([0.0, 0.25, 0.5, 1.0])

    @settings(max_examples=40, deadline=None)
    @given(
        st.sampled_from(["worst_case", "ohlc", "adaptive"]),
        st.sampled_from(["touch", "cross", "conservative"]),
        st.sampled_from([0, 60_000]),
        probs, probs, probs,
        st.integers(min_value=0, max_value=2 ** 31 - 1),
        st.lists(st.integers(min_value=0, max_value=2),
                 min_size=4, max_size=24),
    )
    def check(collision, limit, latency_ms, p_lim, p_stop, p_slip, seed,
              actions):
        md = _walk(seed, max(len(actions) + 6, 16))
        cfg = {**BASE,
               "intrabar_collision_policy": collision,
               "limit_fill_policy": limit,
               "latency_ms": latency_ms,
               "sl_pips": 10.0, "tp_pips": 10.0,
               "commission": 2e-5, "slippage": 1e-5, "leverage": 20.0,
               "prob_fill_on_limit": p_lim, "prob_fill_on_stop": p_stop,
               "prob_slippage": p_slip, "fill_slip_rate": 2e-5,
               "fill_random_seed": seed}
        result = ReplayAdapter().run(cfg, md, actions)
        assert result["reconciled"], (
            collision, limit, latency_ms, p_lim, p_stop, p_slip, seed,
            result["reconciliation"], result["fill_model"])

    check()


# ---------------------------------------------------------------------------
# profile / config path
# ---------------------------------------------------------------------------

PROFILE = {
    "schema_version": "execution_cost_profile.v1", "profile_id": "t",
    "commission_rate_per_side": 2e-5, "full_spread_rate": 1e-4,
    "slippage_bps_per_side": 0.05, "latency_ms": 0,
    "financing_enabled": False,
    "intrabar_collision_policy": "adaptive",
    "limit_fill_policy": "cross", "margin_model": "standard",
    "enforce_margin_preflight": False, "random_seed": 3,
}


def _params_from_profile(tmp_path, prof):
    path = tmp_path / "prof.json"
    path.write_text(json.dumps(prof))
    return EnvParams.from_config({**BASE, "execution_cost_profile": str(path),
                                  "prob_fill_on_stop": 0.1,  # profile wins
                                  "fill_random_seed": 99})


def test_profile_fill_fields_reach_the_engine(tmp_path):
    p = _params_from_profile(tmp_path, {**PROFILE, "prob_fill_on_limit": 0.75,
                                        "prob_fill_on_stop": 0.5,
                                        "prob_slippage": 0.25})
    assert p.fill_model_on
    assert p.fill_thr_limit == 3 * 2 ** 51
    assert p.fill_thr_stop == 2 ** 52
    assert p.fill_thr_slip == 2 ** 51
    assert p.fill_random_seed == 3
    assert p.fill_slip_rate == pytest.approx(0.05 / 10000)


def test_profile_without_fill_fields_gives_defaults(tmp_path):
    p = _params_from_profile(tmp_path, PROFILE)
    assert not p.fill_model_on
    assert (p.fill_thr_limit, p.fill_thr_stop, p.fill_thr_slip) == (2 ** 53, 2 ** 53, 0)
    assert (p.prob_fill_on_limit, p.prob_fill_on_stop, p.prob_slippage) == (1.0, 1.0, 0.0)


@pytest.mark.parametrize("field,value", [("prob_fill_on_limit", 1.5),
                                         ("prob_fill_on_stop", -0.1),
                                         ("prob_slippage", 2.0)])
def test_out_of_range_probability_raises(tmp_path, field, value):
    with pytest.raises(ValueError):
        EnvParams.from_config({**BASE, field: value})
    with pytest.raises(ValueError):
        _params_from_profile(tmp_path, {**PROFILE, field: value})


def test_target_replay_default_fill_model_reads_the_profile():
    from gymfx_amd.contracts import ExecutionCostProfile
    from gymfx_amd.target_replay import TargetReplay

    plain = TargetReplay(ExecutionCostProfile.from_dict(PROFILE)).fill
    assert (plain.prob_fill_on_limit, plain.prob_fill_on_stop,
            plain.prob_slippage) == (1.0, 1.0, 0.0)
    tuned = TargetReplay(ExecutionCostProfile.from_dict(
        {**PROFILE, "prob_fill_on_stop": 0.5, "prob_slippage": 0.25})).fill
    assert (tuned.random_seed, tuned.prob_fill_on_stop,
            tuned.prob_slippage) == (3, 0.5, 0.25)


def test_example_profile_turns_the_model_on():
    import os

    path = os.path.join(os.path.dirname(__file__), "..", "examples", "config",
                        "execution_cost_profiles", "uncertain_fills.json")
    p = EnvParams.from_config({**BASE, "execution_cost_profile": path})
    assert p.fill_model_on and p.fill_thr_stop < 2 ** 53


# ---------------------------------------------------------------------------
# checkpoints written before fill_diag existed
# ---------------------------------------------------------------------------

def test_checkpoint_without_fill_diag_loads_with_zero_counters():
    from gymfx_amd.algo.ppo import PPOConfig, PPOTrainer
    from gymfx_amd.utils.checkpoint import (load_trainer_state_dict,
                                            trainer_state_dict)

    def make():
        md = synthetic_ohlcv(600, seed=6, vol=4e-4)
        cfg = {"n_envs": 16, "device": "cpu", "window_size": 8,
               "env_start_mode": "spread", "autoreset": True,
               "position_size": 1000.0, "seed": 31,
               "strategy_plugin": "direct_fixed_sltp",
               "sl_pips": 6.0, "tp_pips": 6.0, **HALF}
        env = build_vec_environment(cfg, md)
        env.reset(seed=31)
        return PPOTrainer(env, PPOConfig(rollout_steps=8, minibatches=2,
                                         ppo_epochs=1, seed=31, hidden=16))

    src = make()
    src.train_update(with_stats=False)
    sd = trainer_state_dict(src)
    assert "fill_diag" in sd["env_state"]
    del sd["env_state"]["fill_diag"]  # what an older checkpoint looks like
    dst = make()
    load_trainer_state_dict(dst, sd)
    assert torch.equal(dst.env.st.equity, src.env.st.equity)
    assert int(dst.env.st.fill_diag.abs().sum()) == 0
    dst.train_update(with_stats=False)  # and it keeps training
