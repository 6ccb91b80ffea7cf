"""Fused head forward / PPO loss backward / head backward
(PPOConfig.fused_head_bwd, api.head_loss_bwd) — bit-equivalence.

One kernel (head_loss_bwd_kernel) stands for four launches on the head
layer of every minibatch step: the head GEMM, ppo_loss_bwd, the W3 wgrad
partials and the head dgrad.  The reference is always that launch sequence,
called through ``api`` on the same inputs; head, dhead, dh2, the W3/b3 slab
partials and the reduced gradients must be BITWISE equal.  The five logging
sums are order-dependent atomics in both paths and are held to the
tolerance the trainer tests already use across equivalent paths."""
import pytest
import torch

gpu = pytest.mark.gpu

HIDDEN = 256
CLIP_EPS, ENT_COEF, VF_COEF = 0.2, 0.01, 0.5
LOSS_TOL = dict(rtol=1e-5, atol=1e-6)

# (M, slabs, head_dim)
_SHAPES = {
    "two_full_slabs": (256, 2, 4),     # flagship geometry: 128-row slabs
    "single_block": (128, 1, 4),
    "partial_chunks": (300, 3, 4),     # m_per_slab 100: chunks 32,32,32,4
    "ragged_last_slab": (190, 3, 4),   # m_per_slab 64: last slab 62 rows
    "one_chunk_per_slab": (64, 2, 4),  # m_per_slab 32
    "head_dim_3": (256, 2, 3),
    "head_dim_8": (256, 2, 8),
    "refused_big_slab": (512, 2, 4),   # m_per_slab 256 > 128: four launches
}


def _inputs(M, slabs, hd, dev):
    """Random h2 in (-1, 1), W3/b3 at init scale, both advantage signs and
    ratios on both sides of the clip range."""
    g = torch.Generator(device=dev).manual_seed(1000 * M + 10 * slabs + hd)

    def rand(*shape):
        return torch.rand(*shape, device=dev, generator=g)

    bound = 1.0 / HIDDEN ** 0.5
    h2 = (rand(M, HIDDEN) * 2 - 1).to(torch.bfloat16)
    W3 = ((rand(HIDDEN, hd) * 2 - 1) * bound).to(torch.bfloat16)
    W3t = W3.t().contiguous()
    b3 = (rand(hd) * 2 - 1) * bound
    actions = torch.randint(0, hd - 1, (M,), device=dev, generator=g)
    # logp near the uniform policy's, +-0.5: ratios from ~0.6 to ~1.6
    old_logp = -torch.log(torch.tensor(float(hd - 1))) + (rand(M) - 0.5)
    adv = torch.randn(M, device=dev, generator=g)
    ret = torch.randn(M, device=dev, generator=g)
    return h2, W3t, W3, b3, actions, old_logp, adv, ret


def _outputs(M, slabs, hd, dev):
    return dict(
        head=torch.full((M, hd), float("nan"), device=dev),
        dhead=torch.full((M, hd), float("nan"), device=dev,
                         dtype=torch.bfloat16),
        dh2=torch.full((M, HIDDEN), float("nan"), device=dev,
                       dtype=torch.bfloat16),
        dW_part=torch.full((slabs, HIDDEN, hd), float("nan"), device=dev),
        db_part=torch.full((slabs, hd), float("nan"), device=dev),
        dW=torch.full((HIDDEN, hd), float("nan"), device=dev),
        db=torch.full((hd,), float("nan"), device=dev),
        losses=torch.zeros(5, device=dev),
    )


def _four_launches(inp, out, slabs, M, reduce=True):
    from gymfx_amd.ops import api

    h2, W3t, W3, b3, actions, old_logp, adv, ret = inp
    api.gemm(h2, W3t, b3, out["head"], act=0, trans_b=True)
    api.ppo_loss_bwd(out["head"], actions, old_logp, adv, ret, out["dhead"],
                     clip_eps=CLIP_EPS, ent_coef=ENT_COEF, vf_coef=VF_COEF,
                     inv_count=1.0 / M, losses=out["losses"])
    api.wgrad(h2, out["dhead"], out["dW"], out["db"],
              workspace=(out["dW_part"], out["db_part"]), slabs=slabs,
              reduce=reduce)
    api.gemm(out["dhead"], W3, None, out["dh2"], Yact=h2, trans_b=True, act=1,
             dact_tanh=True)


def _fused(inp, out, slabs, M, reduce=True, losses=True):
    from gymfx_amd.ops import api

    api.head_loss_bwd(
        *inp, out["head"], out["dhead"], out["dh2"], out["dW"], out["db"],
        workspace=(out["dW_part"], out["db_part"]), slabs=slabs, reduce=reduce,
        clip_eps=CLIP_EPS, ent_coef=ENT_COEF, vf_coef=VF_COEF,
        inv_count=1.0 / M, losses=out["losses"] if losses else None)


_ref_cache = {}


def _reference(name):
    """Inputs and the four-launch outputs, computed once per shape and
    shared; nobody writes to them afterwards."""
    if name not in _ref_cache:
        M, slabs, hd = _SHAPES[name]
        dev = torch.device("cuda")
        inp = _inputs(M, slabs, hd, dev)
        out = _outputs(M, slabs, hd, dev)
        _four_launches(inp, out, slabs, M)
        torch.cuda.synchronize()
        _ref_cache[name] = (inp, out)
    return _ref_cache[name]


def _assert_bitwise(got, ref, names):
    for nm in names:
        assert torch.equal(got[nm], ref[nm]), nm


_BITWISE = ("head", "dhead", "dh2", "dW_part", "db_part", "dW", "db")


@gpu
@pytest.mark.parametrize("name", list(_SHAPES))
def test_fused_equals_four_launches(name):
    from gymfx_amd.ops import api

    M, slabs, hd = _SHAPES[name]
    inp, ref = _reference(name)
    m_per_slab = -(-M // slabs)
    fusable = api.head_loss_bwd_fusable(M, HIDDEN, hd, slabs)
    assert fusable == (name != "refused_big_slab")
    assert fusable == (m_per_slab <= 128)
    if name == "ragged_last_slab":
        # m_end = min(M, ...) really clips the last slab
        assert slabs * m_per_slab > M > (slabs - 1) * m_per_slab
    if name == "partial_chunks":
        assert m_per_slab % 32 == 4

    # the inputs take both branches of g_lp and of `clipped`
    h2, W3t, W3, b3, actions, old_logp, adv, ret = inp
    logits = ref["head"][:, :hd - 1]
    lp = torch.log_softmax(logits, dim=1).gather(
        1, actions.unsqueeze(1)).squeeze(1)
    ratio = (lp - old_logp).exp()
    clipped = (ratio > 1 + CLIP_EPS) | (ratio < 1 - CLIP_EPS)
    surr1 = ratio * adv
    surr2 = ratio.clamp(1 - CLIP_EPS, 1 + CLIP_EPS) * adv
    active = surr1 <= surr2
    assert bool((adv > 0).any()) and bool((adv < 0).any())
    assert bool(clipped.any()) and bool((~clipped).any())
    assert bool(active.any()) and bool((~active).any())

    out = _outputs(M, slabs, hd, h2.device)
    _fused(inp, out, slabs, M)
    _assert_bitwise(out, ref, _BITWISE)
    assert torch.allclose(out["losses"], ref["losses"], **LOSS_TOL)
    assert float(ref["losses"].abs().sum()) > 0


@gpu
def test_fused_reduce_off_leaves_grads_and_skips_losses():
    """reduce=False (fused optimizer tail): only the partials are written;
    losses=None: the logging sums are skipped, nothing else changes."""
    name = "partial_chunks"
    M, slabs, hd = _SHAPES[name]
    inp, ref = _reference(name)
    out = _outputs(M, slabs, hd, inp[0].device)
    out["dW"].fill_(7.0)
    out["db"].fill_(7.0)
    _fused(inp, out, slabs, M, reduce=False, losses=False)
    _assert_bitwise(out, ref, ("head", "dhead", "dh2", "dW_part", "db_part"))
    assert bool((out["dW"] == 7.0).all()) and bool((out["db"] == 7.0).all())
    assert bool((out["losses"] == 0).all())


@gpu
@pytest.mark.parametrize("name", ["partial_chunks", "refused_big_slab"])
def test_sharded_logging_sums(name):
    """losses as [S, 32] shards: block b adds into row b % S, columns 0..4
    (the four-launch path into row 0); the rows sum to the [5] result."""
    M, slabs, hd = _SHAPES[name]
    inp, ref = _reference(name)
    out = _outputs(M, slabs, hd, inp[0].device)
    out["losses"] = torch.zeros(2, 32, device=inp[0].device)
    _fused(inp, out, slabs, M)
    _assert_bitwise(out, ref, _BITWISE)
    sh = out["losses"]
    assert bool((sh[:, 5:] == 0).all())
    assert torch.allclose(sh[:, :5].sum(dim=0), ref["losses"], **LOSS_TOL)
    if name == "partial_chunks":  # three blocks: rows 0 and 1 both used
        assert bool((sh[:, 4] + sh[:, 2] != 0).all())
    else:
        assert bool((sh[1] == 0).all())


@gpu
def test_fused_more_slabs_than_rows():
    """Trainer-test geometry (tiny minibatch, 512 slabs): two-row slabs and
    empty slabs past M, whose partials must be written as zeros."""
    from gymfx_amd.ops import api

    M, slabs, hd = 200, 128, 4   # m_per_slab 2: slabs 100.. are empty
    dev = torch.device("cuda")
    inp = _inputs(M, slabs, hd, dev)
    ref = _outputs(M, slabs, hd, dev)
    out = _outputs(M, slabs, hd, dev)
    _four_launches(inp, ref, slabs, M)
    assert api.head_loss_bwd_fusable(M, HIDDEN, hd, slabs)
    _fused(inp, out, slabs, M)
    _assert_bitwise(out, ref, _BITWISE)
    assert bool((out["dW_part"][100:] == 0).all())
    assert torch.allclose(out["losses"], ref["losses"], **LOSS_TOL)


# ---------------------------------------------------------------------------
# trainers
# ---------------------------------------------------------------------------

def _make_trainer(fused_head, fused_tail, *, shuffle=True, use_graphs=True):
    from gymfx_amd import build_vec_environment
    from gymfx_amd.algo.ppo import PPOConfig, PPOTrainer
    from gymfx_amd.data.feed import synthetic_ohlcv

    md = synthetic_ohlcv(2000, seed=5, vol=4e-4, extra_feature_columns=3)
    cfg = {
        "n_envs": 64,
        "device": "cuda",
        "window_size": 16,
        "preprocessor_plugin": "feature_window_preprocessor",
        "feature_columns": ["OPEN", "HIGH", "LOW", "CLOSE",
                            "FEAT_0", "FEAT_1", "FEAT_2"],
        "env_start_mode": "spread",
        "autoreset": True,
        "position_size": 1000.0,
        "seed": 3,
    }
    env = build_vec_environment(cfg, md)
    env.reset(seed=3)
    pc = PPOConfig(rollout_steps=16, minibatches=2, ppo_epochs=2, seed=3,
                   use_graphs=use_graphs, shuffle_rows=shuffle,
                   fused_opt_tail=fused_tail, fused_head_bwd=fused_head)
    return PPOTrainer(env, pc)


def _assert_trainers_equal(tf, tu):
    for nm in ("params", "m", "v", "grads", "params_bf16", "adam_ctr"):
        assert torch.equal(getattr(tf.model, nm), getattr(tu.model, nm)), nm
    for nm in ("obs_buf", "act_buf", "logp_buf", "val_buf", "rew_buf",
               "done_buf", "adv_buf", "ret_buf"):
        assert torch.equal(getattr(tf, nm), getattr(tu, nm)), nm
    assert torch.equal(tf.acts_train["head"], tu.acts_train["head"])
    assert torch.equal(tf.dhead, tu.dhead)
    assert torch.equal(tf.scratch["dh2"], tu.scratch["dh2"])
    assert torch.allclose(tf.losses, tu.losses, **LOSS_TOL)


@gpu
@pytest.mark.parametrize("fused_tail", [True, False])
@pytest.mark.parametrize("shuffle", [True, False])
def test_fused_head_equals_unfused_trainer(fused_tail, shuffle):
    tf = _make_trainer(True, fused_tail, shuffle=shuffle)
    tu = _make_trainer(False, fused_tail, shuffle=shuffle)
    assert tf._fused_head and not tu._fused_head
    assert tf.model.fused_tail == fused_tail == tu.model.fused_tail
    for _ in range(2):
        sf = tf.train_update()
        su = tu.train_update()
    torch.cuda.synchronize()
    assert tf._graphs_ready == tu._graphs_ready
    assert tf._graphs_ready or not shuffle
    _assert_trainers_equal(tf, tu)
    for k in su:
        assert sf[k] == pytest.approx(su[k], rel=1e-5, abs=1e-6), k


# ---------------------------------------------------------------------------
# CPU oracle path
# ---------------------------------------------------------------------------

def test_cpu_fallback_equals_composed_fallbacks():
    from gymfx_amd.ops import api

    M, slabs, hd = 96, 2, 4
    dev = torch.device("cpu")
    inp = _inputs(M, slabs, hd, dev)
    h2, W3t, W3, b3, actions, old_logp, adv, ret = inp
    ref = _outputs(M, slabs, hd, dev)
    out = _outputs(M, slabs, hd, dev)
    _four_launches(inp, ref, slabs, M)
    _fused(inp, out, slabs, M)
    for nm in ("head", "dhead", "dh2", "dW", "db", "losses"):
        assert torch.equal(out[nm], ref[nm]), nm
    assert bool(torch.isfinite(out["dh2"].float()).all())


def test_cpu_trainer_knob_is_a_no_op():
    from gymfx_amd import build_vec_environment
    from gymfx_amd.algo.ppo import PPOConfig, PPOTrainer
    from gymfx_amd.data.feed import synthetic_ohlcv

    def make(fused):
        md = synthetic_ohlcv(600, seed=5, vol=4e-4)
        cfg = {"n_envs": 16, "device": "cpu", "window_size": 8,
               "env_start_mode": "spread", "autoreset": True,
               "position_size": 1000.0, "seed": 11}
        env = build_vec_environment(cfg, md)
        env.reset(seed=11)
        pc = PPOConfig(rollout_steps=16, minibatches=2, ppo_epochs=2, seed=11,
                       hidden=32, fused_head_bwd=fused)
        return PPOTrainer(env, pc)

    tf, tu = make(True), make(False)
    for _ in range(2):
        tf.train_update(with_stats=False)
        tu.train_update(with_stats=False)
    assert tf._fused_head and not tu._fused_head
    assert torch.equal(tf.model.params, tu.model.params)
    assert torch.equal(tf.model.m, tu.model.m)
    assert torch.equal(tf.model.v, tu.model.v)
    assert torch.equal(tf.losses, tu.losses)


def test_config_key_maps_to_knob():
    from gymfx_amd.algo.ppo import PPOConfig
    from gymfx_amd.config import DEFAULT_VALUES

    assert DEFAULT_VALUES["fused_head_bwd"] is True
    assert PPOConfig.from_config(dict(DEFAULT_VALUES)).fused_head_bwd is True
    off = PPOConfig.from_config({**DEFAULT_VALUES, "fused_head_bwd": "false"})
    assert off.fused_head_bwd is False
