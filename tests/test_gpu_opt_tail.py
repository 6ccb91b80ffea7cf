"""Fused reduce/optimizer tail (PPOConfig.fused_opt_tail) — bit-equivalence.

The per-minibatch tail used to be 13 launches (six slab reduces, sumsq,
Adam, adam_ctr increment, three mirror transposes, mb_ctr increment).  The
fused path is grads_finalize + adam_tail, with the adam_ctr advance folded
into the Adam kernel; the in-gather mb_ctr advance (GYMFX_GATHER_TICKET=1)
and the LSTM wiring (GYMFX_LSTM_OPT_TAIL=1) measured slower and are opt-in,
but are held to the same contract here.  Every result must be BITWISE what
the unfused sequence produces: the existing kernels are the reference."""
import pytest
import torch

gpu = pytest.mark.gpu


def _dev():
    return torch.device("cuda")


# ---------------------------------------------------------------------------
# 1. grads_finalize vs the reduce kernels inside wgrad
# ---------------------------------------------------------------------------

# (K, N, slabs): every branch of the reduce dispatch
_SHAPES = [
    (260, 256, 128),  # vector path, flagship W1, elems % 4 == 0; bias N=256
    (256, 4, 512),    # small tree, 512 slabs (> 256 per tree); bias N=4
    (67, 63, 5),      # > 4096 elems, elems % 4 == 1, slabs % 4 == 1
    (7, 5, 3),        # tiny small tree
]

_ref_cache = {}


def _wgrad_ref(shape):
    """Native wgrad with its own reduce: (dW_part, db_part, dW_ref, db_ref).
    Computed once per shape and shared; nobody writes to it afterwards."""
    if shape not in _ref_cache:
        from gymfx_amd.ops import api

        K, N, slabs = shape
        M = 64 * slabs
        g = torch.Generator(device="cuda").manual_seed(K * 1000 + N)
        X = torch.randn(M, K, device=_dev(), generator=g).to(torch.bfloat16)
        dY = torch.randn(M, N, device=_dev(), generator=g).to(torch.bfloat16)
        dW_part = torch.empty(slabs, K, N, dtype=torch.float32, device=_dev())
        db_part = torch.empty(slabs, N, dtype=torch.float32, device=_dev())
        dW = torch.empty(K, N, dtype=torch.float32, device=_dev())
        db = torch.empty(N, dtype=torch.float32, device=_dev())
        api.wgrad(X, dY, dW, db, workspace=(dW_part, db_part), slabs=slabs)
        torch.cuda.synchronize()
        _ref_cache[shape] = (dW_part, db_part, dW, db)
    return _ref_cache[shape]


@gpu
@pytest.mark.parametrize("shape", _SHAPES)
def test_finalize_equals_wgrad_reduce(shape):
    from gymfx_amd.ops import api

    K, N, slabs = shape
    dW_part, db_part, dW_ref, db_ref = _wgrad_ref(shape)
    flat = torch.full((K * N + N,), float("nan"), device=_dev())
    api.grads_finalize([(dW_part, K * N, slabs, 0, False),
                        (db_part, N, slabs, K * N, True)], flat)
    assert torch.equal(flat[:K * N].view(K, N), dW_ref)
    assert torch.equal(flat[K * N:], db_ref)


@gpu
def test_finalize_leaves_workspace_unreduced_when_reduce_off():
    """wgrad(reduce=False) fills the same partials and launches no reduce:
    dW/db keep their old contents, finalize then gives the reference."""
    from gymfx_amd.ops import api

    K, N, slabs = 67, 63, 5
    M = 64 * slabs
    g = torch.Generator(device="cuda").manual_seed(K * 1000 + N)
    X = torch.randn(M, K, device=_dev(), generator=g).to(torch.bfloat16)
    dY = torch.randn(M, N, device=_dev(), generator=g).to(torch.bfloat16)
    dW_part_ref, db_part_ref, dW_ref, db_ref = _wgrad_ref((K, N, slabs))
    dW_part = torch.empty_like(dW_part_ref)
    db_part = torch.empty_like(db_part_ref)
    dW = torch.full((K, N), 7.0, device=_dev())
    db = torch.full((N,), 7.0, device=_dev())
    api.wgrad(X, dY, dW, db, workspace=(dW_part, db_part), slabs=slabs,
              reduce=False)
    assert torch.equal(dW_part, dW_part_ref)
    assert torch.equal(db_part, db_part_ref)
    assert bool((dW == 7.0).all()) and bool((db == 7.0).all())
    flat = torch.empty(K * N + N, device=_dev())
    api.grads_finalize([(dW_part, K * N, slabs, 0, False),
                        (db_part, N, slabs, K * N, True)], flat)
    assert torch.equal(flat[:K * N].view(K, N), dW_ref)
    assert torch.equal(flat[K * N:], db_ref)


@gpu
def test_finalize_many_segments_with_offsets():
    """All shapes in ONE table, in shuffled order with a gap the table does
    not cover: offsets are honoured and the gap keeps its contents."""
    from gymfx_amd.ops import api

    segs, expect = [], []
    off = 3  # leading gap
    for shape in (_SHAPES[2], _SHAPES[0], _SHAPES[3], _SHAPES[1]):
        K, N, slabs = shape
        dW_part, db_part, dW_ref, db_ref = _wgrad_ref(shape)
        segs.append((db_part, N, slabs, off, True))
        expect.append((off, db_ref.reshape(-1)))
        off += N
        segs.append((dW_part, K * N, slabs, off, False))
        expect.append((off, dW_ref.reshape(-1)))
        off += K * N + 1  # one-element gap after every weight
    flat = torch.full((off,), -5.0, device=_dev())
    api.grads_finalize(segs, flat)
    covered = torch.zeros(off, dtype=torch.bool, device=_dev())
    for o, ref in expect:
        assert torch.equal(flat[o:o + ref.numel()], ref)
        covered[o:o + ref.numel()] = True
    assert bool((flat[~covered] == -5.0).all())


# ---------------------------------------------------------------------------
# 2. fused norm partials vs the sumsq launch
# ---------------------------------------------------------------------------

def _random_segments(layout, slabs_big, slabs_small, seed):
    """layout: [(K, N) weight followed by its N-bias] laid out MLP-style."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    segs, off = [], 0
    for K, N in layout:
        S = slabs_big if K * N > 4096 else slabs_small
        wp = torch.randn(S, K * N, device=_dev(), generator=g)
        bp = torch.randn(S, N, device=_dev(), generator=g)
        segs.append((wp, K * N, S, off, False))
        off += K * N
        segs.append((bp, N, S, off, True))
        off += N
    return segs, off


@gpu
@pytest.mark.parametrize("case", ["mlp_133636", "n_300"])
def test_finalize_norm_partials_equal_sumsq_launch(case):
    from gymfx_amd.ops import api

    if case == "mlp_133636":
        # flagship parameter count: three-deep j loop in every partial
        segs, n = _random_segments([(260, 256), (256, 256), (256, 4)], 8, 5, 1)
        assert n == 133636
        flat = torch.empty(n, device=_dev())
    else:
        # most partials are zero; the tail of the buffer is not covered by
        # any segment and must enter the norm with the value it has
        segs, used = _random_segments([(7, 5), (20, 10)], 3, 3, 2)
        n = 300
        assert used < n
        flat = torch.randn(n, device=_dev())
    part = torch.full((256,), float("nan"), device=_dev())
    api.grads_finalize(segs, flat, clip_part=part)
    # reference: per-segment reduce by the unfused finalize path is covered
    # above; here the partials of the SAME buffer by the sumsq launch
    part_ref = torch.empty(256, device=_dev())
    scale = torch.empty(1, device=_dev())
    api.grad_clip_scale(flat, 0.5, part_ref, scale)
    assert torch.equal(part, part_ref)
    # and the gradients are the ones the no-partials launch writes
    flat2 = flat.clone() if case == "n_300" else torch.empty(n, device=_dev())
    api.grads_finalize(segs, flat2)
    assert torch.equal(flat, flat2)


# ---------------------------------------------------------------------------
# 3. adam_tail vs adam + increment + transposes
# ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("max_norm", [0.0, 0.05])
def test_adam_tail_equals_adam_increment_transpose(max_norm):
    from gymfx_amd.ops import api

    layout = [(260, 256), (256, 4), (20, 64)]
    offs, off = [], 0
    for K, N in layout:
        offs.append(off)
        off += K * N + N  # weight then its bias
    n = off
    g = torch.Generator(device="cuda").manual_seed(42)

    def state():
        gg = torch.Generator(device="cuda").manual_seed(43)
        p = torch.randn(n, device=_dev(), generator=gg) * 0.1
        m = torch.randn(n, device=_dev(), generator=gg) * 0.01
        v = torch.rand(n, device=_dev(), generator=gg) * 1e-3
        pb = p.to(torch.bfloat16)
        mir = [torch.zeros(N, K, dtype=torch.bfloat16, device=_dev())
               for K, N in layout]
        ctr = torch.zeros((), dtype=torch.int32, device=_dev())
        part = torch.zeros(256, device=_dev())
        return p, m, v, pb, mir, ctr, part

    pr, mr, vr, pbr, mirr, ctrr, partr = state()
    pn, mn, vn, pbn, mirn, ctrn, partn = state()
    ticket = torch.zeros((), dtype=torch.int32, device=_dev())
    for step in range(3):
        grad = torch.randn(n, device=_dev(), generator=g)
        clip_r = (partr, max_norm) if max_norm > 0 else None
        clip_n = (partn, max_norm) if max_norm > 0 else None
        api.adam(pr, grad, mr, vr, pbr, lr=3e-4, step=step + 1, step_ctr=ctrr,
                 clip=clip_r)
        api.increment_counter(ctrr, 1)
        for (K, N), o, t in zip(layout, offs, mirr):
            api.transpose_bf16(pbr[o:o + K * N].view(K, N), t)
        api.adam_tail(pn, grad, mn, vn, pbn, lr=3e-4, step_ctr=ctrn,
                      ticket=ticket, clip=clip_n,
                      mirrors=list(zip(offs, mirn)))
        assert int(ctrn.item()) == step + 1 == int(ctrr.item())
        assert int(ticket.item()) == 0
        assert torch.equal(pn, pr)
        assert torch.equal(mn, mr)
        assert torch.equal(vn, vr)
        assert torch.equal(pbn, pbr)
        for a, b in zip(mirn, mirr):
            assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# trainers
# ---------------------------------------------------------------------------

def _make_trainer(fused, *, policy="mlp", hidden=256, use_graphs=True,
                  max_grad_norm=0.5, seed=3):
    from gymfx_amd import build_vec_environment
    from gymfx_amd.algo.ppo import PPOConfig, PPOTrainer
    from gymfx_amd.data.feed import synthetic_ohlcv

    md = synthetic_ohlcv(2000, seed=5, vol=4e-4, extra_feature_columns=3)
    cfg = {
        "n_envs": 256,
        "device": "cuda",
        "window_size": 16,
        "preprocessor_plugin": "feature_window_preprocessor",
        "feature_columns": ["OPEN", "HIGH", "LOW", "CLOSE",
                            "FEAT_0", "FEAT_1", "FEAT_2"],
        "env_start_mode": "spread",
        "autoreset": True,
        "position_size": 1000.0,
        "seed": seed,
    }
    env = build_vec_environment(cfg, md)
    env.reset(seed=seed)
    pc = PPOConfig(rollout_steps=16, minibatches=4, ppo_epochs=2, seed=seed,
                   policy=policy, bptt_len=4, hidden=hidden,
                   use_graphs=use_graphs, max_grad_norm=max_grad_norm,
                   fused_opt_tail=fused)
    return PPOTrainer(env, pc)


# 4. counters ---------------------------------------------------------------

@gpu
@pytest.mark.parametrize("policy", ["mlp", "lstm"])
def test_gather_advances_mb_ctr_in_kernel(policy, monkeypatch):
    # the in-gather advance is opt-in (measured slower at the flagship shape)
    monkeypatch.setenv("GYMFX_GATHER_TICKET", "1")
    monkeypatch.setenv("GYMFX_LSTM_OPT_TAIL", "1")
    tf = _make_trainer(True, policy=policy, use_graphs=False)
    tu = _make_trainer(False, policy=policy, use_graphs=False)
    assert tf._mb_ticket is not None and tu._mb_ticket is None
    tf.collect_rollout()
    tu.collect_rollout()
    tf.mb_ctr.zero_()
    tu.mb_ctr.zero_()
    names = ["act_mb", "logp_mb", "adv_mb", "ret_mb"]
    names += ["obs_mb_seq", "done_mb", "h0_mb", "c0_mb"] if policy == "lstm" \
        else ["obs_mb"]
    for k in range(1, 7):  # crosses the epoch boundary at k = 4
        tf._gather_body()
        tu._gather_body()
        assert int(tf.mb_ctr.item()) == k == int(tu.mb_ctr.item())
        assert int(tf._mb_ticket.item()) == 0
        for nm in names:
            assert torch.equal(getattr(tf, nm), getattr(tu, nm)), nm


# 5. whole trainer ----------------------------------------------------------

def _assert_trainers_equal(tf, tu):
    mf, mu = tf.model, tu.model
    for nm in ("params", "m", "v", "grads", "params_bf16", "adam_ctr"):
        assert torch.equal(getattr(mf, nm), getattr(mu, nm)), nm
    for nm in mf._wt:
        assert torch.equal(mf.wt(nm), mu.wt(nm)), nm
    assert torch.equal(tf.mb_ctr, tu.mb_ctr)
    assert torch.equal(tf.act_buf, tu.act_buf)
    assert torch.equal(tf.env.st.equity, tu.env.st.equity)


@gpu
@pytest.mark.parametrize("policy", ["mlp", "lstm"])
@pytest.mark.parametrize("hidden", [64, 256])
def test_fused_tail_equals_unfused_trainer(policy, hidden, monkeypatch):
    # the LSTM trainer ignores the knob unless asked (measured slower)
    monkeypatch.setenv("GYMFX_LSTM_OPT_TAIL", "1")
    tf = _make_trainer(True, policy=policy, hidden=hidden)
    tu = _make_trainer(False, policy=policy, hidden=hidden)
    assert tf.model.fused_tail and tf.model.fuse_norm
    assert not tu.model.fused_tail
    for _ in range(3):
        tf.train_update(with_stats=False)
        tu.train_update(with_stats=False)
    torch.cuda.synchronize()
    assert tf._graphs_ready and tu._graphs_ready
    assert int(tf.model.adam_ctr.item()) == 3 * 8
    assert tf.model.state_dict()["adam_step"] == tu.model.state_dict()["adam_step"]
    _assert_trainers_equal(tf, tu)


@gpu
def test_fused_tail_with_gather_ticket_equals_unfused_trainer(monkeypatch):
    monkeypatch.setenv("GYMFX_GATHER_TICKET", "1")
    tf = _make_trainer(True)
    tu = _make_trainer(False)
    assert tf._mb_ticket is not None
    for _ in range(3):
        tf.train_update(with_stats=False)
        tu.train_update(with_stats=False)
    torch.cuda.synchronize()
    assert tf._graphs_ready
    _assert_trainers_equal(tf, tu)


@gpu
def test_fused_tail_equals_unfused_trainer_eager():
    tf = _make_trainer(True, use_graphs=False)
    tu = _make_trainer(False, use_graphs=False)
    for _ in range(3):
        tf.train_update(with_stats=False)
        tu.train_update(with_stats=False)
    torch.cuda.synchronize()
    _assert_trainers_equal(tf, tu)


@gpu
def test_fused_tail_equals_unfused_trainer_clipping_active():
    """max_grad_norm far below the gradient norm: the clip scale derived
    from the fused partials multiplies every step."""
    tf = _make_trainer(True, max_grad_norm=1e-4)
    tu = _make_trainer(False, max_grad_norm=1e-4)
    for _ in range(3):
        tf.train_update(with_stats=False)
        tu.train_update(with_stats=False)
        # the norm of the last minibatch's gradients is above the bound
        assert float(tu.model.grads.norm()) > 1e-4
    torch.cuda.synchronize()
    _assert_trainers_equal(tf, tu)


# 6. CPU oracle path --------------------------------------------------------

@pytest.mark.parametrize("policy", ["mlp", "lstm"])
def test_knob_is_a_no_op_on_the_cpu_fallback(policy, monkeypatch):
    monkeypatch.setenv("GYMFX_LSTM_OPT_TAIL", "1")
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
        pc = PPOConfig(rollout_steps=16, minibatches=4, ppo_epochs=2, seed=11,
                       hidden=32, policy=policy, bptt_len=4,
                       fused_opt_tail=fused)
        return PPOTrainer(env, pc)

    tf, tu = make(True), make(False)
    for _ in range(2):
        tf.train_update(with_stats=False)
        tu.train_update(with_stats=False)
    assert tf.model.fused_tail and not tu.model.fused_tail
    assert torch.equal(tf.model.params, tu.model.params)
    assert torch.equal(tf.model.m, tu.model.m)
    assert torch.equal(tf.model.params_bf16, tu.model.params_bf16)
    for nm in tf.model._wt:
        assert torch.equal(tf.model.wt(nm), tu.model.wt(nm))
    assert int(tf.model.adam_ctr) == int(tu.model.adam_ctr) == 16
    assert int(tf.mb_ctr) == int(tu.mb_ctr)
