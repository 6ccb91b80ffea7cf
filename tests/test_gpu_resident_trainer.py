"""PPOConfig.resident_gemm — the MLP trainer is bitwise the same with the
tall N=256 GEMMs on the weight-resident kernel as on the tiled one, eager and
under captured graphs, and the row threshold keeps small calls off it."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _make_trainer(resident, *, use_graphs):
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
        "seed": 3,
    }
    env = build_vec_environment(cfg, md)
    env.reset(seed=3)
    pc = PPOConfig(rollout_steps=16, minibatches=2, ppo_epochs=1, seed=3,
                   use_graphs=use_graphs, resident_gemm=resident)
    return PPOTrainer(env, pc)


class _Calls:
    """Records the row count of every ext.gemm_resident launch (under graph
    capture: of every captured launch)."""

    def __init__(self, monkeypatch):
        from gymfx_amd.ops import native

        ext = native.require()
        real = ext.gemm_resident
        self.rows = []

        def spy(A, *a, **kw):
            self.rows.append(int(A.shape[0]))
            return real(A, *a, **kw)

        monkeypatch.setattr(ext, "gemm_resident", spy)


@pytest.mark.parametrize("use_graphs", [False, True])
def test_resident_trainer_equals_tiled_trainer(use_graphs, monkeypatch):
    calls = _Calls(monkeypatch)
    tr = _make_trainer(True, use_graphs=use_graphs)
    tt = _make_trainer(False, use_graphs=use_graphs)
    assert tr.model.resident_gemm and not tt.model.resident_gemm
    tr.model.resident_min_rows = 0
    for _ in range(2):
        tr.train_update()
        tt.train_update()
    torch.cuda.synchronize()
    # the update's three tall GEMMs went through the resident kernel
    M_mb = 256 * 16 // 2
    assert calls.rows.count(M_mb) >= 3
    for nm in ("params", "m", "v"):
        assert torch.equal(getattr(tr.model, nm), getattr(tt.model, nm)), nm
    for nm in ("h1", "h2"):
        assert torch.equal(tr.acts_train[nm].view(torch.int16),
                           tt.acts_train[nm].view(torch.int16)), nm
    assert torch.equal(tr.scratch["dh1"].view(torch.int16),
                       tt.scratch["dh1"].view(torch.int16))


def test_default_threshold_keeps_small_calls_on_the_tiled_kernel(monkeypatch):
    """256 envs: the rollout forward has 256 rows and the minibatch 2048,
    both far below the threshold at which the resident kernel fills the
    chip — nothing may be routed."""
    from gymfx_amd.algo.ppo import PPOConfig

    calls = _Calls(monkeypatch)
    t = _make_trainer(True, use_graphs=False)
    assert t.model.resident_gemm
    assert t.model.resident_min_rows == PPOConfig().resident_min_rows > 4096
    t.train_update()
    torch.cuda.synchronize()
    assert calls.rows == []
    # and the model asks for it only from the threshold on
    assert not t.model._resident(256)
    assert not t.model._resident(t.model.resident_min_rows - 1)
    assert t.model._resident(t.model.resident_min_rows)
