"""Host side of the weight-resident tall GEMM: the gemm_resident_ok predicate
and the untouched tile dispatch beside it.  Nothing here touches the GPU: the
tests run wherever the extension imports.  The CPU path of
api.gemm(resident=True) is the plain torch path."""
import pytest
import torch


@pytest.fixture(scope="module")
def ext():
    from gymfx_amd.ops import native

    e = native.load()
    if e is None:
        pytest.skip("HIP extension not built")
    return e


FWD = dict(trans_b=True, act=2, dact_tanh=False, add_bias=True, accum=False)
DGRAD = dict(trans_b=True, act=1, dact_tanh=True, add_bias=False, accum=False)


@pytest.mark.parametrize("K", [256, 260])
@pytest.mark.parametrize("epi", [FWD, DGRAD], ids=["fwd", "dgrad"])
def test_predicate_accepts_the_flagship_shapes(ext, K, epi):
    assert ext.gemm_resident_ok(65536, 256, K, **epi)
    assert ext.gemm_resident_ok(262144, 256, K, **epi)


@pytest.mark.parametrize("K", [8, 36, 228, 264])
@pytest.mark.parametrize("M", [1, 256, 257, 300])
def test_predicate_accepts_any_row_count_and_short_k(ext, M, K):
    """A ragged last group is guarded in the kernel, so M is free."""
    assert ext.gemm_resident_ok(M, 256, K, **FWD)
    assert ext.gemm_resident_ok(M, 256, K, **DGRAD)


def test_predicate_refuses_what_the_kernel_does_not_do(ext):
    ok = ext.gemm_resident_ok
    assert not ok(65536, 192, 256, **FWD)
    assert not ok(65536, 1024, 256, **FWD)
    assert not ok(65536, 256, 268, **FWD)
    assert not ok(65536, 256, 258, **FWD)   # rows move in 8-byte pieces
    assert not ok(65536, 256, 0, **FWD)
    assert not ok(0, 256, 256, **FWD)
    assert not ok(65536, 256, 256, **{**FWD, "trans_b": False})
    assert not ok(65536, 256, 256, **{**FWD, "accum": True})
    assert not ok(65536, 256, 256, **{**FWD, "act": 0})
    assert not ok(65536, 256, 256, **{**FWD, "act": 1})
    # tanh without bias and tanh' with bias are not implemented
    assert not ok(65536, 256, 256, **{**FWD, "add_bias": False})
    assert not ok(65536, 256, 256, **{**DGRAD, "add_bias": True})
    assert not ok(65536, 256, 256, **{**DGRAD, "act": 2})
    assert not ok(65536, 256, 256, a_perm=True, **FWD)


# the tile dispatch as the parent commit has it
PARENT_VARIANTS = 77  # 57 gemm_kernel + 12 wgrad_glds + 8 wgrad_partial
FLAGSHIP = [
    ((65536, 256, 260), FWD, "tb1_act2_dt0_ab1_nf2_bk32_acc0_perm0"),
    ((65536, 256, 256), FWD, "tb1_act2_dt0_ab1_nf2_bk32_acc0_perm0"),
    ((65536, 256, 256), DGRAD, "tb1_act1_dt1_ab0_nf2_bk32_acc0_perm0"),
    ((4096, 256, 260), FWD, "tb1_act2_dt0_ab1_nf2_bk32_acc0_perm0"),
]


def test_tile_dispatch_is_unchanged(ext):
    names = ext.mfma_variants()
    assert len(names) == len(set(names)) == PARENT_VARIANTS
    assert not [n for n in names if "resident" in n]
    for (M, N, K), epi, want in FLAGSHIP:
        name, grid = ext.gemm_variant(M, N, K, **epi)
        assert name == want
        assert tuple(grid) == (M // 64, N // 64)


def test_cpu_resident_keyword_is_the_torch_path():
    from gymfx_amd.ops import api

    gen = torch.Generator().manual_seed(3)
    M, N, K = 96, 256, 260
    A = torch.randn(M, K, generator=gen).to(torch.bfloat16)
    Wt = (torch.randn(N, K, generator=gen) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, generator=gen)
    Y = torch.tanh(torch.randn(M, N, generator=gen)).to(torch.bfloat16)
    for kw in (dict(bias=bias, act=2), dict(bias=None, act=1, dact_tanh=True, Yact=Y)):
        b = kw.pop("bias")
        out = []
        for res in (False, True):
            C = torch.zeros(M, N, dtype=torch.bfloat16)
            api.gemm(A, Wt, b, C, trans_b=True, resident=res, **kw)
            out.append(C)
        assert torch.equal(out[0], out[1])
