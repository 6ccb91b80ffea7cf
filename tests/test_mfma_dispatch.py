"""Host-side tile dispatch of the MFMA GEMM / wgrad launchers (select_gemm /
select_wgrad in ops/csrc/mfma_dispatch.h) through the gemm_variant /
wgrad_variant / mfma_variants bindings.  Nothing here touches the GPU: the
tests run wherever the extension imports."""
import pytest

import mfma_cases as mc


@pytest.fixture(scope="module")
def ext():
    from gymfx_amd.ops import native

    e = native.load()
    if e is None:
        pytest.skip("HIP extension not built")
    return e


UNSET = mc.knob_ints({})
KNOB_SETS = [UNSET] + [mc.knob_ints(env) for env in mc.CHILD_KNOBS]


def _cdiv(a, b):
    return -(-a // b)


def _gemm_grid_of(name, c):
    """The grid the named instantiation needs to cover [M, N]: its own tile
    is 64 x 32*NFRAG whatever knob chose it."""
    nf = int(name.split("_nf")[1].split("_")[0])
    return (_cdiv(c.M, 64), _cdiv(c.N, 32 * nf))


def _wgrad_grid_of(name, c):
    kind, _, tile, _ = name.split("_")
    fk, fn = (int(x) for x in tile.split("x"))
    if kind == "glds":
        assert c.N % (32 * fn) == 0, "glds needs full N tiles"
    return (_cdiv(c.K, 32 * fk), _cdiv(c.N, 32 * fn), c.slabs)


@pytest.mark.parametrize("c", mc.INPROC_GEMM, ids=lambda c: c.id)
def test_inproc_gemm_case_reaches_its_variant(ext, c):
    name, grid = mc.gemm_variant(ext, c, UNSET)
    assert c.expect and c.expect in name
    assert tuple(grid) == _gemm_grid_of(name, c)


@pytest.mark.parametrize("c", mc.INPROC_WGRAD, ids=lambda c: c.id)
def test_inproc_wgrad_case_reaches_its_variant(ext, c):
    name, grid = mc.wgrad_variant(ext, c, UNSET)
    assert name == c.expect
    assert tuple(grid) == _wgrad_grid_of(name, c)


@pytest.mark.parametrize("kn", KNOB_SETS, ids=lambda k: "-".join(
    f"{a}{b}" for a, b in k.items()))
def test_grid_covers_the_output_under_every_knob(ext, kn):
    """Whatever tile a knob forces, the grid is the one of the kernel that
    is launched.  The gather-fused GEMM has only the 64-wide kernel: under a
    forced (or automatic) 128/256-wide tile its grid must stay 64-wide."""
    for c in mc.INPROC_GEMM + mc.CHILD_GEMM:
        name, grid = mc.gemm_variant(ext, c, kn)
        assert tuple(grid) == _gemm_grid_of(name, c), (c.id, name)
        if c.perm_mult:
            assert name == "tb1_act2_dt0_ab1_nf2_bk32_acc0_perm1"
    for c in mc.INPROC_WGRAD + mc.CHILD_WGRAD:
        name, grid = mc.wgrad_variant(ext, c, kn)
        assert tuple(grid) == _wgrad_grid_of(name, c), (c.id, name)


def test_gather_fused_gemm_grid_at_auto_mid_shape(ext):
    # N >= 1024 and M >= 16384 picks the 64x128 tile for the plain kernel;
    # the gather-fused kernel is 64 wide and needs all 16 column blocks
    plain = ext.gemm_variant(16384, 1024, 36, trans_b=True, act=2, add_bias=True)
    fused = ext.gemm_variant(16384, 1024, 36, trans_b=True, act=2,
                             add_bias=True, a_perm=True)
    assert plain == ("tb1_act2_dt0_ab1_nf4_bk32_acc0_perm0", (256, 8))
    assert fused == ("tb1_act2_dt0_ab1_nf2_bk32_acc0_perm1", (256, 16))
    for wide in (1, 4):
        assert ext.gemm_variant(130, 256, 36, trans_b=True, act=2, add_bias=True,
                                a_perm=True, wide=wide)[1] == (3, 4)


def test_knob_semantics(ext):
    v = lambda *a, **k: ext.gemm_variant(*a, **k)[0]  # noqa: E731
    # wide needs N >= 192, mid N >= 96; below that the 64x64 tile stays
    assert "_nf8_" in v(64, 192, 64, wide=1)
    assert "_nf2_" in v(64, 188, 64, wide=1)
    assert "_nf4_" in v(64, 96, 64, wide=4)
    assert "_nf2_" in v(64, 92, 64, wide=4)
    # wide=0 switches the automatic 64x128 tile off
    assert "_nf4_" in v(16384, 1024, 36, wide=-1)
    assert "_nf2_" in v(16384, 1024, 36, wide=0)
    assert "_nf2_" in v(16383, 1024, 36, wide=-1)
    # BK64: trans_b only, automatic from K = 512, never with wide/mid/accum
    assert "_bk64_" in v(128, 64, 512, trans_b=True, act=1, bk64=-1, n1=-1)
    assert "_bk32_" in v(128, 64, 508, trans_b=True, act=1, bk64=-1)
    assert "_bk64_" in v(128, 64, 36, trans_b=True, act=1, bk64=1)
    assert "_bk32_" in v(128, 64, 512, trans_b=True, act=1, bk64=0)
    assert "_bk32_" in v(128, 64, 512, trans_b=False, act=1, bk64=1)
    assert "_bk32_" in v(128, 256, 512, trans_b=True, act=1, bk64=1, wide=1)
    assert "_bk32_acc1" in v(128, 64, 512, trans_b=True, act=0, accum=True, bk64=1)
    # N1: plain f32 epilogue only, N <= 256, automatic while M*N <= 2^20
    n1 = dict(trans_b=True, act=0, wide=-1, bk64=-1)
    assert "_nf1_bk64_" in v(4096, 256, 512, n1=-1, **n1)
    assert "_nf2_bk64_" in v(4100, 256, 512, n1=-1, **n1)
    assert "_nf1_bk64_" in v(8192, 256, 512, n1=1, **n1)
    assert "_nf2_bk64_" in v(64, 256, 512, n1=0, **n1)
    assert "_nf2_bk64_" in v(64, 260, 512, n1=1, **n1)
    assert "_nf2_bk64_" in v(64, 256, 512, n1=1, add_bias=True, **n1)
    # the tanh' dgrad epilogue is bf16-out without bias whatever act says
    assert v(64, 64, 64, act=0, dact_tanh=True).startswith("tb0_act1_dt1_ab0")
    w = lambda *a, **k: ext.wgrad_variant(*a, **k)[0]  # noqa: E731
    # automatic 128x128 from 384 workgroups; the knob overrides both ways
    assert w(4096, 256, 260, 64, big=-1) == "glds_db1_5x4_perm0"
    assert w(4032, 256, 260, 63, big=-1) == "glds_db1_2x2_perm0"
    assert w(4096, 256, 260, 32, big=-1) == "glds_db1_2x2_perm0"
    assert w(4096, 256, 260, 32, big=1) == "glds_db1_5x4_perm0"
    assert w(4096, 256, 260, 64, big=0) == "glds_db1_2x2_perm0"
    # 5x4 only where it saves a K pass and N <= 512
    assert w(4096, 256, 256, 64, big=1) == "glds_db1_4x4_perm0"
    assert w(4096, 1024, 260, 64, big=1) == "glds_db1_4x4_perm0"
    # the 128-wide tile needs K, N >= 128
    assert w(4096, 64, 260, 64, big=1) == "glds_db1_2x2_perm0"
    assert w(4096, 256, 100, 64, want_db=False, big=1) == "glds_db0_2x2_perm0"
    # glds needs whole 64-row chunks per slab and whole N tiles
    assert w(4000, 256, 260, 64, big=0).startswith("partial_")
    assert w(4096, 200, 260, 64, big=0).startswith("partial_")
    assert w(4096, 256, 36, 64, big=0).startswith("partial_")


def test_omitted_knobs_are_the_process_values(ext):
    import os

    kn = mc.knob_ints(os.environ)
    for c in mc.INPROC_GEMM + mc.CHILD_GEMM:
        assert mc.gemm_variant(ext, c) == mc.gemm_variant(ext, c, kn)
    for c in mc.INPROC_WGRAD + mc.CHILD_WGRAD:
        assert mc.wgrad_variant(ext, c) == mc.wgrad_variant(ext, c, kn)


def test_uninstantiated_combination_raises(ext):
    # the gather fusion exists for the L1 forward epilogue only
    with pytest.raises(RuntimeError, match="no gemm kernel"):
        ext.gemm_variant(64, 64, 64, trans_b=False, act=1, a_perm=True)


def test_matrix_covers_every_instantiation(ext):
    """The case tables (in-process plus the forced-knob children) reach every
    instantiated variant; a new instantiation without a case fails here."""
    listed = ext.mfma_variants()
    assert len(listed) == len(set(listed))
    assert mc.predicted_variants(ext) == set(listed)
