"""Weight-resident tall GEMM (ext.gemm_resident) — bit-equality with ext.gemm.

The reference is always ext.gemm on the same operands: its
tb1_act2_dt0_ab1_nf2_bk32 and tb1_act1_dt1_ab0_nf2_bk32 variants are anchored
to fp64 by tests/test_gpu_mfma_matrix.py.  Outputs are compared as raw int16
bits and must be EQUAL; there is no tolerance anywhere in this file.  Output
buffers start as NaN (an element the kernel skips fails) and every operand
sits between 4 KiB NaN guard bands that must come back intact.

Shapes are the smallest that reach each path of the kernel: one 256-row
group, more groups than workgroups (the persistent loop re-using the weight
image), a ragged last group, K with 0 / 1 / 7 / 8 full 32-deep chunks, with
and without a 4-element or 8-element tail.
"""
import pytest
import torch

import mfma_cases as mc

pytestmark = pytest.mark.gpu

N = 256
EPIS = ["fwd", "dgrad"]  # bias + tanh | x (1 - Yact^2)


@pytest.fixture(scope="module")
def ext():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gymfx_amd.ops import native

    return native.require()


def _bits(t):
    return t.view(torch.int16)


def _operands(M, K, seed, dev="cuda"):
    gen = torch.Generator().manual_seed(7000 + seed)
    A = mc._randn_bf16((M, K), gen, 1.0, dev)
    Wt = mc._randn_bf16((N, K), gen, K ** -0.5, dev)
    bias = torch.randn(N, generator=gen).to(dev)
    Y = torch.tanh(torch.randn(M, N, generator=gen)).to(torch.bfloat16).to(dev)
    return A, Wt, bias, Y


def _flags(epi):
    # (act, dact_tanh, uses bias)
    return (2, False, True) if epi == "fwd" else (1, True, False)


def _reference(ext, A, Wt, bias, Y, epi):
    act, dact, ab = _flags(epi)
    C = torch.full((A.shape[0], N), float("nan"), dtype=torch.bfloat16,
                   device=A.device)
    ext.gemm(A, Wt, bias if ab else None, C, Y if dact else None, True, act,
             dact, False)
    torch.cuda.synchronize()
    return C


def _resident(ext, A, Wt, bias, Y, epi, max_blocks=0):
    """One launch on guarded buffers; asserts the guards, returns C."""
    act, dact, ab = _flags(epi)
    gA, gW = mc.guarded_copy(A), mc.guarded_copy(Wt)
    gb = mc.guarded_copy(bias) if ab else None
    gY = mc.guarded_copy(Y) if dact else None
    gC = mc.Guarded((A.shape[0], N), torch.bfloat16, A.device)  # NaN-filled
    ext.gemm_resident(gA.t, gW.t, gb.t if gb else None, gC.t,
                      gY.t if gY else None, act, dact, max_blocks)
    torch.cuda.synchronize()
    for name, g in (("A", gA), ("Wt", gW), ("bias", gb), ("Yact", gY), ("C", gC)):
        if g is not None:
            assert g.intact(), f"guard band of {name} changed"
    assert torch.equal(_bits(gA.t), _bits(A)) and torch.equal(_bits(gW.t), _bits(Wt))
    return gC.t


def _assert_equal_bits(out, ref):
    neq = _bits(out) != _bits(ref)
    n = int(neq.sum())
    if n:
        r, c = (int(x[0]) for x in torch.nonzero(neq, as_tuple=True))
        pytest.fail(f"{n} of {out.numel()} elements differ; first at "
                    f"[{r}, {c}]: {float(out[r, c])} vs {float(ref[r, c])}")


# (M, K, max_blocks)
CASES = [
    (256, 256, 0), (256, 260, 0),      # the two workload shapes, one group
    (256, 264, 0),                     # largest K: 8-element tail
    (256, 36, 0), (256, 228, 0),       # one chunk + tail, seven chunks + tail
    (256, 8, 0),                       # no full chunk at all
    (768, 260, 2),                     # workgroup 0 does groups 0 and 2
    (768, 256, 2),
    (512, 260, 1),                     # one workgroup, two groups
    (512, 36, 1),
    (300, 260, 0), (257, 256, 0),      # ragged last group
    (257, 228, 1),
]


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M,K,max_blocks", CASES,
                         ids=[f"{m}x{k}-b{b}" for m, k, b in CASES])
def test_random_operands_bitwise(ext, M, K, max_blocks, epi):
    act, dact, ab = _flags(epi)
    assert ext.gemm_resident_ok(M, N, K, True, act, dact, ab, False)
    A, Wt, bias, Y = _operands(M, K, M + K)
    ref = _reference(ext, A, Wt, bias, Y, epi)
    assert not bool(torch.isnan(ref).any())
    out = _resident(ext, A, Wt, bias, Y, epi, max_blocks)
    _assert_equal_bits(out, ref)


@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("M", [300, 257])
def test_ragged_m_matches_the_predicate(ext, M, epi):
    """The kernel guards a ragged last group, so the predicate accepts any M
    and api.gemm(resident=True) must route there and stay bitwise equal."""
    from gymfx_amd.ops import api

    act, dact, ab = _flags(epi)
    K = 260
    assert ext.gemm_resident_ok(M, N, K, True, act, dact, ab, False)
    A, Wt, bias, Y = _operands(M, K, 31 * M)
    ref = _reference(ext, A, Wt, bias, Y, epi)
    C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device="cuda")
    api.gemm(A, Wt, bias if ab else None, C, Yact=Y if dact else None,
             trans_b=True, act=act, dact_tanh=dact, resident=True)
    torch.cuda.synchronize()
    _assert_equal_bits(C, ref)


def test_api_falls_back_where_the_predicate_refuses(ext):
    """N = 192 has no resident kernel: resident=True must change nothing."""
    from gymfx_amd.ops import api

    M, K, n = 256, 260, 192
    assert not ext.gemm_resident_ok(M, n, K, True, 2, False, True, False)
    gen = torch.Generator().manual_seed(5)
    A = mc._randn_bf16((M, K), gen, 1.0, "cuda")
    Wt = mc._randn_bf16((n, K), gen, K ** -0.5, "cuda")
    bias = torch.randn(n, generator=gen).cuda()
    out = []
    for res in (False, True):
        C = torch.full((M, n), float("nan"), dtype=torch.bfloat16, device="cuda")
        api.gemm(A, Wt, bias, C, trans_b=True, act=2, resident=res)
        out.append(C)
    torch.cuda.synchronize()
    _assert_equal_bits(out[1], out[0])


PROBE_ROWS = [0, 15, 16, 31, 32, 255, 256]
PROBE_KS = [0, 7, 8, 31, 32, 255, 256, 259]


@pytest.mark.parametrize("epi", EPIS)
def test_one_hot_probes(ext, epi):
    """A zero except A[i, k*] = 1, i at the fragment / wave / group
    boundaries and k* at the chunk boundaries and in the tail, rotated so
    every (i, k*) pair is hit.  The accumulator of row i is then column k* of
    the weights with no rounding at all, so the output row is the bf16
    epilogue of that column exactly — computed here on the host side of the
    kernel (fp32 torch ops cannot reproduce fast_tanh bit for bit, so the
    forward epilogue's expected bits come from ext.gemm; the dgrad epilogue
    is reproduced independently)."""
    M, K = 512, 260
    _, Wt, bias, Y = _operands(M, K, 99)
    for s in range(len(PROBE_KS)):
        sel = [PROBE_KS[(j + s) % len(PROBE_KS)] for j in range(len(PROBE_ROWS))]
        A = torch.zeros(M, K, dtype=torch.bfloat16, device="cuda")
        A[PROBE_ROWS, sel] = 1.0
        out = _resident(ext, A, Wt, bias, Y, epi, max_blocks=1)
        ref = _reference(ext, A, Wt, bias, Y, epi)
        _assert_equal_bits(out, ref)
        if epi == "dgrad":
            pre = torch.zeros(M, N, dtype=torch.float32, device="cuda")
            pre[PROBE_ROWS] = Wt[:, sel].t().float()
            y = Y.float()
            exp = (pre * (1.0 - y * y)).to(torch.bfloat16)
            # signed zeros: -w * 0 and 0 * (1 - y^2) agree in value, compare
            # values there and bits everywhere else
            nz = exp != 0
            assert torch.equal(_bits(out)[nz], _bits(exp)[nz])
            assert bool((out[~nz] == 0).all())
        else:
            # rows without a one: tanh(bias) only, the same in every such row
            plain = [r for r in range(M) if r not in PROBE_ROWS]
            assert bool((_bits(out[plain]) == _bits(out[plain[0]])).all())
            # a probed row differs from it wherever the weight column is big
            # enough to move the bf16 result
            for r, k in zip(PROBE_ROWS, sel):
                w = Wt[:, k].float()
                moved = (torch.tanh(w + bias) - torch.tanh(bias)).abs() > 2.0 ** -6
                assert bool((out[r][moved] != out[plain[0]][moved]).all()), (r, k)


def test_tanh_saturation_at_the_largest_bf16_inputs(ext):
    """Largest finite bf16 operands: the pre-activation overflows to +-inf
    (or stays huge), fast_tanh clamps, h must be +-1 exactly wherever the
    reference says so — and nowhere NaN."""
    M, K = 256, 260
    big = torch.finfo(torch.bfloat16).max
    gen = torch.Generator().manual_seed(11)
    sign_a = (torch.randint(0, 2, (M, K), generator=gen) * 2 - 1).float()
    sign_w = (torch.randint(0, 2, (N, K), generator=gen) * 2 - 1).float()
    A = (sign_a * big).to(torch.bfloat16).cuda()
    # one +-big weight per row, the rest zero: no inf - inf inside the sum
    Wt = torch.zeros(N, K)
    Wt[torch.arange(N), torch.arange(N) % K] = big
    Wt = (Wt * sign_w).to(torch.bfloat16).cuda()
    bias = torch.randn(N, generator=gen).cuda()
    ref = _reference(ext, A, Wt, bias, None, "fwd")
    # the construction: every pre-activation is +-inf, the reference
    # saturates all of them
    assert bool((ref.float().abs() == 1.0).all())
    out = _resident(ext, A, Wt, bias, None, "fwd")
    _assert_equal_bits(out, ref)
