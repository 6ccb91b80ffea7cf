"""Case tables, fp64 references and derived error bounds of the MFMA GEMM /
wgrad variant matrix (tests/test_gpu_mfma_matrix.py, tests/test_mfma_dispatch.py).

Run as a script it is the forced-knob child: ``python mfma_cases.py --child``
runs CHILD_GEMM / CHILD_WGRAD under the GYMFX_* knobs of its environment and
prints one JSON report line on stdout.

Every tolerance here is derived, none is fitted.  u = 2^-23 is one fp32 ulp
(relative) per accumulation step, which covers a truncating as well as a
rounding adder; products of two bf16 values have 16 significant bits and
are exact in fp32.  A sum of n terms accumulated in ANY order with relative
error <= u per add is within (n-1)*u*sum|terms| of the true sum (to first
order), so:

  GEMM, f32 out    |C - ref| <= (K+2)*u*S,  S = |A|.|B| + |bias| + |C0|
                   (K product adds, the bias add, the accumulate add)
  bf16 out         e = the f32 bound pushed through the epilogue, then
                   tol = e + 2^-8*(|ref| + e): (__bf16) rounds to nearest
                   even, 8 significant bits, so half an ulp is at most
                   2^-8 relative, taken of the largest value the fp32
                   result can have
    tanh           1-Lipschitz, so e passes unchanged, plus FAST_TANH_ABS
    (1 - y^2)      the factor is at most 1, so e passes unchanged; y*y,
                   1 - y*y and the product are three more fp32 roundings of
                   a value of magnitude <= |pre|: + 3*u*|pre|
  wgrad            mps = ceil(M/slabs) rows per slab:
                   |dW_part[s] - ref_s| <= (mps+2)*u*(|X_s|^T.|dY_s|)
                   |dW - ref| <= (mps+slabs+2)*u*(|X|^T.|dY|)
                   and the same factors times sum|dY| for db_part / db
"""
from __future__ import annotations

import json
import math
import os
import sys
from dataclasses import dataclass, replace
from typing import Optional

import torch

U = 2.0 ** -23

# fast_tanh(x) = 1 - 2*rcp(exp2(x*2.885...) + 1), absolute error budget in
# units of 2^-24, for |x| <= 15 (the clamp itself is exact):
#  * exp2 argument: the product x*c rounds (2^-24 relative) and c itself is
#    a rounded constant (2^-24): the argument is off by <= 2*|x|*c*2^-24,
#    i.e. e = exp(2x) by 2*|2x|*2^-24 relative.  d tanh/d ln(e) =
#    (1 - tanh^2)/2 and |x|*(1 - tanh(x)^2) <= 0.45, so < 1 unit.
#  * v_exp_f32: 1 ulp = 2^-23 relative on e, times (1 - tanh^2)/2 <= 1/2:
#    1 unit.
#  * e + 1 rounds (2^-24) and v_rcp_f32 is 1 ulp (2^-23): r = rcp(e+1) is
#    off by 1.5*2^-23 relative, and 2*r <= 2, so 2*r is off by <= 3*2^-23:
#    6 units.
#  * the final 1 - 2r has magnitude <= 1: one rounding (or truncation) is
#    <= 2^-23: 2 units.
# Sum 10 units = 10*2^-24 < 2^-20: the allowance the bound uses.
FAST_TANH_ABS = 2.0 ** -20

BF16_HALF_ULP = 2.0 ** -8
GUARD_BYTES = 4096
PERM_SEED = 0x5EED1234


# ---------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------
@dataclass(frozen=True)
class GemmCase:
    M: int
    N: int
    K: int
    tb: bool = False
    act: int = 0
    bias: bool = False
    dact: bool = False
    accum: bool = False
    # a_perm: A is an [M*mult, K] slab read through the epoch permutation
    perm_mult: int = 0
    step_base: int = 0
    mb_ctr: int = 0
    ctr_off: int = 0
    expect: str = ""  # substring the variant name must contain

    @property
    def id(self) -> str:
        s = (f"{self.M}x{self.N}x{self.K}-tb{int(self.tb)}-act{self.act}"
             f"-b{int(self.bias)}-dt{int(self.dact)}-acc{int(self.accum)}")
        if self.perm_mult:
            s += f"-perm{self.perm_mult}@{self.step_base}.{self.mb_ctr}{self.ctr_off:+d}"
        return s

    def flags(self) -> dict:
        return dict(trans_b=self.tb, act=self.act, dact_tanh=self.dact,
                    add_bias=self.bias, accum=self.accum,
                    a_perm=self.perm_mult > 0)


@dataclass(frozen=True)
class WgradCase:
    M: int
    K: int
    N: int
    slabs: int
    db: bool = True
    perm_mult: int = 0
    step_base: int = 0
    mb_ctr: int = 0
    ctr_off: int = 0
    expect: str = ""

    @property
    def id(self) -> str:
        s = f"{self.M}x{self.K}x{self.N}-s{self.slabs}-db{int(self.db)}"
        if self.perm_mult:
            s += f"-perm{self.perm_mult}@{self.step_base}.{self.mb_ctr}{self.ctr_off:+d}"
        return s


# (act, bias, dact): the seven instantiated epilogues; accum is the eighth
EPILOGUES = [(0, False, False), (0, True, False), (1, False, False),
             (1, True, False), (2, False, False), (2, True, False),
             (1, False, True)]


def _epilogue_cases(M, N, K, tb, expect, epilogues=EPILOGUES, accum=True):
    out = [GemmCase(M, N, K, tb, a, b, d, expect=expect) for a, b, d in epilogues]
    if accum:
        # accum never takes the BK64 pipeline
        out.append(GemmCase(M, N, K, tb, 0, accum=True,
                            expect=expect.split("_bk")[0] + "_bk32_acc1"))
    return out


def _inproc_gemm():
    cases = []
    # 64x64 / BK32: every epilogue, both layouts.  M=65 puts an LDS-direct
    # block and a register-staged block in one launch; K=36/68/260 leave 4
    # live elements in the last 8-wide vector; 3 and 4 go the scalar path.
    for shape in [(1, 4, 4), (63, 60, 36), (64, 64, 64), (65, 68, 260),
                  (130, 3, 256), (128, 256, 3), (200, 100, 68)]:
        for tb in (False, True):
            cases += _epilogue_cases(*shape, tb, "nf2_bk32")
    # BK64 64x64 (auto at trans_b, K >= 512) with bias or act set
    for shape in [(128, 64, 516), (65, 68, 580)]:
        cases += _epilogue_cases(*shape, True, "nf2_bk64", EPILOGUES[1:],
                                 accum=False)
    # 64x32 (N1 auto: trans_b, act 0, no bias, M*N small, K >= 512)
    for shape in [(100, 40, 516), (64, 256, 512)]:
        cases.append(GemmCase(*shape, True, 0, expect="nf1_bk64"))
    # accum never takes the BK64 pipeline
    cases.append(GemmCase(128, 64, 516, True, 0, accum=True,
                          expect="nf2_bk32_acc1"))
    # auto 64x128 tile (N >= 1024, M >= 16384)
    for tb in (False, True):
        cases.append(GemmCase(16384, 1024, 36, tb, 0, True, expect="nf4_bk32"))
    # gather-fused first GEMM: 96*11 source rows (not a power of two, so the
    # cycle-walk runs), 8 minibatches, counters at zero and later
    for sb, ctr, off in [(0, 0, 0), (5, 11, 0), (3, 12, -1)]:
        cases.append(GemmCase(132, 100, 68, True, 2, True, perm_mult=8,
                              step_base=sb, mb_ctr=ctr, ctr_off=off,
                              expect="nf2_bk32_acc0_perm1"))
    # ... and at the auto-mid shape: the grid must still be the 64-wide one
    cases.append(GemmCase(16384, 1024, 36, True, 2, True, perm_mult=2,
                          step_base=1, mb_ctr=3, expect="nf2_bk32_acc0_perm1"))
    return cases


def _with_perm_and_db(c: WgradCase, perm: bool):
    out = [c, replace(c, db=False, expect=c.expect.replace("db1", "db0"))]
    if perm:
        out += [replace(x, perm_mult=2, step_base=2, mb_ctr=5, ctr_off=-1,
                        expect=x.expect.replace("perm0", "perm1")) for x in list(out)]
    return out


def _inproc_wgrad():
    cases = []
    table = [
        # (M, K, N, slabs), variant, also under x_perm
        ((256, 64, 64, 4), "glds_db1_2x2_perm0", False),
        ((256, 68, 64, 4), "glds_db1_2x2_perm0", True),
        ((512, 100, 128, 4), "glds_db1_2x2_perm0", False),
        ((4096, 324, 256, 64), "glds_db1_4x4_perm0", True),
        # the MLP headline shape: 100 live columns in the second K tile
        ((4096, 260, 256, 64), "glds_db1_5x4_perm0", True),
        # register-staged kernel: N=4 is the head layer (reduce: elems<=4096)
        ((300, 256, 4, 3), "partial_db1_2x2_perm0", True),
        ((190, 256, 3, 3), "partial_db1_2x2_perm0", False),
        # 8 slabs over 5 rows: slabs 5..7 are empty and must come out zero
        ((5, 64, 64, 8), "partial_db1_2x2_perm0", False),
        ((2560, 260, 256, 64), "partial_db1_4x4_perm0", True),
    ]
    for shape, name, perm in table:
        cases += _with_perm_and_db(WgradCase(*shape, expect=name), perm)
    return cases


INPROC_GEMM = _inproc_gemm()
INPROC_WGRAD = _inproc_wgrad()

# Forced-knob children: one fresh process each (the knobs are read once per
# process).  Values are strings for the environment; select_* sees ints.
CHILD_KNOBS = [
    {"GYMFX_GEMM_WIDE": "1", "GYMFX_GEMM_BK64": "1", "GYMFX_GEMM_N1": "1",
     "GYMFX_WGRAD_BIG": "1"},
    {"GYMFX_GEMM_WIDE": "4", "GYMFX_GEMM_BK64": "0", "GYMFX_GEMM_N1": "0",
     "GYMFX_WGRAD_BIG": "0"},
    {"GYMFX_GEMM_WIDE": "1", "GYMFX_GEMM_BK64": "1", "GYMFX_GEMM_N1": "0",
     "GYMFX_WGRAD_BIG": "0"},
]


def _child_gemm():
    cases = []
    for shape in [(130, 256, 36), (65, 200, 68), (128, 100, 516)]:
        for tb in (False, True):
            for a, b, d in EPILOGUES:
                cases.append(GemmCase(*shape, tb, a, b, d))
            cases.append(GemmCase(*shape, tb, 0, accum=True))
    # the gather-fused GEMM under a forced wide / mid tile knob
    cases.append(GemmCase(130, 256, 36, True, 2, True, perm_mult=3,
                          step_base=4, mb_ctr=7,
                          expect="nf2_bk32_acc0_perm1"))
    return cases


def _child_wgrad():
    cases = []
    for shape in [(128, 516, 256, 2), (130, 68, 200, 3), (128, 36, 100, 2)]:
        cases += _with_perm_and_db(WgradCase(*shape), True)
    return cases


CHILD_GEMM = _child_gemm()
CHILD_WGRAD = _child_wgrad()


def knob_ints(env: dict) -> dict:
    """GYMFX_* environment -> the knob keyword arguments of the variant
    queries (-1 = unset)."""
    g = lambda k: int(env[k]) if k in env else -1  # noqa: E731
    return {"wide": g("GYMFX_GEMM_WIDE"), "bk64": g("GYMFX_GEMM_BK64"),
            "n1": g("GYMFX_GEMM_N1"), "big": g("GYMFX_WGRAD_BIG")}


def gemm_variant(ext, c: GemmCase, knobs: Optional[dict] = None):
    kw = {}
    if knobs is not None:
        kw = {k: knobs[k] for k in ("wide", "bk64", "n1")}
    return ext.gemm_variant(c.M, c.N, c.K, **c.flags(), **kw)


def wgrad_variant(ext, c: WgradCase, knobs: Optional[dict] = None):
    kw = {} if knobs is None else {"big": knobs["big"]}
    return ext.wgrad_variant(c.M, c.N, c.K, c.slabs, want_db=c.db,
                             x_perm=c.perm_mult > 0, **kw)


def predicted_variants(ext) -> set:
    """Every variant name the matrix reaches: the in-process tables under
    unset knobs plus the child tables under each child's knobs."""
    unset = knob_ints({})
    names = {gemm_variant(ext, c, unset)[0] for c in INPROC_GEMM}
    names |= {wgrad_variant(ext, c, unset)[0] for c in INPROC_WGRAD}
    for env in CHILD_KNOBS:
        kn = knob_ints(env)
        names |= {gemm_variant(ext, c, kn)[0] for c in CHILD_GEMM}
        names |= {wgrad_variant(ext, c, kn)[0] for c in CHILD_WGRAD}
    return names


# ---------------------------------------------------------------------------
# guard bands
# ---------------------------------------------------------------------------
class Guarded:
    """A contiguous tensor carved out of a larger flat buffer with 4 KiB of
    NaN before and after it.  The body starts 4096 bytes into the
    allocation, so it keeps the (512-byte) alignment a tensor of its own
    would have.  NaN guards serve both ways: an input read past its end
    poisons the output, and a write into an output's guard changes its
    bits."""

    def __init__(self, shape, dtype, device):
        n = int(math.prod(shape))
        self.g = GUARD_BYTES // torch.empty((), dtype=dtype).element_size()
        self.flat = torch.full((2 * self.g + n,), float("nan"), dtype=dtype,
                               device=device)
        self.t = self.flat[self.g:self.g + n].view(*shape)
        assert self.t.is_contiguous()
        assert not self.t.is_cuda or self.t.data_ptr() % 512 == 0
        self._bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
        self._pat = torch.full((self.g,), float("nan"), dtype=dtype,
                               device=device).view(self._bits)

    def intact(self) -> bool:
        lo = self.flat[:self.g].view(self._bits)
        hi = self.flat[self.flat.numel() - self.g:].view(self._bits)
        return bool(torch.equal(lo, self._pat) and torch.equal(hi, self._pat))


def guarded_copy(src: torch.Tensor) -> Guarded:
    g = Guarded(tuple(src.shape), src.dtype, src.device)
    g.t.copy_(src)
    return g


# ---------------------------------------------------------------------------
# shared pieces
# ---------------------------------------------------------------------------
def _randn_bf16(shape, gen, scale, device):
    return (torch.randn(*shape, generator=gen) * scale).to(torch.bfloat16).to(device)


def _perm_dict(c, device):
    return {"seed": PERM_SEED, "minibatches": c.perm_mult, "ctr_off": c.ctr_off,
            "step_base": torch.tensor(c.step_base, dtype=torch.int64, device=device),
            "mb_ctr": torch.tensor(c.mb_ctr, dtype=torch.int64, device=device)}


def _perm_kwargs(pd):
    return dict(ap_seed=pd["seed"], ap_minibatches=pd["minibatches"],
                ap_ctr_off=pd["ctr_off"], ap_step_base=pd["step_base"],
                ap_mb_ctr=pd["mb_ctr"])


def _source_slab(c, logical, gen, device, zero_rest):
    """Scatter the logical [M, K] operand into the [M*mult, K] source slab at
    the rows the reference permutation (api._perm_rows) selects."""
    from gymfx_amd.ops import api

    pd = _perm_dict(c, device)
    n_rows = c.M * c.perm_mult
    idx = api._perm_rows(n_rows, c.M, pd).to(device)
    assert idx.unique().numel() == c.M
    if zero_rest:
        src = torch.zeros(n_rows, c.K, dtype=torch.bfloat16, device=device)
    else:
        src = _randn_bf16((n_rows, c.K), gen, 1.0, device)
    src[idx] = logical
    return src, pd


def _worst(err, tol):
    """(all within bound, largest err/tol).  An element with tol == 0 must be
    exact; NaN anywhere fails."""
    ok = bool((err <= tol).all())
    ratio = torch.where(tol > 0, err / tol, torch.where(
        err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    r = float(ratio.max()) if ratio.numel() else 0.0
    return ok, r


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


class Failures(list):
    def check(self, cond, msg):
        if not cond:
            self.append(msg)


# ---------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------
def _gemm_launch(ext, c: GemmCase, A_log, B, bias, Y, C0, gen, fails, tag,
                 zero_rest=False):
    """One launch on guarded buffers; returns the output tensor."""
    dev = A_log.device
    pd = None
    A_src = A_log
    if c.perm_mult:
        A_src, pd = _source_slab(c, A_log, gen, dev, zero_rest)
    gA, gB = guarded_copy(A_src), guarded_copy(B)
    gbias = guarded_copy(bias) if c.bias else None
    gY = guarded_copy(Y) if c.dact else None
    gC = Guarded((c.M, c.N), torch.float32 if c.act == 0 else torch.bfloat16, dev)
    if c.accum:
        gC.t.copy_(C0)
    ext.gemm(gA.t, gB.t, gbias.t if gbias else None, gC.t,
             gY.t if gY else None, c.tb, c.act, c.dact, c.accum,
             **(_perm_kwargs(pd) if pd else {}))
    _sync(dev)
    for name, g in (("A", gA), ("B", gB), ("bias", gbias), ("Yact", gY), ("C", gC)):
        if g is not None:
            fails.check(g.intact(), f"{tag}: guard band of {name} changed")
    fails.check(torch.equal(gA.t, A_src) and torch.equal(gB.t, B),
                f"{tag}: an input operand was modified")
    return gC.t


def _gemm_bound(c: GemmCase, A_log, B, bias, Y, C0):
    """fp64 reference of the case and the elementwise tolerance (see the
    module docstring for the derivation)."""
    Bd = B.double().t() if c.tb else B.double()
    Ad = A_log.double()
    pre = Ad @ Bd
    S = Ad.abs() @ Bd.abs()
    if c.bias:
        pre = pre + bias.double()
        S = S + bias.double().abs()
    if c.accum:
        pre = pre + C0.double()
        S = S + C0.double().abs()
    e = (c.K + 2) * U * S
    if c.act == 0:
        return pre, e
    ref = pre
    if c.act == 2:
        ref = torch.tanh(pre)
        e = e + FAST_TANH_ABS
    if c.dact:
        ref = ref * (1.0 - Y.double() ** 2)
        e = e + 3 * U * pre.abs()
    return ref, e + BF16_HALF_ULP * (ref.abs() + e)


def _probe_rows(M):
    return sorted({r for r in (0, 63, 64, M - 1) if 0 <= r < M})


def _probe_ks(K):
    return sorted({k for k in (0, 31, 32, 63, 64, K - 9, K - 8, K - 1) if 0 <= k < K})


def run_gemm_case(ext, c: GemmCase, device="cuda", seed=0) -> dict:
    """Random operands against the fp64 bound, then one-hot probes: A is
    zero except A[i, k*] = 1 for i at the block boundaries and k* at every
    staging boundary, rotated over the launches so every (i, k*) pair is
    hit.  Row i of the product is then row k* of B exactly."""
    fails = Failures()
    gen = torch.Generator().manual_seed(1000 + seed)
    M, N, K = c.M, c.N, c.K
    A = _randn_bf16((M, K), gen, 1.0, device)
    B = _randn_bf16((N, K) if c.tb else (K, N), gen, K ** -0.5, device)
    bias = torch.randn(N, generator=gen).to(device) if c.bias else None
    Y = torch.tanh(torch.randn(M, N, generator=gen)).to(torch.bfloat16).to(device) \
        if c.dact else None
    C0 = torch.randn(M, N, generator=gen).to(device) if c.accum else None

    out = _gemm_launch(ext, c, A, B, bias, Y, C0, gen, fails, "random")
    ref, tol = _gemm_bound(c, A, B, bias, Y, C0)
    ok, worst = _worst((out.double() - ref).abs(), tol)
    fails.check(ok, f"random: error is {worst:.3g} x the bound")

    rows, ks = _probe_rows(M), _probe_ks(K)
    Bmat = B.t() if c.tb else B  # logical [K, N]
    for s in range(len(ks)):
        A1 = torch.zeros(M, K, dtype=torch.bfloat16, device=device)
        sel = [ks[(j + s) % len(ks)] for j in range(len(rows))]
        A1[rows, sel] = 1.0
        tag = f"one-hot rows {rows} k* {sel}"
        out = _gemm_launch(ext, c, A1, B, bias, Y, C0, gen, fails, tag,
                           zero_rest=True)
        ref, tol = _gemm_bound(c, A1, B, bias, Y, C0)
        ok, w = _worst((out.double() - ref).abs(), tol)
        fails.check(ok, f"{tag}: error is {w:.3g} x the bound")
        worst = max(worst, w)
        if c.act != 2 and not c.dact:
            # exact: the accumulator holds B[k*, :] (or 0) with no rounding,
            # then at most one fp32 add each for bias and accumulate, then
            # round-to-nearest-even to bf16 — all reproducible bit for bit
            exp = torch.zeros(M, N, dtype=torch.float32, device=device)
            exp[rows] = Bmat[sel].float()
            if c.bias:
                exp = exp + bias
            if c.accum:
                exp = C0 + exp
            if c.act == 1:
                exp = exp.to(torch.bfloat16)
            fails.check(torch.equal(out, exp), f"{tag}: not bitwise exact")
    return {"ok": not fails, "worst": worst, "fails": list(fails)}


# ---------------------------------------------------------------------------
# wgrad
# ---------------------------------------------------------------------------
def _wgrad_launch(ext, c: WgradCase, X_log, dY, gen, fails, tag, zero_rest=False):
    dev = X_log.device
    pd = None
    X_src = X_log
    if c.perm_mult:
        X_src, pd = _source_slab(c, X_log, gen, dev, zero_rest)
    gX, gdY = guarded_copy(X_src), guarded_copy(dY)
    kw = _perm_kwargs(pd) if pd else {}
    res = {}
    for reduce in (False, True):
        # everything NaN: an element the kernels do not write fails
        gWp = Guarded((c.slabs, c.K, c.N), torch.float32, dev)
        gW = Guarded((c.K, c.N), torch.float32, dev)
        gbp = Guarded((c.slabs, c.N), torch.float32, dev) if c.db else None
        gb = Guarded((c.N,), torch.float32, dev) if c.db else None
        ext.wgrad(gX.t, gdY.t, gWp.t, gbp.t if c.db else None, gW.t,
                  gb.t if c.db else None, c.slabs, reduce=reduce, **kw)
        _sync(dev)
        for name, g in (("X", gX), ("dY", gdY), ("dW_part", gWp), ("dW", gW),
                        ("db_part", gbp), ("db", gb)):
            if g is not None:
                fails.check(g.intact(),
                            f"{tag} reduce={reduce}: guard band of {name} changed")
        res[reduce] = (gWp.t, gbp.t if c.db else None, gW.t,
                       gb.t if c.db else None)
    Wp0, bp0, W0, b0 = res[False]
    Wp1, bp1, W1, b1 = res[True]
    fails.check(bool(torch.isnan(W0).all()) and (b0 is None or bool(torch.isnan(b0).all())),
                f"{tag}: reduce=False wrote dW/db")
    fails.check(torch.equal(Wp0, Wp1) and (bp0 is None or torch.equal(bp0, bp1)),
                f"{tag}: slab partials differ between reduce=False and True")
    return Wp0, bp0, W1, b1


def _wgrad_bound(c: WgradCase, X_log, dY):
    """Per-slab and total fp64 references with their tolerances."""
    mps = -(-c.M // c.slabs)
    pad = c.slabs * mps - c.M
    Xd = torch.nn.functional.pad(X_log.double(), (0, 0, 0, pad))
    Yd = torch.nn.functional.pad(dY.double(), (0, 0, 0, pad))
    Xs = Xd.view(c.slabs, mps, c.K).transpose(1, 2)
    Ys = Yd.view(c.slabs, mps, c.N)
    ref_p = torch.bmm(Xs, Ys)
    S_p = torch.bmm(Xs.abs(), Ys.abs())
    refb_p = Ys.sum(1)
    Sb_p = Ys.abs().sum(1)
    fp, ft = (mps + 2) * U, (mps + c.slabs + 2) * U
    return {"dW_part": (ref_p, fp * S_p), "db_part": (refb_p, fp * Sb_p),
            "dW": (ref_p.sum(0), ft * S_p.sum(0)),
            "db": (refb_p.sum(0), ft * Sb_p.sum(0))}


def _check_wgrad(c, outs, X_log, dY, fails, tag):
    Wp, bp, W, b = outs
    bound = _wgrad_bound(c, X_log, dY)
    worst = 0.0
    got = {"dW_part": Wp, "dW": W}
    if c.db:
        got.update({"db_part": bp, "db": b})
    for name, t in got.items():
        ref, tol = bound[name]
        ok, w = _worst((t.double() - ref).abs(), tol)
        fails.check(ok, f"{tag}: {name} error is {w:.3g} x the bound")
        worst = max(worst, w)
    return worst


def run_wgrad_case(ext, c: WgradCase, variant: str, device="cuda", seed=0) -> dict:
    """Random operands against the fp64 bounds (every slab and the total),
    then one-hot probes: X zero except X[m*, k*] = 1, so dW[k*, :] is
    dY[m*, :] exactly, in the slab that owns m* and in the total."""
    fails = Failures()
    gen = torch.Generator().manual_seed(2000 + seed)
    M, K, N = c.M, c.K, c.N
    X = _randn_bf16((M, K), gen, 1.0, device)
    dY = _randn_bf16((M, N), gen, 0.1, device)
    outs = _wgrad_launch(ext, c, X, dY, gen, fails, "random")
    worst = _check_wgrad(c, outs, X, dY, fails, "random")

    mps = -(-M // c.slabs)
    TK = 32 * int(variant.split("_")[2].split("x")[0])
    first_live = K - K % TK if K % TK else 0
    rows = sorted({m for m in (0, mps - 1, mps, M - 1) if 0 <= m < M})
    ks = []
    for k in (0, first_live, K - 1, 33, 5, 7, 11):
        if 0 <= k < K and k not in ks and len(ks) < 4:
            ks.append(k)
    for s in range(len(ks)):
        sel = [ks[(j + s) % len(ks)] for j in range(len(rows))]
        X1 = torch.zeros(M, K, dtype=torch.bfloat16, device=device)
        X1[rows, sel] = 1.0
        tag = f"one-hot m* {rows} k* {sel}"
        Wp, bp, W, b = _wgrad_launch(ext, c, X1, dY, gen, fails, tag, zero_rest=True)
        worst = max(worst, _check_wgrad(c, (Wp, bp, W, b), X1, dY, fails, tag))
        expW = torch.zeros(K, N, dtype=torch.float32, device=device)
        expWp = torch.zeros(c.slabs, K, N, dtype=torch.float32, device=device)
        expW[sel] = dY[rows].float()
        expWp[[m // mps for m in rows], sel] = dY[rows].float()
        fails.check(torch.equal(W, expW), f"{tag}: dW not bitwise exact")
        fails.check(torch.equal(Wp, expWp), f"{tag}: dW_part not bitwise exact")
    return {"ok": not fails, "worst": worst, "fails": list(fails)}


# ---------------------------------------------------------------------------
# forced-knob child
# ---------------------------------------------------------------------------
def child_main() -> int:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from gymfx_amd.ops import native

    ext = native.require()
    report = {"knobs": knob_ints(os.environ), "cases": []}
    for i, c in enumerate(CHILD_GEMM):
        name, grid = gemm_variant(ext, c)
        r = run_gemm_case(ext, c, seed=i)
        report["cases"].append({"op": "gemm", "id": c.id, "variant": name,
                                "grid": list(grid), **r})
    for i, c in enumerate(CHILD_WGRAD):
        name, grid = wgrad_variant(ext, c)
        r = run_wgrad_case(ext, c, name, seed=i)
        report["cases"].append({"op": "wgrad", "id": c.id, "variant": name,
                                "grid": list(grid), **r})
    report["variants"] = sorted({x["variant"] for x in report["cases"]})
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    if sys.argv[1:] == ["--child"]:
        sys.exit(child_main())
    sys.exit("usage: mfma_cases.py --child")
