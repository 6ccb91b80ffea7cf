"""GPU: every instantiated gemm_kernel / wgrad_glds_kernel /
wgrad_partial_kernel variant against an fp64 reference.

The fused-kernel tests prove bitwise equality with the launch sequences they
replace; those chains end at the MFMA GEMM, the wgrad kernels and the slab
reduce.  This module anchors that end: each variant runs at the smallest
shapes that reach its edges, on guard-banded buffers, against
``A.double() @ B.double()`` with an elementwise bound derived from the
number formats (tests/mfma_cases.py), plus one-hot probes that must come out
bit for bit.  Tile knobs are read once per process, so forced-knob variants
run in fresh child processes that report as JSON."""
import json
import os
import subprocess
import sys

import pytest
import torch

import mfma_cases as mc

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT_S = 240


def _ext():
    from gymfx_amd.ops import native

    return native.require()


# ---------------------------------------------------------------------------
# in-process: default knobs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(mc.INPROC_GEMM)),
                         ids=[c.id for c in mc.INPROC_GEMM])
def test_gemm_variant_vs_fp64(i):
    ext, c = _ext(), mc.INPROC_GEMM[i]
    name, grid = mc.gemm_variant(ext, c)
    assert c.expect in name, f"case no longer reaches {c.expect}: {name}"
    r = mc.run_gemm_case(ext, c, seed=i)
    print(f"{c.id} -> {name} grid {grid}: worst error {r['worst']:.3g} x bound")
    assert r["ok"], "\n".join(r["fails"])


@pytest.mark.parametrize("i", range(len(mc.INPROC_WGRAD)),
                         ids=[c.id for c in mc.INPROC_WGRAD])
def test_wgrad_variant_vs_fp64(i):
    ext, c = _ext(), mc.INPROC_WGRAD[i]
    name, grid = mc.wgrad_variant(ext, c)
    assert name == c.expect, f"case no longer reaches {c.expect}: {name}"
    r = mc.run_wgrad_case(ext, c, name, seed=i)
    print(f"{c.id} -> {name} grid {grid}: worst error {r['worst']:.3g} x bound")
    assert r["ok"], "\n".join(r["fails"])


# ---------------------------------------------------------------------------
# forced knobs: fresh child processes, one after another
# ---------------------------------------------------------------------------
_reports = {}
_abnormal = []  # index of a child that ended by signal / timeout / error


def _child_report(idx):
    if idx in _reports:
        return _reports[idx]
    if _abnormal:
        pytest.skip(f"forced-knob child {_abnormal[0]} ended abnormally; "
                    "no further child is launched")
    env = {k: v for k, v in os.environ.items()
           if not any(k in e for e in mc.CHILD_KNOBS)}
    env.update(mc.CHILD_KNOBS[idx])
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else [])
    cmd += [os.path.abspath(mc.__file__), "--child"]
    try:
        p = subprocess.run(cmd, env=env, capture_output=True, text=True,
                           timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        _abnormal.append(idx)
        pytest.fail(f"child {idx} ({mc.CHILD_KNOBS[idx]}) timed out")
    if p.returncode != 0:
        _abnormal.append(idx)
        pytest.fail(f"child {idx} ({mc.CHILD_KNOBS[idx]}) exited with "
                    f"{p.returncode}:\n{p.stderr[-2000:]}")
    _reports[idx] = json.loads(p.stdout.strip().splitlines()[-1])
    return _reports[idx]


@pytest.mark.parametrize("idx", range(len(mc.CHILD_KNOBS)),
                         ids=["-".join(f"{k[6:]}={v}" for k, v in e.items())
                              for e in mc.CHILD_KNOBS])
def test_forced_knob_child(idx):
    assert len(mc.CHILD_KNOBS) <= 4
    ext = _ext()
    rep = _child_report(idx)
    kn = mc.knob_ints(mc.CHILD_KNOBS[idx])
    assert rep["knobs"] == kn
    want = [("gemm", c.id, mc.gemm_variant(ext, c, kn)) for c in mc.CHILD_GEMM]
    want += [("wgrad", c.id, mc.wgrad_variant(ext, c, kn)) for c in mc.CHILD_WGRAD]
    assert len(rep["cases"]) == len(want)
    bad = []
    for got, (op, cid, (name, grid)) in zip(rep["cases"], want):
        print(f"{op} {cid} -> {got['variant']} grid {got['grid']}: "
              f"worst error {got['worst']:.3g} x bound")
        # the child launched what the query predicts for its knobs
        assert (got["op"], got["id"]) == (op, cid)
        assert (got["variant"], tuple(got["grid"])) == (name, tuple(grid))
        if not got["ok"]:
            bad.append(f"{op} {cid} [{name}]: " + "; ".join(got["fails"]))
    assert not bad, "\n".join(bad)
    # one gather-fused GEMM ran under this child's forced wide / mid tile
    assert any(g["variant"].endswith("_perm1") and g["op"] == "gemm"
               for g in rep["cases"])


def test_every_instantiation_was_exercised():
    """The variants the in-process cases launch under this process's knobs,
    plus the ones the children report having launched, are exactly the
    extension's list of instantiations."""
    ext = _ext()
    hit = {mc.gemm_variant(ext, c)[0] for c in mc.INPROC_GEMM}
    hit |= {mc.wgrad_variant(ext, c)[0] for c in mc.INPROC_WGRAD}
    for idx in range(len(mc.CHILD_KNOBS)):
        hit |= set(_child_report(idx)["variants"])
    listed = set(ext.mfma_variants())
    assert hit == listed, (f"never run: {sorted(listed - hit)}; "
                           f"not listed: {sorted(hit - listed)}")


# ---------------------------------------------------------------------------
# transpose_bf16 / f32_to_bf16: exact
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", [(4, 256), (256, 4), (68, 132), (260, 256),
                                 (64, 64)])
def test_transpose_bf16_exact(K, N):
    ext = _ext()
    g = torch.Generator().manual_seed(K * 1000 + N)
    src = mc.guarded_copy(torch.randn(K, N, generator=g).to(torch.bfloat16).cuda())
    dst = mc.Guarded((N, K), torch.bfloat16, "cuda")
    ext.transpose_bf16(src.t, dst.t)
    torch.cuda.synchronize()
    assert src.intact() and dst.intact()
    assert torch.equal(dst.t, src.t.t().contiguous())


def _f32_specials():
    bits = [
        0x00000000, 0x80000000,              # +-0
        0x7F800000, 0xFF800000,              # +-inf
        0x7F7F0000, 0xFF7F0000,              # largest finite bf16
        0x7F7F8000, 0xFF7F8000,              # tie above it: to even = inf
        0x7F7FFFFF, 0xFF7FFFFF,              # FLT_MAX rounds up to inf
        0x7F7F7FFF,                          # just below the tie: stays finite
        0x3F808000, 0xBF808000,              # tie, even below: rounds down
        0x3F818000, 0xBF818000,              # tie, even above: rounds up
        0x3F808001, 0x3F817FFF,              # either side of a tie
        0x3FFF8000,                          # tie that carries into the exponent
        0x00808000, 0x00818000,              # ties at the smallest normals
    ]
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)


@pytest.mark.parametrize("n", [1, 255, 257, 100003])
def test_f32_to_bf16_exact(n):
    ext = _ext()
    g = torch.Generator().manual_seed(n)
    # random values over the whole exponent range, and random exact ties
    x = torch.randn(n, generator=g) * torch.exp2(
        torch.randint(-100, 100, (n,), generator=g).float())
    ties = (torch.randint(0x0080, 0x7F7F, (n,), generator=g, dtype=torch.int32)
            << 16 | 0x8000).view(torch.float32)
    x = torch.where(torch.rand(n, generator=g) < 0.25, ties, x)
    sp = _f32_specials()
    k = min(n, sp.numel())
    # n == 1 takes a tie; the larger sizes hold every special value
    x[:k] = sp[:k] if n > 1 else sp[11:12]
    src = mc.guarded_copy(x.cuda())
    dst = mc.Guarded((n,), torch.bfloat16, "cuda")
    ext.f32_to_bf16(src.t, dst.t)
    torch.cuda.synchronize()
    assert src.intact() and dst.intact()
    want = x.to(torch.bfloat16)  # CPU round-to-nearest-even
    assert torch.equal(dst.t.cpu().view(torch.int16), want.view(torch.int16))
