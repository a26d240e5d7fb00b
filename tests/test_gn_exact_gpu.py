"""Exact-answer, per-element tests of every GroupNorm kernel path of
dv_norm.hip (gn_reduce_kernel, gn_apply_kernel, gn_coop_kernel through
ops.group_norm_act, dv_gn_fwd and dv_gn_bwd) on the closed-form inputs of
tests/gn_cases.py (proved against float64 F.group_norm + autograd in
tests/test_gn_cases_host.py).  Every element of every output is held to its
own expectation -- no norms, nothing sampled -- so one wrong channel vector,
a wrong clamped tail row, a replica dropped or counted twice, a neighbour's
statistics or a store past the end fails and is named (clip, pixel, channel).

Launch facts are recomputed here from the tune constants read out of
dv_norm.hip (gn_tune(), GN_U) with mirrors of gn_rows, gn_replicas,
gn_direct_ok / gn_direct_dq and gn_coop_plan, and asserted against the
table: a retune that moves a shape off its path fails instead of silently
losing coverage.

Coverage (P = pixels per clip; bf16: VEC 8, f32: VEC 4; tpr = C / VEC threads
per row, rpp = 256 / tpr rows per pass; "blocks" = forward reduce workgroups
per clip, R = sums replicas, DQ = the bf16 forward apply's register prologue
width, 0 = LDS prologue):
  row  nb, P, C, G        bf16 fwd: blocks R DQ   what it pins
  1    2, 37, 64, 8        1  1 1   less than one pass: only clamped tail rows
  2    2, 4133, 64, 8     17  2 1   R = 2, a tail block, direct prologue DQ 1
  3    2, 3617, 512, 8   114  8 0   R = 8; tpr 64 refuses direct (R > 4): split LDS
                                    prologue (gn_terms_issue / finish); f32 tpr 128
  4    3, 1000, 256, 8    16  1 1   three clips (clip offsets), tpr 32
  5    2, 50, 48, 8        1  1 0   C/G = 6: not DIR, not direct; tpr 6 leaves 4 idle
                                    threads (act_rows); reduce `pre` LDS prologue
  6    3, 70, 1024, 32     5  1 0   C > 512: gn_group_terms, stage_params, `pre` off;
                                    f32 rpp = 1
  7    2, 300, 8, 1        1  1 1   one group; bf16 tpr 1, rpp 256: the shuffle fold
  8    2, 130, 512, 64     5  1 1   G = 64, C/G = 8
  8f   2, 130, 64, 64 f32           C/G = 1 (a bf16 vector cannot hold one group)
Reduce kernels: forward U = 8, backward U = 4.  The backward reduce takes the
register prologue (DIR) where C/G % VEC == 0 -- every row but 5 and 8f -- and
else the LDS prologue with the `pre` pre-loads (C <= 512): row 5 in both
types (6 % 8, 6 % 4 != 0) and row 8f.
Apply kernels: forward U = 4, backward U = 2, SILU x RES instantiations through
the act / residual variants; the backward apply always takes the LDS prologue.
  A  rows 1, 3, 5 through the raw ABI: ld = C + 16 slices at channel offset 8,
     two guard rows, own sums / next, accumulate 0 and 1
  B  pre-summed statistics, nb 2, P 256 (bf16 DQ; f32 always LDS):
       C 64   R 1, 3, 8 -> DQ 1;  R 9 -> DQ 2 (f32: gn_group_terms' 8-at-a-time
              loop, second round);  R 64 -> direct refused, gn_group_terms, 8 rounds
       C 256  R 3 -> DQ 2;  R 8 -> DQ 4
       C 512  R 3 -> DQ 4;  R 8 -> split LDS prologue
       C 1024, G 32, R 2 -> gn_group_terms
  C  single launch gn_coop_kernel (bf16; dv_gn_path 3, and 2 = its bounded
     wait's fallback), nb 16, C 64, P 100 / 1100 / 2100 / 4200 / 8200 -> NV 1 / 2 /
     4 / 8 / 16 with k = 2 / 9 / 9 / 9 / 9 workgroups per clip, the last one partial;
     nb 2, C 512, P 70 -> NV 1, k 9.  The backward keeps dy in registers (KEEPX)
     at every NV; P = 8200 also runs the backward in automatic mode, the one
     class production sends here.

Tolerances -- derived from the arithmetic, none from a run (u = 2^-8):
  two-level statistics.  z / s is an integer <= 9, so the per-channel f32
      sums of z and z^2 are exact in any order (threads, LDS, atomics,
      replicas); the group terms are formed in double: mean = m, var = s^2,
      rstd = 1 / s come out exactly, on the single launch too (its sums cross
      workgroups through the same f32 atomics): mean, rstd bit for bit.
  two-level y, act NONE.  A, B and z A + B are exact in f32 (host test):
      f32 y bit for bit; bf16 y = the round-to-nearest-even bf16 of it.
  two-level y, SiLU.  v is exact; sigmoid2 and the product add, relative to
      silu(v): the multiply by -log2 e (its rounding and the constant's, an
      absolute error in the exponent, hence a relative error <= 1.25 |v| 2^-24
      in exp2), v_exp_f32 at 1 ulp (2 x 2^-24), the add, v_rcp_f32 at 1 ulp (2),
      the multiply by v: (6 + 1.25 |v|) 2^-24 <= 7 (1 + |v|) 2^-24, k = 7; the
      residual add rounds the result once more, k = 8.  With a residual the
      error is relative to |silu(v)|, not to |e| = |silu(v) + res|: res >= 1/2
      keeps |e| >= 0.22 and the test asserts, element by element, that the
      derived error 7 (1 + |v|) 2^-24 |silu(v)| + 2^-24 |e| is inside the bound
          f32:  k 2^-24 (1 + |v|) |e| + 1e-6        bf16: 2^-8 |e| + 1e-6.
  two-level dz, act NONE.  dv = dy, zhat = +-1 and the per-channel sums are
      exact; gamma' s1 summed over the group is exact (2^24 bound asserted in
      gn_cases).  Roundings left: m1 = sum / n and m2 = sum / n (correctly
      rounded divisions), then dv K1 + m1' (one fma) and + zhat m2' (one fma),
      each of a value <= S = rstd (|gamma' dv| + |m1| + |m2|): k' = 4,
          f32:  4 2^-24 S        bf16:  + 2^-8 |e|   (the stored rounding).
  two-level dgamma, dbeta, dss (f32 outputs).  gamma s2 + beta s1 is a product
      and an fma; sc s2 a product, then one atomic add per clip: k'' = 2 + nb,
          k'' 2^-24 |e|   (every one of these roundings is in fact exact here).
  Gaussian y, dz (SiLU and NONE): d = 8 x the largest per-element error of
      F.group_norm + FiLM + act (+ autograd) evaluated in f32 on the CPU against
      float64 on the same input (the kernels sum in one pass, torch does not);
          f32:  d        bf16:  2^-8 |e| + d.
      Both numbers are recorded with parity_log; the kernels' output never
      sets the bound.  The SiLU gradient is checked on this family.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import gn_cases as gc

pytestmark = pytest.mark.gpu

U = 2.0 ** -8
E24 = 2.0 ** -24
BF16, F32 = torch.bfloat16, torch.float32
BOTH = (BF16, F32)
ROW_DTYPES = {"1": BOTH, "2": BOTH, "3": BOTH, "4": BOTH, "5": BOTH, "6": BOTH, "7": BOTH, "8": BOTH, "8f": (F32,)}
# row -> (forward reduce workgroups per clip, R, DQ) in bf16
ROW_PLAN = {"1": (1, 1, 1), "2": (17, 2, 1), "3": (114, 8, 0), "4": (16, 1, 1), "5": (1, 1, 0), "6": (5, 1, 0),
            "7": (1, 1, 1), "8": (5, 1, 1)}
# part B: (C, G, R) -> bf16 DQ
PRESUM_DQ = {(64, 8, 1): 1, (64, 8, 3): 1, (64, 8, 8): 1, (64, 8, 9): 2, (64, 8, 64): 0, (256, 8, 3): 2,
             (256, 8, 8): 4, (512, 8, 3): 4, (512, 8, 8): 0, (1024, 32, 2): 0}
# part C: (nb, P, C) -> (NV, workgroups per clip)
COOP_PLAN = {(16, 100, 64): (1, 2), (16, 1100, 64): (2, 9), (16, 2100, 64): (4, 9), (16, 4200, 64): (8, 9),
             (16, 8200, 64): (16, 9), (2, 70, 512): (1, 9)}
VARIANTS = [(act, film, res) for act in (gc.ACT_NONE, gc.ACT_SILU) for film in (False, True) for res in (False, True)]
SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dalle2-video_amd", "csrc",
                   "dv_norm.hip")


def _ids(v):
    return {BF16: "bf16", F32: "f32"}.get(v, str(v))


def _vid(v):
    act, film, res = v
    return ("silu" if act else "none") + ("-film" if film else "") + ("-res" if res else "")


# ---- launch facts (mirrors of dv_norm.hip's host planning) ----------------------------------
@functools.lru_cache(maxsize=None)
def tune():
    """gn_tune(): (ur0, ua0, ur1, ua1, tr0, ta0, tr1, ta1), read from the source."""
    txt = open(SRC).read()
    names = {k: int(re.search(r"constexpr int %s = (\d+);" % k, txt).group(1)) for k in ("GN_U", "GN_DQ", "GN_CT")}
    body = re.search(r"static const GnTune t\{([^}]*)\}", txt).group(1)
    vals = [int(eval(x, {"__builtins__": {}}, names)) for x in body.split(",")]
    assert len(vals) == 8
    return dict(zip(("ur0", "ua0", "ur1", "ua1", "tr0", "ta0", "tr1", "ta1"), vals), **names)


def vec_of(dtype):
    return 8 if dtype == BF16 else 4


def gn_rows(nb, P, C, vec, u, target):
    pass_ = (256 // (C // vec)) * u
    r = -(-(P * nb) // target)
    r = -(-r // pass_) * pass_
    return max(r, pass_)


def fwd_reduce_plan(nb, P, C, dtype, cap=8):
    """(workgroups per clip, R) of the forward reduce; cap = replicas the sums buffer holds (<= 8)."""
    t = tune()
    blocks = -(-P // gn_rows(nb, P, C, vec_of(dtype), t["ur0"], t["tr0"]))
    return blocks, max(1, min((blocks + 15) // 16, 8, cap))


def direct_dq(C, G, R, dtype):
    """DQ of the forward apply (0: LDS prologue)."""
    if dtype != BF16:
        return 0
    tpr, cg = C // 8, C // G
    if not (tpr <= 64 and tpr & (tpr - 1) == 0 and cg % 8 == 0 and R <= tune()["GN_DQ"] * (64 // tpr)):
        return 0
    nq = -(-R // (64 // tpr))
    return 1 if nq <= 1 else 2 if nq <= 2 else 4


def coop_plan(nb, P, C):
    """(NV, workgroups per clip) of the single launch."""
    rpp = tune()["GN_CT"] // (C // 8)
    kmax = 256 // nb
    nvmin = -(-P // (kmax * rpp))
    assert nvmin <= 16
    nv = next(v for v in (1, 2, 4, 8, 16) if nvmin <= v)
    return nv, -(-P // (nv * rpp))


def test_rows_reach_the_paths_the_table_names():
    for row, (blocks, R, dq) in ROW_PLAN.items():
        nb, P, C, G = gc.ROWS[row]
        assert fwd_reduce_plan(nb, P, C, BF16) == (blocks, R), row
        assert direct_dq(C, G, R, BF16) == dq, row
    for (C, G, R), dq in PRESUM_DQ.items():
        assert direct_dq(C, G, R, BF16) == dq, (C, G, R)
    for (nb, P, C), plan in COOP_PLAN.items():
        assert coop_plan(nb, P, C) == plan, (nb, P, C)
        rpw = plan[0] * (tune()["GN_CT"] // (C // 8))
        assert plan[1] > 1 and P % rpw != 0  # k > 1 workgroups per clip, the last one partial
    # the automatic backward takes the single launch only at NV = 16
    assert coop_plan(16, 8200, 64)[0] == 16
    # row 1 is less than one pass; rows 2 and 3 end in a partial block; f32 row 6 has one row per pass
    t = tune()
    assert gc.ROWS["1"][1] < (256 // 8) * t["ua0"]
    for row in ("2", "3"):
        nb, P, C, G = gc.ROWS[row]
        assert P % gn_rows(nb, P, C, 8, t["ur0"], t["tr0"]) != 0
    assert 256 // (1024 // 4) == 1


# ---- comparison ---------------------------------------------------------------------------
def check(got, want, bound, what, ctx):
    """Every element: |got - want| <= bound (a tensor that broadcasts, or a number).  On
    failure names the worst element.  Returns (largest deviation, largest deviation / bound)."""
    got = got.detach().double().cpu().reshape(want.shape)
    assert bool(torch.isfinite(got).all()), f"{ctx} {what}: non-finite values"
    dev = (got - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(dev)
    over = dev - bound
    if bool((over > 0).any()):
        worst = int(over.argmax())
        idx = tuple(int(i) for i in np.unravel_index(worst, tuple(dev.shape)))
        names = ("clip", "pixel", "channel") if dev.dim() == 3 else ("index",) * dev.dim()
        where = ", ".join(f"{n} {i}" for n, i in zip(names, idx))
        pytest.fail(f"{ctx} {what}: {int((over > 0).sum())} of {dev.numel()} elements off; worst at {where}: got "
                    f"{float(got.flatten()[worst])!r}, expected {float(want.flatten()[worst])!r}, allowed "
                    f"{float(bound.flatten()[worst]):.3e}")
    ratio = torch.where(bound > 0, dev / bound.clamp_min(1e-300), dev)
    return float(dev.max()), float(ratio.max())


def stored(want, dtype):
    """The closed form as the kernel stores it: exact in f32, round-to-nearest-even in bf16."""
    return want.float().to(dtype).double()


def y_bound(exp, act, res, dtype):
    """act NONE: 0 (bit exact against stored()); SiLU: the module docstring's bound, after
    asserting that the derived error of every element is inside it."""
    if act == gc.ACT_NONE:
        return 0.0
    e, v = exp["y"].abs(), exp["v"].abs()
    derived = 7 * E24 * (1 + v) * gc.silu(exp["v"]).abs() + (E24 * e if res else 0.0)
    if dtype == F32:
        bound = (8 if res else 7) * E24 * (1 + v) * e + 1e-6
    else:
        bound = U * e + 1e-6
        derived = derived * (1 + U) + 2.0 ** -9 * e
    assert bool((derived <= bound).all()), "the derived SiLU error exceeds the stated bound"
    return bound


def dz_bound(exp, dtype):
    b = 4 * E24 * exp["S"]
    return b + U * exp["dz"].abs() if dtype == BF16 else b


@functools.lru_cache(maxsize=2)
def expectation(family, shape, act, film, res):
    return gc.build(family, *shape).expect(act, film, res)


def dev_t(t, dtype, grad=False):
    return t.contiguous().to("cuda", dtype).requires_grad_(grad)


def run_ops(case, dtype, act, film, res, backward):
    """ops.group_norm_act (nf = nb, h = 1, w = P) and, if asked, its backward.  Returns the
    outputs and the `next` buffers of the forward and the backward call."""
    from dalle2_video import ops

    nb, P, C, G = case.nb, case.P, case.C, case.G
    z = dev_t(case.z.reshape(nb, 1, P, C), dtype, backward)
    gamma, beta = dev_t(case.gamma, F32, backward), dev_t(case.beta, F32, backward)
    ss = dev_t(case.ss, F32, backward) if film else None
    r = dev_t(case.res.reshape(nb, 1, P, C), dtype) if res else None
    ws = ops._gn_sums(z.device)
    out = {"next_fwd": ws.bufs[(ws.i + 2) % 3]}
    with torch.set_grad_enabled(backward):
        y = ops.group_norm_act(z, gamma, beta, nb, G, case.eps, scale_shift=ss, res=r, act=act)
        if backward:
            saved = y.grad_fn.saved_tensors
            out["mean"], out["rstd"] = saved[4], saved[5]
            out["next_fwd_zero"] = bool((out["next_fwd"] == 0).all())
            out["next_bwd"] = ws.bufs[(ws.i + 2) % 3]
            (y.float() * case.dy.reshape(nb, 1, P, C).to("cuda", F32)).sum().backward()
            out.update(dz=z.grad, dgamma=gamma.grad, dbeta=beta.grad)
            if film:
                out["dss"] = ss.grad
            assert z.grad.dtype == dtype
    torch.cuda.synchronize()
    assert y.dtype == dtype
    out["y"] = y.detach()
    return out


def check_two_level(case, exp, got, dtype, act, film, res, ctx, log):
    nb = case.nb
    log["y_dev"], log["y_dev_over_bound"] = check(
        got["y"], stored(exp["y"], dtype) if act == gc.ACT_NONE else exp["y"], y_bound(exp, act, res, dtype),
        "y", ctx)
    if "mean" in got:
        check(got["mean"].reshape(nb, case.G), exp["mean"], 0.0, "mean", ctx)
        check(got["rstd"].reshape(nb, case.G), exp["rstd"], 0.0, "rstd", ctx)
    if "dz" in got:
        log["dz_dev"], log["dz_dev_over_bound"] = check(got["dz"], exp["dz"], dz_bound(exp, dtype), "dz", ctx)
        k2 = (2 + nb) * E24
        for k in ("dgamma", "dbeta") + (("dss",) if film else ()):
            log[k + "_dev"], _ = check(got[k], exp[k], k2 * exp[k].abs(), k, ctx)


# ---- the table: every row x FiLM x residual x activation ------------------------------------
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
@pytest.mark.parametrize("row", sorted(ROW_DTYPES))
def test_gn_two_level_exact(parity_log, row, variant):
    """Forward in both activations; mean / rstd and the backward with act NONE (dv = dy keeps
    the sums exact; the SiLU gradient is test_gn_gaussian's)."""
    act, film, res = variant
    shape = gc.ROWS[row]
    case, exp = gc.build("two", *shape), expectation("two", shape, act, film, res)
    for dtype in ROW_DTYPES[row]:
        ctx = f"row {row} {shape} {_ids(dtype)} {_vid(variant)}"
        got = run_ops(case, dtype, act, film, res, backward=act == gc.ACT_NONE)
        log = dict(row=row, dtype=_ids(dtype), variant=_vid(variant))
        check_two_level(case, exp, got, dtype, act, film, res, ctx, log)
        if "next_bwd" in got:
            assert got["next_fwd_zero"] and bool((got["next_bwd"] == 0).all()), f"{ctx}: `next` not zeroed"
        else:
            assert bool((got["next_fwd"] == 0).all()), f"{ctx}: `next` not zeroed"
        parity_log(**log)


@functools.lru_cache(maxsize=1)
def gaussian_reference(shape, act, film, res):
    """(float64 expectation, d per output): d = 8 x the largest error of the f32 CPU reference."""
    case = gc.build("gauss", *shape)
    exp, r32 = case.expect(act, film, res), gc.reference(case, act, film, res, F32)
    d = {k: 8 * float((r32[k].double() - exp[k]).abs().max()) for k in ("y", "dz")}
    return exp, d


@pytest.mark.parametrize("variant", [(gc.ACT_SILU, True, False), (gc.ACT_SILU, False, True), (gc.ACT_NONE, True, True)],
                         ids=_vid)
@pytest.mark.parametrize("row", ["1", "2", "3", "4", "5", "6", "7", "8", "8f"])
def test_gn_gaussian(parity_log, row, variant):
    act, film, res = variant
    shape = gc.ROWS[row]
    case = gc.build("gauss", *shape)
    exp, d = gaussian_reference(shape, act, film, res)
    for dtype in ROW_DTYPES[row]:
        ctx = f"gaussian row {row} {shape} {_ids(dtype)} {_vid(variant)}"
        got = run_ops(case, dtype, act, film, res, backward=True)
        log = dict(row=row, dtype=_ids(dtype), variant=_vid(variant), y_ref_f32_err=d["y"] / 8,
                   dz_ref_f32_err=d["dz"] / 8)
        for k in ("y", "dz"):
            bound = d[k] + (U * exp[k].abs() if dtype == BF16 else 0.0)
            print(f"{ctx} {k}: reference f32 error {d[k] / 8:.3e}, allowance d = {d[k]:.3e}")
            log[k + "_dev"], log[k + "_dev_over_bound"] = check(got[k], exp[k], bound, k, ctx)
        parity_log(**log)


# ---- A: the whole-call contract through the raw ABI -----------------------------------------
SENT = 12352.0  # exact in bf16
PAD, OFF, GUARD = 16, 8, 2


class Slab:
    """A (rows + GUARD, C + PAD) buffer full of the sentinel; the tensor lives in the channel
    slice [OFF, OFF + C) of the first `rows` rows."""

    def __init__(self, rows, C, dtype, data=None):
        self.rows, self.C = rows, C
        self.buf = torch.full((rows + GUARD, C + PAD), SENT, dtype=dtype, device="cuda")
        if data is not None:
            self.buf[:rows, OFF:OFF + C] = data.reshape(rows, C).to("cuda", dtype)
        self.before = self.buf.clone()
        self.ld = C + PAD

    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + OFF * self.buf.element_size())

    def data(self):
        return self.buf[:self.rows, OFF:OFF + self.C]

    def outside_untouched(self, inside_too=False):
        a, b = self.buf.clone(), self.before.clone()
        if not inside_too:
            a[:self.rows, OFF:OFF + self.C] = 0
            b[:self.rows, OFF:OFF + self.C] = 0
        return torch.equal(a, b)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def raw_fwd(dtype, z, y, res, nb, P, C, G, eps, gamma, beta, ss, act, mean, rstd, sums, nxt, replicas):
    from dalle2_video import _lib

    is_slab = isinstance(z, Slab)
    _lib.call("dv_gn_fwd", _lib.DV_BF16 if dtype == BF16 else _lib.DV_F32,
              z.ptr() if is_slab else _p(z), z.ld if is_slab else C, y.ptr() if is_slab else _p(y),
              y.ld if is_slab else C, None if res is None else (res.ptr() if is_slab else _p(res)),
              0 if res is None else (res.ld if is_slab else C), nb, P, C, G, ctypes.c_float(eps), _p(gamma),
              _p(beta), _p(ss), act, _p(mean), _p(rstd), _p(sums), _p(nxt), nxt.numel(), replicas, _lib.stream())
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", BOTH, ids=_ids)
@pytest.mark.parametrize("act", [gc.ACT_NONE, gc.ACT_SILU], ids=["none", "silu"])
@pytest.mark.parametrize("row", ["1", "3", "5"])
def test_gn_whole_call_contract(parity_log, row, act, dtype):
    from dalle2_video import _lib

    shape = nb, P, C, G = gc.ROWS[row]
    film, res = True, True
    case, exp = gc.build("two", *shape), expectation("two", shape, act, film, res)
    ctx = f"raw row {row} {shape} {_ids(dtype)} act {act}"
    rows = nb * P
    z, r, dy = Slab(rows, C, dtype, case.z), Slab(rows, C, dtype, case.res), Slab(rows, C, dtype, case.dy)
    y, dz = Slab(rows, C, dtype), Slab(rows, C, dtype)
    gamma, beta, ss = dev_t(case.gamma, F32), dev_t(case.beta, F32), dev_t(case.ss, F32)
    mean = torch.full((nb * G,), float("nan"), device="cuda")
    rstd = mean.clone()
    rstride = nb * C * 2
    n = 8 * rstride + nb
    sums, nxt = torch.zeros(n, device="cuda"), torch.ones(n, device="cuda")
    raw_fwd(dtype, z, y, r, nb, P, C, G, 0.0, gamma, beta, ss, act, mean, rstd, sums, nxt, 0)
    assert bool((nxt == 0).all()), f"{ctx}: forward left `next` unzeroed"
    # `sums` is not re-zeroed: its replicas hold the clip's per-channel totals, exactly
    _, R = fwd_reduce_plan(nb, P, C, dtype)
    tot = sums[:8 * rstride].reshape(8, nb, C, 2)
    assert bool((tot[R:] == 0).all()), f"{ctx}: a replica past R = {R} was written"
    check(tot.sum(0)[..., 0], case.z.sum(1), 0.0, "sums[.., 0]", ctx)
    check(tot.sum(0)[..., 1], (case.z * case.z).sum(1), 0.0, "sums[.., 1]", ctx)
    got = dict(y=y.data().reshape(nb, P, C), mean=mean, rstd=rstd)
    log = dict(row=row, dtype=_ids(dtype), act=act)
    check_two_level(case, exp, got, dtype, act, film, res, ctx, log)
    assert y.outside_untouched(), f"{ctx}: y written outside its slice (padding or guard rows)"
    for name, s in (("z", z), ("res", r)):
        assert s.outside_untouched(inside_too=True), f"{ctx}: {name} modified"

    if act == gc.ACT_NONE:
        pre = ((torch.arange(C) % 5).double() - 2) / 4  # a dyadic pre-fill
        for accumulate in (0, 1):
            fill = float("nan") if not accumulate else 0.0
            dgamma = torch.full((C,), fill, device="cuda") + (pre.to("cuda", F32) if accumulate else 0)
            dbeta = dgamma.clone()
            dss = torch.full((nb, 2 * C), float("nan"), device="cuda")
            sums2, nxt2 = torch.zeros(n, device="cuda"), torch.ones(n, device="cuda")
            dz.buf.copy_(dz.before)
            _lib.call("dv_gn_bwd", _lib.DV_BF16 if dtype == BF16 else _lib.DV_F32, dy.ptr(), dy.ld, z.ptr(), z.ld,
                      dz.ptr(), dz.ld, nb, P, C, G, _p(gamma), _p(beta), _p(ss), act, _p(mean), _p(rstd),
                      _p(dgamma), _p(dbeta), _p(dss), _p(sums2), _p(nxt2), n, accumulate, _lib.stream())
            torch.cuda.synchronize()
            c2 = f"{ctx} accumulate {accumulate}"
            assert bool((nxt2 == 0).all()), f"{c2}: backward left `next` unzeroed"
            add = pre if accumulate else torch.zeros(C, dtype=torch.float64)
            k2 = (2 + nb + accumulate) * E24
            log["dz_dev"], _ = check(dz.data().reshape(nb, P, C), exp["dz"], dz_bound(exp, dtype), "dz", c2)
            check(dgamma, exp["dgamma"] + add, k2 * (exp["dgamma"] + add).abs(), "dgamma", c2)
            check(dbeta, exp["dbeta"] + add, k2 * (exp["dbeta"] + add).abs(), "dbeta", c2)
            check(dss, exp["dss"], k2 * exp["dss"].abs(), "dss", c2)
            assert dz.outside_untouched(), f"{c2}: dz written outside its slice (padding or guard rows)"
            for name, s in (("z", z), ("dy", dy)):
                assert s.outside_untouched(inside_too=True), f"{c2}: {name} modified"
    parity_log(**log)


# ---- B: pre-summed statistics ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", BOTH, ids=_ids)
@pytest.mark.parametrize("C,G,R", gc.PRESUM)
def test_gn_presummed_statistics(parity_log, C, G, R, dtype):
    nb, P = gc.PRESUM_NB, gc.PRESUM_P
    shape = (nb, P, C, G)
    act, film, res = gc.ACT_NONE, True, True
    case, exp = gc.build("two", *shape), expectation("two", shape, act, film, res)
    ctx = f"presum {shape} R {R} {_ids(dtype)} (DQ {direct_dq(C, G, R, dtype)})"
    z, r = dev_t(case.z.reshape(nb * P, C), dtype), dev_t(case.res.reshape(nb * P, C), dtype)
    y = torch.full((nb * P + GUARD, C), SENT, dtype=dtype, device="cuda")
    sums = gc.presums(case, R).to("cuda", F32).reshape(-1).contiguous()
    nxt = torch.ones_like(sums)
    mean = torch.full((nb * G,), float("nan"), device="cuda")
    rstd = mean.clone()
    raw_fwd(dtype, z, y, r, nb, P, C, G, 0.0, dev_t(case.gamma, F32), dev_t(case.beta, F32), dev_t(case.ss, F32),
            act, mean, rstd, sums, nxt, R)
    assert bool((nxt == 0).all()), f"{ctx}: `next` not zeroed"
    assert bool((y[nb * P:] == SENT).all()), f"{ctx}: a store past the last row"
    log = dict(C=C, R=R, dtype=_ids(dtype))
    check_two_level(case, exp, dict(y=y[:nb * P].reshape(nb, P, C), mean=mean, rstd=rstd), dtype, act, film, res,
                    ctx, log)
    parity_log(**log)


# ---- C: the single launch -------------------------------------------------------------------
# forced (3), its fallback (2); automatic (0) where production takes the single launch: the NV = 16 backward
COOP_RUNS = [(s, path) for s in gc.COOP for path in (3, 2)] + [(gc.COOP[4], 0)]


@pytest.mark.parametrize("shape,path", COOP_RUNS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"path{v}")
def test_gn_single_launch_exact(parity_log, shape, path):
    from dalle2_video import _lib

    nb, P, C, G = shape
    act, film, res = gc.ACT_NONE, True, True
    case, exp = gc.build("two", *shape), expectation("two", shape, act, film, res)
    ctx = f"single launch {shape} path {path} NV {coop_plan(nb, P, C)[0]}"
    _lib.call("dv_gn_path", path)
    try:
        got = run_ops(case, BF16, act, film, res, backward=True)
    finally:
        _lib.call("dv_gn_path", 0)
    log = dict(shape=list(shape), path=path)
    check_two_level(case, exp, got, BF16, act, film, res, ctx, log)
    # `next`, with the nb arrival counters at its end, is zero after the forward and the backward
    assert got["next_fwd_zero"] and bool((got["next_bwd"] == 0).all()), f"{ctx}: `next` / counters not zeroed"
    parity_log(**log)


@pytest.mark.parametrize("shape", [gc.COOP[1], gc.COOP[5]], ids=lambda s: "x".join(map(str, s)))
def test_gn_single_launch_silu_forward(parity_log, shape):
    from dalle2_video import _lib

    nb, P, C, G = shape
    act, film, res = gc.ACT_SILU, True, False
    case, exp = gc.build("two", *shape), expectation("two", shape, act, film, res)
    for path in (3, 2):
        _lib.call("dv_gn_path", path)
        try:
            got = run_ops(case, BF16, act, film, res, backward=False)
        finally:
            _lib.call("dv_gn_path", 0)
        log = dict(shape=list(shape), path=path)
        check_two_level(case, exp, got, BF16, act, film, res, f"single launch {shape} path {path} silu", log)
        parity_log(**log)
