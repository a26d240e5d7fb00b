"""Exact-answer, per-element tests of the mid self-attention kernels
(dv_mqa_prep / dv_mqa_fwd / dv_mqa_fwd_fp8 / dv_mqa_bwd through ops.mqa) on
the closed-form inputs of tests/mqa_cases.py (proved against float64 attention
in tests/test_mqa_cases_host.py).  Every element of every result is held to
its closed form on its own -- no norms -- so one wrong query row, one wrong
key row, or one key too many or too few in the softmax fails.  B = 2 and the
clips carry different code books, so the clip offset matters.

Clip lengths (N keys + the null key, padded to NKP):
    31 /   32  one full tile, no mask; second key half empty; half-filled last query group
    32 /   64  the last tile holds one valid key
    95 /   96  odd tile count, no pad
    96 /  128  one valid key in the last tile, even tile count
    97 /  128  N odd again
   160 /  192  161 = 7 * 23 (the selection multiplier must not be 7)
  1279 / 1280  the LDS limit (largest whole-clip-in-LDS forward and bf16 backward)
  1280 / 1312  streamed: chunks of 512, 512, 288 keys (9 tiles: odd count last)
  1535 / 1536  three full chunks, no mask
  1536 / 1568  the last chunk is one tile with one valid key

Coverage (regime: B = bounded scores, no running max; O = online max.  Every
path sees lengths with pad keys and without -- 31, 95, 1279, 1535 have none):
    path                      kernels                       bounded            online
    LDS forward (bf16)        mqa_fwd_fa                    flat 0, +-32       flat +-64, select   N <= 1279
    streamed forward (bf16)   mqa_fwd_fa_stream             flat 0, +-32       flat +-64, select   N >= 1280
    fp8 forward               mqa_v8 + mqa_fwd_fa_stream8   (online only: every family)           N >= 1280
    f32 forward               mqa_fwd<float>                (one regime: every family)            every N
    LDS backward (bf16)       mqa_dq_fa, mqa_dkdv_fa,       flat 0, -32        select              N <= 1279
                              mqa_finish_fa                 (lse from the bounded / online forward)
    f32 backward              mqa_bwd_d, mqa_dq, mqa_dkdv,  flat 0, -32        select              every N (f32);
                              mqa_finish <float>                                                  N >= 1280 (bf16 in/out)
The fp8 kernel is only taken at NKP > 1280 (ops.mqa_fp8_ok), i.e. at the three
streamed lengths; at N = 1279 (NKP = 1280) ops.mqa stays on the bf16 LDS kernel.

Tolerances -- derived from the arithmetic, none from a run (u = 2^-8 is the
largest relative error of one round-to-nearest to bf16):
  forward     p is 0, 1 or one constant, V is 0 / 1: the f32 accumulations are
              exact integer sums times that constant; one f32 reciprocal and one
              rounding of the output remain:
                  bf16, fp8: |o - e| <= 2^-8 |e| + 1e-6      f32: <= 2e-6 |e| + 1e-6.
              One rounding more in the code: in the bounded regime p = exp2(score)
              is not shifted by a max, so flat +-32 has p = 2^+-46.25, which the
              PV MFMA takes rounded to bf16 while the row sum l adds the f32
              value: every output is scaled by bf16(p) / p (1 + 1.44e-3 at +32,
              1 - 1.25e-3 at -32; mqa_cases.flat_p_rounding -- v_exp_f32's own
              error cannot move that rounding, 2^0.25 * 128 = 152.2 and
              2^0.75 * 128 = 215.3 are far from a tie).  For bf16 at those two
              levels the bound is (2^-8 + |bf16(p) / p - 1|) |e| + 1e-6.
  selection   dV sums a few dozen integers <= 3: exact in bf16 and f32 -> 1e-5
  backward    absolute.  dQ, dK, dnull[0] are 0 up to the 2^-46 leak (about 2e-7) -> 1e-5.
  flat        p = 1 / (N + 1) recomputed from lse, rounded to bf16 for the MFMA
  backward    (u, the same for every entry), the result rounded to bf16 (u):
                  bf16: |dV - e| <= 2^-7 |e|.
              f32 (mqa_dkdv_kernel<float>): p = expf(s - L) carries the roundings
              of L = m + logf(l), of the product with log2 e and of v_log / v_exp,
              together < 4e-6 relative; then each wave adds its 2 heads' p * dO
              terms to one f32 accumulator one after the other (n = 2 * 32 *
              ceil(N / 32) additions, 8 atomic adds join the waves).  All terms
              are positive multiples of ONE constant p, so the roundings do not
              average out (the same additions in numpy give +2.2e-5 at 1,537
              keys, -1.7e-5 at 1,281): the bound is the worst case n 2^-24,
                  f32: |dV - e| <= (4e-6 + (n + 8 + B) 2^-24) |e|   (+ B: dnull sums the clips)
              -- 8e-6 at N = 31, 1.9e-4 at N = 1536, where one key more or less
              still moves dV by 6.5e-4.  (A flat 2e-5 does not hold from about
              1,281 keys on; the kernel is right, the sum is that long.)
              dnull[1] is stored in f32, but on the bf16 LDS path it is the
              sum of the SAME MFMA results, so it carries p's rounding:
              (2^-8 + 2e-5) |e| there; the f32 bound above where the f32
              kernels run (f32, and bf16 at NKP > 1280).
  flat 0      dK and dnull[0] are exact zeros (q = 0) -> 1e-5.  dQ = scale * sum_j dS_j
  dQ, dK      with dS_j = p (dP_j - D): zero in exact arithmetic; the kernel's D =
              dO . o uses the stored o (relative error <= u in bf16, 2e-6 in
              f32) and dS is rounded to bf16 (u) for the MFMA, |dP_j - D| <=
              sum_d dO_d; the stored keys carry bf16(scale log2 e) (+0.2 %):
                  bf16: |dQ| <= scale * 1.01 * 2 u * sum_d dO_d + 1e-6
                  f32:  |dQ| <= scale * 2e-5 * sum_d dO_d + 1e-6.
"""
import pytest
import torch

import mqa_cases as mc

pytestmark = pytest.mark.gpu

B = 2
NS = (31, 32, 95, 96, 97, 160, 1279, 1280, 1535, 1536)
FP8_NS = tuple(N for N in NS if mc.nkp(N) > 1280)  # where ops.mqa takes dv_mqa_fwd_fp8
FAMILIES = tuple(str(c) for c in mc.FLAT_LEVELS) + ("select",)
BWD_FAMILIES = ("0", "-32", "select")
DTYPES = [torch.bfloat16, torch.float32]
U = 2.0 ** -8


def _ids(v):
    return {torch.bfloat16: "bf16", torch.float32: "f32"}.get(v, str(v))


def _dev(t, dtype, grad=False):
    return t.to("cuda", dtype).requires_grad_(grad)


def check(got, want, rel, abs_, what, case, row_kind, pi=None):
    """Every element: |got - want| <= rel * |want| + abs_ (rel, abs_ may be tensors that
    broadcast).  On failure names the worst element: clip, token, head, dim, key tile.
    Returns the worst deviation and the worst deviation / allowance."""
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{case.name} N={case.N} {what}: non-finite values"
    dev = (got - want).abs()
    ratio = dev / (rel * want.abs() + abs_)
    worst = int(ratio.argmax())
    if float(ratio.flatten()[worst]) > 1.0:
        r, c = divmod(worst, want.shape[-1]) if want.dim() == 2 else (0, worst)
        N = case.N
        if row_kind == "query":  # (B * N, H * 32)
            clip, tok, head, dim = r // N, r % N, c // mc.D, c % mc.D
            key = int(pi[clip, tok * mc.H + head]) if pi is not None else None
            where = (f"clip {clip} token {tok} head {head} dim {dim}"
                     + (f", selected key {key} (key tile {key // 32})" if key is not None else ""))
        elif row_kind == "key":  # (B * N, 32 or 64): token t is key t + 1
            clip, tok = r // N, r % N
            where = f"clip {clip} token {tok} dim {c} (key {tok + 1}, key tile {(tok + 1) // 32})"
        else:  # dnull: key 0
            where = f"dim {c} (key 0, key tile 0)"
        nbad = int((ratio > 1.0).sum())
        pytest.fail(f"{case.name} N={N} NKP={mc.nkp(N)} {what}: {nbad} of {ratio.numel()} elements off; worst at "
                    f"{where}: got {float(got.flatten()[worst])!r}, expected {float(want.flatten()[worst])!r}, "
                    f"allowed {float((rel * want.abs() + abs_).flatten()[worst]):.3e}")
    return float(dev.max()), float(ratio.max())


def fwd_tol(dtype, case, fp8=False):
    if dtype == torch.float32:
        return 2e-6, 1e-6
    extra = 0.0
    if not fp8 and case.name.startswith("flat"):
        extra = mc.flat_p_rounding(int(case.name[4:]))  # the bounded regime's bf16(p) / p
    return U + extra, 1e-6


def f32_flat_bwd_rel(N):
    """Flat family, f32 dk/dv kernel: p's own error plus the worst case of the sequential f32
    additions behind one dV element (module docstring); dnull[1] adds the B clips as well."""
    n = (mc.H // 8) * 32 * ((N + 31) // 32)  # per wave: H / 8 heads x whole 32-row query tiles
    return 4e-6 + (n + 8 + B) * 2.0 ** -24


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("family", FAMILIES)
def test_mqa_forward_exact(parity_log, family, N, dtype):
    from dalle2_video import ops

    case = mc.build(family, B, N)
    with torch.no_grad():
        o = ops.mqa(_dev(case.q, dtype), _dev(case.kv, dtype), _dev(case.null_kv, torch.float32), B, N, mc.H,
                    mc.SCALE)
    assert o.dtype == dtype
    rel, abs_ = fwd_tol(dtype, case)
    dev, ratio = check(o, case.o, rel, abs_, "o", case, "query", case.pi)
    parity_log(family=family, N=N, dtype=_ids(dtype), fwd_max_dev=dev, fwd_dev_over_bound=ratio)


@pytest.mark.parametrize("N", FP8_NS)
@pytest.mark.parametrize("family", FAMILIES)
def test_mqa_forward_fp8_exact(parity_log, family, N):
    """p in {0, 1} (x 128, the block scale) and V in {0, 1} are exact in e4m3, and the fp8
    kernel always subtracts the max: the bf16 expectations hold at the one-rounding bound."""
    from dalle2_video import ops

    case = mc.build(family, B, N)
    q, kv = _dev(case.q, torch.bfloat16), _dev(case.kv, torch.bfloat16)
    null_kv = _dev(case.null_kv, torch.float32)
    with torch.no_grad():
        ops.TIMER = ops.KernelTimer()
        try:
            with ops.mx8_convs(attention=True):
                o = ops.mqa(q, kv, null_kv, B, N, mc.H, mc.SCALE)
            names = set(ops.TIMER.summary())
        finally:
            ops.TIMER = None
    assert "attn:mqa_fwd8" in names, names  # the fp8 kernel ran, not the bf16 one
    rel, abs_ = fwd_tol(torch.bfloat16, case, fp8=True)
    dev, ratio = check(o, case.o, rel, abs_, "o (fp8 PV)", case, "query", case.pi)
    parity_log(family=family, N=N, dtype="fp8", fwd_max_dev=dev, fwd_dev_over_bound=ratio)


@pytest.mark.parametrize("dtype", DTYPES, ids=_ids)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("family", BWD_FAMILIES)
def test_mqa_backward_exact(parity_log, family, N, dtype):
    from dalle2_video import ops

    case = mc.build(family, B, N)
    q, kv = _dev(case.q, dtype, True), _dev(case.kv, dtype, True)
    null_kv = _dev(case.null_kv, torch.float32, True)
    gy = mc.upstream(B, N)
    o = ops.mqa(q, kv, null_kv, B, N, mc.H, mc.SCALE)
    (o.float() * gy.to("cuda", torch.float32)).sum().backward()
    bf16 = dtype == torch.bfloat16
    f32_kernels = not bf16 or mc.nkp(N) > ops.MQA_BF16_BWD_MAX_NKP  # bf16 past the LDS limit: cast to f32
    log = dict(family=family, N=N, dtype=_ids(dtype), f32_kernels=f32_kernels)

    # the forward that autograd recorded (f32 kernels, output cast to bf16, past the LDS limit)
    if bf16 and f32_kernels:
        rel, abs_ = U + 2e-6, 1e-6
    else:
        rel, abs_ = fwd_tol(dtype, case)
    log["fwd_max_dev"], _ = check(o, case.o, rel, abs_, "o (grad mode)", case, "query", case.pi)

    dkv, dnull = kv.grad, null_kv.grad
    assert q.grad.dtype == dtype and dkv.dtype == dtype and dnull.dtype == torch.float32
    if family == "select":
        log["dv_max_dev"], _ = check(dkv[:, mc.D:], case.dv, 0.0, 1e-5, "dV", case, "key")
        log["dnull_v_max_dev"], _ = check(dnull[1], case.dnull_v, 0.0, 1e-5, "dnull[1]", case, "null")
        log["dq_max_dev"], _ = check(q.grad, case.dq, 0.0, 1e-5, "dQ", case, "query", case.pi)
        log["dk_max_dev"], _ = check(dkv[:, :mc.D], case.dkv[:, :mc.D], 0.0, 1e-5, "dK", case, "key")
        log["dnull_k_max_dev"], _ = check(dnull[0], case.dnull[0], 0.0, 1e-5, "dnull[0]", case, "null")
    else:
        rel_f32 = f32_flat_bwd_rel(N)
        log["dv_max_dev"], log["dv_dev_over_bound"] = check(
            dkv[:, mc.D:], case.dv, 2 * U if bf16 else rel_f32, 0.0, "dV", case, "key")
        rel_null = rel_f32 if f32_kernels else U + 2e-5
        log["dnull_v_max_dev"], log["dnull_v_dev_over_bound"] = check(
            dnull[1], case.dnull_v, rel_null, 0.0, "dnull[1]", case, "null")
        if family == "0":
            sum_do = gy.reshape(B * N, mc.H, mc.D).sum(-1, keepdim=True).expand(B * N, mc.H, mc.D)
            dq_abs = mc.SCALE * (1.01 * 2 * U if bf16 else 2e-5) * sum_do.reshape(B * N, mc.H * mc.D) + 1e-6
            log["dq_max_dev"], log["dq_dev_over_bound"] = check(
                q.grad, case.dq, 0.0, dq_abs, "dQ", case, "query")
            log["dk_max_dev"], _ = check(dkv[:, :mc.D], case.dkv[:, :mc.D], 0.0, 1e-5, "dK", case, "key")
            log["dnull_k_max_dev"], _ = check(dnull[0], case.dnull[0], 0.0, 1e-5, "dnull[0]", case, "null")
    parity_log(**log)
