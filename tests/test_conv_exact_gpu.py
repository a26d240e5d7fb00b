"""Bit-exact conv forward / dgrad / wgrad on integer operands.

A convolution of small integers has an exactly representable answer: every
product and every partial sum, in any order, is an integer far below 2^24, so
f32 accumulation is exact whatever the tiling, split or summation order.  The
only inexact step left is the final bf16 store, and round-to-nearest-even of an
integer is unique -- so a kernel's output must equal the float64 reference BIT
FOR BIT, element by element.  One wrong pixel, one dropped tap at a corner, a
truncating epilogue: each is a failure here, where the relative-L2 checks of
test_conv_gpu.py move by a fraction of their tolerance (the CPU self-check at
the end of this file shows it on the reference alone).

Contract under test ("bias + residual fused"): accumulate in f32,
add bias and residual in f32, round once.  One family rounds twice by
construction and is held to exactly that: the dual-source stripe conv runs as
two passes through the bf16 output (see `expected_forward`).

Every case asserts its own routing with the dispatch mirrors of ops.py, so a
later change of the dispatch rules cannot silently drop a family from here.
"""
import functools
import types

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32

# ---------------------------------------------------------------------------
# case tables: (nf, h, w, c0, c1, cout, k), the family the forward must land in,
# the family its input gradient must land in (chosen as ConvFn.backward does)
# ---------------------------------------------------------------------------
FWD_CASES = [
    # resident-weight stripe kernel (64 input channels, W in {32, 64, 128})
    ((2, 8, 32, 64, 0, 128, 3), BF16, "conv_fwd_stripe_kernel<32>", "conv_fwd_glds_kernel"),  # two cout tiles
    ((2, 4, 64, 64, 0, 64, 3), BF16, "conv_fwd_stripe_kernel<64>", "conv_fwd_stripe_kernel<64>"),
    ((2, 3, 128, 64, 0, 64, 3), BF16, "conv_fwd_stripe_kernel<128>", "conv_fwd_stripe_kernel<128>"),  # one-row stages
    # five stages per workgroup: the 6-slot row ring wraps inside a frame (fewer
    # stages never reuse a slot; with <= 256 / (cout / 64) stages each workgroup has one)
    ((2, 40, 128, 64, 0, 896, 3), BF16, "conv_fwd_stripe_kernel<128>", "conv_fwd_glds_kernel"),
    # dual source 64 + 64: two stripe passes (the double rounding of expected_forward)
    ((2, 4, 64, 64, 64, 64, 3), BF16, "conv_fwd_stripe_kernel<64>", "conv_fwd_stripe_kernel<64>"),
    # window ("frame") kernel at 8^2 and 16^2
    ((4, 8, 8, 48, 16, 64, 3), BF16, "conv_fwd_frame_kernel<8>", "conv_fwd_frame_kernel<8>"),  # split at a 16-channel boundary
    ((64, 8, 8, 64, 0, 64, 3), BF16, "conv_fwd_frame_kernel<8>", "conv_fwd_frame_kernel<8>"),  # M = 4096: 32 tiles
    ((2, 8, 8, 768, 0, 512, 3), BF16, "conv_fwd_frame_kernel<8>", "conv_fwd_frame_kernel<8>"),  # K = 6912: 48 chunks
    ((64, 8, 8, 64, 0, 320, 3), BF16, "conv_fwd_frame_kernel<8>", "conv_fwd_frame_kernel<8>"),  # the tap-split form
    ((64, 8, 8, 48, 16, 320, 3), BF16, "conv_fwd_frame_kernel<8>", "conv_fwd_frame_kernel<8>"),  # tap split, dual source
    ((2, 8, 16, 128, 0, 64, 3), BF16, "conv_fwd_frame_kernel<16>", "conv_fwd_frame_kernel<16>"),
    ((16, 16, 16, 64, 0, 384, 3), BF16, "conv_fwd_frame_kernel<16>", "conv_fwd_frame_kernel<16>"),  # 64-channel tiles
    ((16, 16, 16, 64, 0, 640, 3), BF16, "conv_fwd_frame_kernel<16>", "conv_fwd_frame_kernel<16>"),  # 8 waves x 128 channels
    # 1x1 streaming kernel: dual source, 297 pixels (ragged last tile)
    ((3, 9, 11, 64, 64, 64, 1), BF16, "conv1x1_stream_kernel<64,2>", "conv1x1_stream_kernel<128,1>"),
    # glds implicit GEMM: ragged pixel and channel tiles; K = 6912 (three frames: no whole
    # 128-pixel tile, which the window kernel would take); cout 3 (the scalar epilogue)
    ((3, 9, 11, 128, 64, 192, 3), BF16, "conv_fwd_glds_kernel", "conv_fwd_glds_kernel"),
    ((3, 8, 8, 768, 0, 512, 3), BF16, "conv_fwd_glds_kernel", "conv_fwd_glds_kernel"),
    ((2, 6, 6, 64, 0, 3, 1), BF16, "conv_fwd_glds_kernel", "conv_fwd_kernel<bf16"),
    # register-staged kernel (cin % 64 != 0)
    ((3, 5, 7, 16, 8, 40, 3), BF16, "conv_fwd_kernel<bf16", "conv_fwd_kernel<bf16"),
    ((2, 6, 6, 24, 0, 3, 1), BF16, "conv_fwd_kernel<bf16", "conv_fwd_kernel<bf16"),
    # small-channel direct kernel (dv_conv_small_fwd): CP 16; a padded output tile
    ((2, 5, 32, 8, 8, 8, 3), BF16, "xe_fwd_kernel", "xe_fwd_kernel"),
    ((1, 6, 32, 16, 0, 24, 7), BF16, "xe_fwd_kernel", "conv_fwd_kernel<bf16"),
    # f32 kernels
    ((3, 5, 7, 16, 8, 40, 3), F32, "conv_fwd_kernel<float", "conv_fwd_kernel<float"),
    ((2, 8, 8, 64, 0, 64, 3), F32, "conv_fwd_kernel<float", "conv_fwd_kernel<float"),
]

# forms of the window kernel the cases above must reach: ops.frame_tile's
# (channels per workgroup, waves, tap split) of the forward
FRAME_FORMS = {
    (4, 8, 8, 48, 16, 64, 3): (32, 4, False),
    (64, 8, 8, 64, 0, 64, 3): (32, 4, False),
    (2, 8, 8, 768, 0, 512, 3): (32, 4, False),
    (64, 8, 8, 64, 0, 320, 3): (64, 8, True),
    (64, 8, 8, 48, 16, 320, 3): (64, 8, True),
    (2, 8, 16, 128, 0, 64, 3): (32, 4, False),
    (16, 16, 16, 64, 0, 384, 3): (64, 4, False),
    (16, 16, 16, 64, 0, 640, 3): (128, 8, False),
}

WGRAD_CASES = [
    ((16, 8, 8, 128, 0, 128, 3), BF16, "conv_wgrad_win_kernel<8>"),
    ((8, 16, 16, 64, 64, 64, 3), BF16, "conv_wgrad_win_kernel<16>"),  # the shape class the round-6 race appeared in
    ((8, 32, 32, 64, 0, 64, 3), BF16, "conv_wgrad_win_kernel<32>"),
    ((2, 64, 64, 64, 64, 64, 3), BF16, "conv_wgrad_win_kernel<64>"),
    # four stages per split: the 3-deep stage ring wraps and the halves sum follows a
    # multi-stage loop (every case above has one stage per split)
    ((8, 16, 16, 512, 0, 512, 3), BF16, "conv_wgrad_win_kernel<16>"),
    ((32, 8, 8, 256, 256, 512, 3), BF16, "conv_wgrad_win_kernel<8>"),
    ((8, 16, 16, 128, 0, 64, 1), BF16, "conv_wgrad_1x1_kernel"),
    ((8, 16, 16, 64, 64, 128, 1), BF16, "conv_wgrad_1x1_kernel"),
    ((3, 9, 11, 128, 64, 64, 3), BF16, "conv_wgrad_glds_kernel<64,128>"),
    ((2, 7, 5, 256, 0, 64, 3), BF16, "conv_wgrad_glds_kernel<64,256>"),
    ((3, 9, 11, 128, 64, 192, 3), BF16, "conv_wgrad_glds_kernel<128,128>"),
    # odd cin in bf16 is the glds kernel too (a ragged K tile: K = 216); the register-staged
    # conv_wgrad_kernel<bf16> runs only past 2^31 elements, a size no quick test reaches
    ((3, 5, 7, 16, 8, 40, 3), BF16, "conv_wgrad_glds_kernel<64,128>"),
    ((3, 5, 7, 16, 8, 40, 3), F32, "conv_wgrad_kernel<float>"),
]
WGRAD_STAGES_PER_SPLIT = {(8, 16, 16, 512, 0, 512, 3): 4, (32, 8, 8, 256, 256, 512, 3): 4}


def _id(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    if isinstance(v, torch.dtype):
        return "bf16" if v == BF16 else "f32"
    return None


# ---------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------
def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def mismatches(got, want):
    """(count, first few (index..., got, want)) of the elements whose bits differ."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = (bits(got) != bits(want)).nonzero()
    first = [tuple(i.tolist()) + (got[tuple(i)].item(), want[tuple(i)].item()) for i in bad[:8]]
    return bad.shape[0], first


def assert_bits_equal(got, want, what):
    if torch.equal(bits(got), bits(want)):
        return
    n, first = mismatches(got, want)
    raise AssertionError(f"{what}: {n} of {want.numel()} elements differ; first (index..., got, want): {first}")


def rne(ref, dtype):
    """The one rounding of the contract: the exact (float64, integer) value to f32
    (exact below 2^24), then round-to-nearest-even to the dtype.  (+ 0.0: the
    reference's zeros carry no sign.)"""
    return (ref + 0.0).float().to(dtype)


def needs_rounding(ref):
    return (ref.float().bfloat16().double() != ref).double().mean().item()


# ---------------------------------------------------------------------------
# operands and the float64 reference (CPU only)
# ---------------------------------------------------------------------------
def ints(g, shape, a):
    return torch.randint(-a, a + 1, shape, generator=g).double()


def conv_ref(x, wt, k):
    """float64 F.conv2d over channels-last frames."""
    return F.conv2d(x.permute(0, 3, 1, 2), wt[:, :, 0], padding=k // 2).permute(0, 2, 3, 1)


@functools.lru_cache(maxsize=2)
def fwd_problem(case, dtype, full):
    """Operands (float64 integers) and the reference of one forward / dgrad case.
    full: with bias (integer f32 in +-600) and residual (bf16-representable
    integers in +-1023: every integer to 256, even ones to 512, multiples of 4
    beyond), large on purpose -- at K = 576 the bare conv stays below 256 and
    nothing would round.  The gradient has no residual: dY is drawn from +-4
    where 9 cout >= 1152, so some of its elements round as well."""
    nf, h, w, c0, c1, cout, k = case
    cin = c0 + c1
    g = torch.Generator().manual_seed(1000 + sum(case) + 7 * int(full))
    x = ints(g, (nf, h, w, cin), 2)
    wt = ints(g, (cout, cin, 1, k, k), 2)
    a_dy = 4 if 9 * cout >= 1152 else 2
    dy = ints(g, (nf, h, w, cout), a_dy)
    bias = ints(g, (cout,), 600) if full else None
    res = ints(g, (nf, h, w, cout), 1023).bfloat16().double() if full else None
    xr = x.clone().requires_grad_()
    conv = conv_ref(xr, wt, k)
    y = conv.detach()
    if full:
        y = y + bias + res
    conv.backward(dy)
    dx = xr.grad
    p = types.SimpleNamespace(x=x, wt=wt, dy=dy, bias=bias, res=res, y=y, dx=dx)
    # conditions on the reference alone
    assert max(y.abs().max().item(), dx.abs().max().item()) < 2 ** 24  # K A^2 + 1623 <= 8064 * 8 + 1623
    assert (y == y.round()).all() and (dx == dx.round()).all()
    p.y_rounds, p.dx_rounds = needs_rounding(y), needs_rounding(dx)
    if dtype == BF16 and full:
        assert p.y_rounds >= 0.01, p.y_rounds  # the rounding mode is really exercised
    return p


def expected_forward(p, case, dtype, family):
    """What the forward must store.  Every family but one: the exact value
    rounded ONCE.  The dual-source stripe conv (64 + 64 input channels at
    W in {32, 64, 128}) runs as two passes of the single-source kernel --
    pass 1 stores bf16(conv(x0, w[:, :64]) + bias + res), pass 2 reads it back
    as its residual and stores bf16(pass 1 + conv(x1, w[:, 64:])) -- so the
    first source's sum is rounded to bf16 before the second is added.
    That is not an epilogue reorder (the intermediate goes through the bf16
    output tensor), so exactly this family is held to its two roundings."""
    nf, h, w, c0, c1, cout, k = case
    if family.startswith("conv_fwd_stripe_kernel") and c1:
        y1 = conv_ref(p.x[..., :c0], p.wt[:, :c0], k)
        if p.bias is not None:
            y1 = y1 + p.bias + p.res
        y1 = rne(y1, dtype).double()
        return rne(y1 + conv_ref(p.x[..., c0:], p.wt[:, c0:], k), dtype)
    return rne(p.y, dtype)


def wgrad_problem_uncached(case):
    """x, dY in {0, 1}: every split-K partial of every split is at most the
    final value, so with dW, db <= 256 the bf16 partials of the window / 1x1
    wgrads are exact and the f32 gradient must equal the reference exactly."""
    nf, h, w, c0, c1, cout, k = case
    cin, m = c0 + c1, nf * h * w
    p_dy = min(0.5, 128 / m)
    p_x = min(0.5, 32 / (m * p_dy))
    g = torch.Generator().manual_seed(2000 + sum(case))
    x = (torch.rand(nf, h, w, cin, generator=g) < p_x).double()
    dy = (torch.rand(nf, h, w, cout, generator=g) < p_dy).double()
    dw = torch.nn.grad.conv2d_weight(x.permute(0, 3, 1, 2), (cout, cin, k, k), dy.permute(0, 3, 1, 2),
                                     padding=k // 2)[:, :, None]
    db = dy.sum((0, 1, 2))
    assert dw.max().item() <= 256 and db.max().item() <= 256, (dw.max().item(), db.max().item())
    assert dw.mean().item() >= 8, dw.mean().item()  # not a sparse near-zero gradient
    return types.SimpleNamespace(x=x, dy=dy, dw=dw, db=db)


wgrad_problem = functools.lru_cache(maxsize=2)(wgrad_problem_uncached)


# ---------------------------------------------------------------------------
# routing, from the mirrors of ops.py (shape / dtype only: runs without a GPU)
# ---------------------------------------------------------------------------
def probe(dtype, shape):
    """What the mirrors read of a tensor: a contiguous, 16-B aligned device tensor."""
    return types.SimpleNamespace(dtype=dtype, shape=shape, is_cuda=True, data_ptr=lambda: 0)


def dname(dtype):
    return "bf16" if dtype == BF16 else "float"


def fwd_family(ops, case, dtype, has_res):
    """As ConvFn.forward chooses."""
    nf, h, w, c0, c1, cout, k = case
    cin, m = c0 + c1, nf * h * w
    x0 = probe(dtype, (nf, h, w, c0))
    x1 = probe(dtype, (nf, h, w, c1)) if c1 else None
    ldr = cout if has_res else 0
    if ops.small_conv_ok(x0, x1, cin, cin, cout, c0, c1, ldr, k, w):
        return "xe_fwd_kernel"
    if ops.window_ok(x0, x1, cin, c0 if c1 else cin, cout, c0, c1 or c0, cout, ldr, k, h, w, nf):
        return f"conv_fwd_frame_kernel<{w}>"
    return ops.conv_fwd_name(dname(dtype), m, cin, c0 if c1 else cin, cout, max(c0, c1), k, h, w)


def dgrad_family(ops, case, dtype):
    """As ConvFn.backward chooses for a contiguous dY, no sink, no parked skips."""
    nf, h, w, c0, c1, cout, k = case
    cin, m = c0 + c1, nf * h * w
    cout8 = (cout + 7) // 8 * 8  # dY padded to 8 channels
    dy8 = probe(dtype, (nf, h, w, cout8))
    if dtype == BF16 and cout <= 16 and cin <= 32 and k % 2 == 1 and k <= 15 and w % 32 == 0 and cin % 4 == 0:
        return "xe_fwd_kernel"
    if ops.window_ok(dy8, None, cout8, cout8, cin, cout8, cout8, cin, 0, k, h, w, nf):
        return f"conv_fwd_frame_kernel<{w}>"
    return ops.conv_fwd_name(dname(dtype), m, cout8, cout8, cin, cout8, k, h, w)


def wgrad_family(ops, case, dtype):
    """As ConvFn.backward chooses (none of the cases is the cross-embed wgrad's:
    a single source of <= 8 channels)."""
    nf, h, w, c0, c1, cout, k = case
    cin, m = c0 + c1, nf * h * w
    assert c1 or cin > 8
    cout8 = (cout + 7) // 8 * 8
    maxld = max(cout8, c0, c1)
    if cout8 == cout:
        return ops.conv_wgrad_name(dname(dtype), m, cout8, cin, c0, bool(c1), k, h, w, maxld)
    return ops.gemm_wgrad_name(dname(dtype), m, cout8, cin * k * k, maxld)


def check_fwd_routing(ops, case, dtype, fam_f, fam_d, full):
    nf, h, w, c0, c1, cout, k = case
    assert fwd_family(ops, case, dtype, full).startswith(fam_f), (case, fwd_family(ops, case, dtype, full))
    assert dgrad_family(ops, case, dtype).startswith(fam_d), (case, dgrad_family(ops, case, dtype))
    if fam_f.startswith("conv_fwd_frame_kernel"):
        assert ops.frame_tile(nf * h * w, w, cout) == FRAME_FORMS[case], (case, ops.frame_tile(nf * h * w, w, cout))


def test_case_tables_route_as_stated():
    """Every row of both tables lands in the family it names (no GPU needed: the
    mirrors read shapes and dtypes only), every family of the conv paths has a
    row, and the multi-stage rows really run several stages per workgroup."""
    from dalle2_video import ops

    for case, dtype, fam_f, fam_d in FWD_CASES:
        for full in (True, False):
            check_fwd_routing(ops, case, dtype, fam_f, fam_d, full)
    for case, dtype, fam in WGRAD_CASES:
        assert wgrad_family(ops, case, dtype) == fam, (case, wgrad_family(ops, case, dtype))
    for case, sps in WGRAD_STAGES_PER_SPLIT.items():
        nf, h, w, c0, c1, cout, k = case
        assert ops.wgrad_split(nf * h * w, c0 + c1, cout, k)[0] == sps
    nf, h, w, _, _, cout, _ = RING_WRAP
    assert RING_WRAP in [row[0] for row in FWD_CASES] and ops.stripe_stages(nf * h * w, h, w, cout) == 5
    assert set(FRAME_FORMS.values()) == {(32, 4, False), (64, 4, False), (64, 8, True), (128, 8, False)}
    named = {f for _, _, f, _ in FWD_CASES} | {f for _, _, _, f in FWD_CASES} | {f for _, _, f in WGRAD_CASES}
    for fam in ("conv_fwd_stripe_kernel<32>", "conv_fwd_stripe_kernel<64>", "conv_fwd_stripe_kernel<128>",
                "conv_fwd_frame_kernel<8>", "conv_fwd_frame_kernel<16>", "conv1x1_stream_kernel<64,2>",
                "conv_fwd_glds_kernel", "conv_fwd_kernel<bf16", "conv_fwd_kernel<float", "xe_fwd_kernel",
                "conv_wgrad_win_kernel<8>", "conv_wgrad_win_kernel<16>", "conv_wgrad_win_kernel<32>",
                "conv_wgrad_win_kernel<64>", "conv_wgrad_1x1_kernel", "conv_wgrad_glds_kernel<64,128>",
                "conv_wgrad_glds_kernel<64,256>", "conv_wgrad_glds_kernel<128,128>", "conv_wgrad_kernel<float>"):
        assert fam in named, fam


# ---------------------------------------------------------------------------
# a. forward and dgrad
# ---------------------------------------------------------------------------
RING_WRAP = (2, 40, 128, 64, 0, 896, 3)  # the one large case: with bias and residual only
FWD_PARAMS = [pytest.param(*row, full, id="-".join([_id(row[0]), _id(row[1]), "bias_res" if full else "plain"]))
              for row in FWD_CASES for full in (True, False) if full or row[0] != RING_WRAP]


@gpu
@pytest.mark.parametrize("case,dtype,fam_f,fam_d,full", FWD_PARAMS)
def test_conv_fwd_dgrad_exact(case, dtype, fam_f, fam_d, full):
    from dalle2_video import ops

    nf, h, w, c0, c1, cout, k = case
    check_fwd_routing(ops, case, dtype, fam_f, fam_d, full)
    p = fwd_problem(case, dtype, full)
    print(f"{case} {dname(dtype)}: max |y| {p.y.abs().max().item():.0f}, rounding {p.y_rounds:.3f} of y, "
          f"{p.dx_rounds:.3f} of dx")
    dev = "cuda"
    xd = p.x.to(dev, dtype)
    x0 = (xd[..., :c0].contiguous() if c1 else xd).requires_grad_()
    x1 = xd[..., c0:].contiguous().requires_grad_() if c1 else None
    wd = p.wt.to(dev, F32)
    bd = p.bias.to(dev, F32) if full else None
    rd = p.res.to(dev, dtype) if full else None
    y = ops.conv(x0, wd, bd, x1=x1, res=rd)
    assert y.dtype == dtype
    assert_bits_equal(y, expected_forward(p, case, dtype, fam_f), f"forward {case} [{fam_f}] (frame, row, col, channel)")
    y.backward(p.dy.to(dev, dtype))
    dx = torch.cat([x0.grad] + ([x1.grad] if c1 else []), dim=-1)
    assert dx.dtype == dtype
    assert_bits_equal(dx, rne(p.dx, dtype), f"dgrad {case} [{fam_d}] (frame, row, col, channel)")


# ---------------------------------------------------------------------------
# b. weight and bias gradient
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case,dtype,fam", WGRAD_CASES, ids=_id)
def test_conv_wgrad_exact(case, dtype, fam):
    from dalle2_video import ops

    nf, h, w, c0, c1, cout, k = case
    cin = c0 + c1
    assert wgrad_family(ops, case, dtype) == fam
    if case in WGRAD_STAGES_PER_SPLIT:
        assert ops.wgrad_split(nf * h * w, cin, cout, k)[0] == WGRAD_STAGES_PER_SPLIT[case]
    p = wgrad_problem(case)
    print(f"{case} {dname(dtype)}: dW max {p.dw.max().item():.0f} mean {p.dw.mean().item():.1f}, "
          f"db max {p.db.max().item():.0f}")
    dev = "cuda"
    xd = p.x.to(dev, dtype)
    x0 = xd[..., :c0].contiguous() if c1 else xd
    x1 = xd[..., c0:].contiguous() if c1 else None
    dyd = p.dy.to(dev, dtype)
    wd = torch.zeros(cout, cin, 1, k, k, device=dev).requires_grad_()
    bd = torch.zeros(cout, device=dev).requires_grad_()
    what = f"{case} [{fam}] (cout, cin, 1, ky, kx)"

    def backward():
        ops.conv(x0, wd, bd, x1=x1).backward(dyd)

    # twice into the same leaves without zeroing: the second run accumulates
    for n in (1, 2):
        backward()
        assert_bits_equal(wd.grad, (n * p.dw).float(), f"dW, run {n} {what}")
        assert_bits_equal(bd.grad, (n * p.db).float(), f"db, run {n} {what}")
    # the deferred split-K sums (the trainer's path): partials parked in the arena,
    # one batched sum when the context ends -- overwriting, then accumulating
    wd.grad = bd.grad = None
    for n in (1, 2):
        with ops.defer_wgrad():
            backward()
        assert_bits_equal(wd.grad, (n * p.dw).float(), f"dW, deferred run {n} {what}")
        assert_bits_equal(bd.grad, (n * p.db).float(), f"db, deferred run {n} {what}")


# ---------------------------------------------------------------------------
# CPU self-check: the bit comparison sees what the relative-L2 metric does not
# ---------------------------------------------------------------------------
def test_bit_comparison_sees_what_the_norm_misses():
    """On the float64 reference of the (2, 4, 64, 64 -> 64) case alone: one tap
    dropped at one corner pixel, one output channel of one frame off by 1, and
    truncation in place of round-to-nearest-even each pass test_conv_gpu.rel()
    at its bf16 tolerance of 1.5e-2 -- and each is a mismatch here."""
    from test_conv_gpu import rel

    case = (2, 4, 64, 64, 0, 64, 3)
    p = fwd_problem(case, BF16, True)
    want = rne(p.y, BF16)
    assert mismatches(want, want.clone())[0] == 0

    tap = p.y.clone()  # pixel (0, 0) of frame 0 without its tap (+1, +1): x[0, 1, 1] . w[:, :, 2, 2]
    tap[0, 0, 0] -= p.wt[:, :, 0, 2, 2] @ p.x[0, 1, 1]
    chan = p.y.clone()  # channel 5 of frame 1 one too high
    chan[1, :, :, 5] += 1
    f32 = (p.y + 0.0).float()
    trunc = (f32.view(torch.int32) & -65536).view(torch.float32).bfloat16()  # toward zero (sign-magnitude)
    for name, got in (("dropped tap", rne(tap, BF16)), ("channel + 1", rne(chan, BF16)), ("truncation", trunc)):
        n, first = mismatches(got, want)
        err = rel(got.float(), p.y)
        print(f"{name}: {n} elements differ, rel {err:.2e}")
        assert n > 0, name
        assert err < 1.5e-2, (name, err)
        with pytest.raises(AssertionError, match="elements differ"):
            assert_bits_equal(got, want, name)
    # the one-pixel error stays in its pixel, the channel error in its frame and channel
    assert mismatches(rne(tap, BF16), want)[0] <= 64
    assert all(i[0] == 1 and i[3] == 5 for i in mismatches(rne(chan, BF16), want)[1])
