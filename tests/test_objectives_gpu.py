"""x0 / v prediction objectives and dynamic thresholding on the GPU: the fused
loss (ops.diffusion_loss_cl), the two update kernels with an objective and a
per-sample threshold (ops.p_sample_step / ops.ddim_step), the quantile kernel
(ops.dynamic_threshold_scale), one decoder step, the sampling loops, the
cascade dispatch and training.

Expected values: the float64 restatements of tests/test_objectives_host.py,
evaluated on the CPU on the f32 schedule tables.  The DDPM update gathers the
scheduler's tables (sqrt_alphas_cumprod, ...), so its restatement reads those;
the DDIM update derives every coefficient from alphas_cumprod on the device,
so its restatement does as tests/test_ddim_gpu.py's does.

Tolerances (norm-wise relative error per sample unless stated), the scheme of
tests/test_ddim_gpu.py:
  loss, loss gradient (f32), update out / x0   <= max(1e-6, 4 * e32), e32 = the
                                   error of the same restatement evaluated in f32
  loss gradient (bf16)             the float64 gradient rounded to bf16, 1 ulp
  quantile s                       <= 1e-6 relative, vs torch.quantile in float64
                                   on the same f32 values
  decoder step vs oracle Unet3D    <= 1e-4: the bar of
                                   test_ddim_gpu.test_decoder_ddim_step_vs_oracle_unet
                                   and test_sample_gpu.test_decoder_p_sample_vs_oracle
  loops, graph replay vs eager     torch.equal with an elementwise denoiser;
                                   < 1e-5 with Unet3D: the bar of
                                   test_ddim_gpu.test_ddim_loop_graph_replay_matches_eager
  training loss / to_out gradient  1e-4 / 1e-3: the f32 bars of
                                   test_unet_gpu.test_p_losses_forward_backward_vs_oracle
  trainer, replayed vs eager loss  <= 1e-5, flat gradient <= 1e-5: the f32 bars of
                                   test_cfg2_trainer_gpu.test_cfg2_trainer_graph_replay_vs_eager_vs_oracle
The observed values are printed and appended to $DV_PARITY_LOG.
"""
import functools
import math

import pytest
import torch

import test_ddim_gpu as TD
import test_objectives_host as H
from oracle import dv_ref as R

pytestmark = pytest.mark.gpu

bc = H.bc
rel = TD.rel
rel_per_sample = TD.rel_per_sample
_sched = TD._sched


def _tol(e32):
    # a non-finite f32 restatement allows nothing extra
    return [max(1e-6, 4 * e) if math.isfinite(e) else 1e-6 for e in e32]


def _tab(table, t, dtype):
    return bc(table.cpu().to(dtype)[t.cpu()])


def x0_from(x, pred, a_or_sched, t, objective, dtype, ddim):
    """Unthresholded x0 of the objective.  ddim: the factors come from
    alphas_cumprod; otherwise from the scheduler's gathered tables."""
    s = a_or_sched
    if objective == "x0":
        return pred
    if ddim:
        a = _tab(s.alphas_cumprod, t, dtype)
        if objective == "v":
            return H.predict_start_from_v(x, pred, a.sqrt(), (1 - a).sqrt())
        return H.predict_start_from_noise(x, pred, (1 / a).sqrt(), (1 / a - 1).sqrt())
    if objective == "v":
        return H.predict_start_from_v(x, pred, _tab(s.sqrt_alphas_cumprod, t, dtype),
                                      _tab(s.sqrt_one_minus_alphas_cumprod, t, dtype))
    return H.predict_start_from_noise(x, pred, _tab(s.sqrt_recip_alphas_cumprod, t, dtype),
                                      _tab(s.sqrt_recipm1_alphas_cumprod, t, dtype))


def ddpm_restatement(x, pred, z, t, s, objective, clip, dyn_p, dtype):
    """(x_prev, x0) of p_mean_variance + p_sample (:1585-1664), every operation in `dtype`."""
    x, pred, z = x.cpu().to(dtype), pred.cpu().to(dtype), z.cpu().to(dtype)
    x0 = x0_from(x, pred, s, t, objective, dtype, ddim=False)
    if clip:
        x0 = H.dynamic_threshold(x0, dyn_p)
    mean = _tab(s.posterior_mean_coef1, t, dtype) * x0 + _tab(s.posterior_mean_coef2, t, dtype) * x
    nz = bc((t.cpu() != 0).to(dtype))
    return mean + nz * (0.5 * _tab(s.posterior_log_variance_clipped, t, dtype)).exp() * z, x0


def ddim_restatement(x, pred, z, t, tn, s, eta, objective, clip, dyn_p, dtype):
    """(x_next, x0) of one step of the DDIM loop (:1843-1876), every operation in `dtype`."""
    x, pred, z = x.cpu().to(dtype), pred.cpu().to(dtype), z.cpu().to(dtype)
    a, a_next = _tab(s.alphas_cumprod, t, dtype), _tab(s.alphas_cumprod, tn, dtype)
    x0 = x0_from(x, pred, s, t, objective, dtype, ddim=True)
    if clip:
        x0 = H.dynamic_threshold(x0, dyn_p)
    pred_noise = H.predict_noise_from_start(x, x0, (1 / a).sqrt(), (1 / a - 1).sqrt())
    c1 = eta * ((1 - a / a_next) * (1 - a_next) / (1 - a)).sqrt()
    c2 = ((1 - a_next) - c1 ** 2).sqrt()
    z = torch.where(bc(tn.cpu() == 0), torch.zeros_like(z), z)
    return x0 * a_next.sqrt() + c1 * z + c2 * pred_noise, x0


def _check(parity_log, got_pair, want_pair, f32_pair, **tags):
    for name, got, want, f32 in zip(("out", "x0"), got_pair, want_pair, f32_pair):
        e32 = rel_per_sample(f32, want)
        err = rel_per_sample(got, want)
        tol = _tol(e32)
        parity_log(what=name, rel=err, e32=e32, tol=tol, **tags)
        assert all(e <= b for e, b in zip(err, tol)), (name, err, tol)


def _pred_forms(pred, form):
    """(device tensor in `form`, the CPU values it holds)."""
    from dalle2_video import ops

    if form == "ncthw":
        return pred.cuda(), pred
    if form == "cl_f32":
        return ops.to_cl(pred.cuda(), torch.float32), pred
    return ops.to_cl(pred.cuda(), torch.bfloat16), pred.bfloat16().float()


# ---------------------------------------------------------------------------
# loss kernel
# ---------------------------------------------------------------------------
LOSS_SHAPE = (3, 3, 2, 5, 7)  # odd pixel count, channel pad 3 -> 8


@functools.lru_cache(maxsize=None)
def _loss_inputs():
    g = torch.Generator().manual_seed(11)
    x_start = torch.rand(LOSS_SHAPE, generator=g)
    noise = torch.randn(LOSS_SHAPE, generator=g)
    pred = torch.randn(LOSS_SHAPE, generator=g)
    return x_start, noise, pred, torch.tensor([0, 537, 999]), torch.tensor([0.5, 1.25, 2.0])


def loss_restatement(pred, x_start, noise, t, s, objective, w, dtype):
    """p_losses :1988-2002 on a given prediction: (loss, d loss / d pred)."""
    pred = pred.to(dtype).clone().requires_grad_(True)
    xs = x_start.to(dtype) * 2 - 1
    nz = noise.to(dtype)
    if objective == "v":
        target = H.calculate_v(xs, nz, _tab(s.sqrt_alphas_cumprod, t, dtype),
                               _tab(s.sqrt_one_minus_alphas_cumprod, t, dtype))
    else:
        target = xs if objective == "x0" else nz
    per = ((pred - target) ** 2).flatten(1).mean(dim=1)
    if w is not None:
        per = per * w.to(dtype)
    loss = per.mean()
    loss.backward()
    return loss.detach(), pred.grad


def _cl_of(v):
    B, C, T, Hh, W = v.shape
    return v.permute(0, 2, 3, 4, 1).reshape(B * T, Hh, W, C)


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("objective", ["eps", "x0", "v"])
def test_diffusion_loss_vs_float64_autograd(parity_log, objective, dtype, weights):
    from dalle2_video import ops

    s = _sched("cosine")
    x_start, noise, pred, t, w = _loss_inputs()
    w = w if weights else None
    pred_cl = ops.to_cl(pred.cuda(), dtype).requires_grad_(True)
    held = pred if dtype == torch.float32 else pred.bfloat16().float()
    loss = ops.diffusion_loss_cl(pred_cl, x_start.cuda(), noise.cuda(), t.cuda(), s, objective, normalize=True,
                                 sample_w=None if w is None else w.cuda())
    loss.backward()
    l64, g64 = loss_restatement(held, x_start, noise, t, s, objective, w, torch.float64)
    l32, g32 = loss_restatement(held, x_start, noise, t, s, objective, w, torch.float32)
    e32 = abs(l32.item() - l64.item()) / abs(l64.item())
    err = abs(loss.item() - l64.item()) / abs(l64.item())
    parity_log(objective=objective, dtype=str(dtype), weights=weights, loss_rel=err, loss_e32=e32)
    assert err <= max(1e-6, 4 * e32)
    got = pred_cl.grad[..., :3].float().cpu()
    assert (pred_cl.grad[..., 3:] == 0).all()
    want = _cl_of(g64)
    if dtype == torch.float32:
        n = got.shape[0] // 3  # frames per sample
        ge32 = [rel(_cl_of(g32)[i * n:(i + 1) * n], want[i * n:(i + 1) * n]) for i in range(3)]
        gerr = [rel(got[i * n:(i + 1) * n], want[i * n:(i + 1) * n]) for i in range(3)]
        parity_log(objective=objective, weights=weights, grad_rel=gerr, grad_e32=ge32)
        assert all(e <= b for e, b in zip(gerr, _tol(ge32))), (gerr, ge32)
    else:
        wb = want.float().bfloat16().float()
        ulp = torch.ldexp(torch.ones_like(wb), torch.frexp(wb).exponent - 8)  # bf16 spacing at wb
        worst = ((got - wb).abs() / ulp).max().item()
        parity_log(objective=objective, weights=weights, grad_bf16_ulps=worst)
        assert worst <= 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_eps_loss_is_the_mse_kernel(dtype):
    from dalle2_video import ops

    s = _sched("cosine")
    x_start, noise, pred, t, w = _loss_inputs()
    outs = []
    for fn in (lambda p: ops.diffusion_loss_cl(p, x_start.cuda(), noise.cuda(), t.cuda(), s, "eps", sample_w=w.cuda()),
               lambda p: ops.mse_loss_cl(p, noise.cuda(), w.cuda())):
        p = ops.to_cl(pred.cuda(), dtype).requires_grad_(True)
        loss = fn(p)
        loss.backward()
        outs.append((loss.detach(), p.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_loss_out_of_schedule_timestep_is_nan():
    from dalle2_video import ops

    s = _sched("cosine")
    x_start, noise, pred, t, _ = _loss_inputs()
    for objective in ("x0", "v"):
        p = ops.to_cl(pred.cuda(), torch.float32).requires_grad_(True)
        loss = ops.diffusion_loss_cl(p, x_start.cuda(), noise.cuda(), torch.tensor([0, 1000, 5]).cuda(), s, objective)
        loss.backward()
        assert torch.isnan(loss)
        n = p.shape[0] // 3
        assert torch.isnan(p.grad[n:2 * n, ..., :3]).all() and torch.isfinite(p.grad[:n]).all()


# ---------------------------------------------------------------------------
# update kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["ncthw", "cl_f32", "cl_bf16"])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("kind", ["cosine", "linear"])
@pytest.mark.parametrize("objective", ["x0", "v"])
def test_ddim_step_objectives_vs_float64_restatement(parity_log, objective, kind, eta, clip, form):
    """The pairs 1 -> 0, 3 -> 1, 537 -> 500, 999 -> 958 in one batch."""
    from dalle2_video import ops

    s = _sched(kind)
    x, pred, z, t, tn = TD._kernel_inputs()
    pred_dev, pred = _pred_forms(pred, form)
    noise = z.cuda() if eta != 0 else None
    got = ops.ddim_step(x.cuda(), pred_dev, noise, t.cuda(), tn.cuda(), s, eta, clip_denoised=clip,
                        objective=objective)
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    want = ddim_restatement(x, pred, z, t, tn, s, eta, objective, clip, None, torch.float64)
    f32 = ddim_restatement(x, pred, z, t, tn, s, eta, objective, clip, None, torch.float32)
    _check(parity_log, got, want, f32, kernel="ddim", objective=objective, kind=kind, eta=eta, clip=clip, form=form)
    if eta == 0 and form == "ncthw":
        xin = x.cuda().clone()
        out_ip, _ = ops.ddim_step(xin, pred_dev, None, t.cuda(), tn.cuda(), s, eta, clip_denoised=clip, out=xin,
                                  want_x0=False, objective=objective)
        assert out_ip is xin and torch.equal(xin, got[0])


@pytest.mark.parametrize("form", ["ncthw", "cl_f32", "cl_bf16"])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("kind", ["cosine", "linear"])
@pytest.mark.parametrize("objective", ["x0", "v"])
def test_p_sample_step_objectives_vs_float64_restatement(parity_log, objective, kind, clip, form):
    """t = 1, 3, 537, 999 in one batch (the DDPM update takes no eta)."""
    from dalle2_video import ops

    s = _sched(kind)
    x, pred, z, t, _ = TD._kernel_inputs()
    pred_dev, pred = _pred_forms(pred, form)
    got = ops.p_sample_step(x.cuda(), pred_dev, z.cuda(), t.cuda(), s, clip_denoised=clip, objective=objective)
    assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all()
    want = ddpm_restatement(x, pred, z, t, s, objective, clip, None, torch.float64)
    f32 = ddpm_restatement(x, pred, z, t, s, objective, clip, None, torch.float32)
    _check(parity_log, got, want, f32, kernel="ddpm", objective=objective, kind=kind, clip=clip, form=form)
    if form == "ncthw":
        xin = x.cuda().clone()
        out_ip, _ = ops.p_sample_step(xin, pred_dev, z.cuda(), t.cuda(), s, clip_denoised=clip, out=xin,
                                      want_x0=False, objective=objective)
        assert out_ip is xin and torch.equal(xin, got[0])


@pytest.mark.parametrize("form", ["ncthw", "cl_bf16"])
def test_default_objective_is_explicit_eps(form):
    from dalle2_video import ops

    s = _sched("cosine")
    x, pred, z, t, tn = TD._kernel_inputs()
    pred_dev, _ = _pred_forms(pred, form)
    a = ops.p_sample_step(x.cuda(), pred_dev, z.cuda(), t.cuda(), s)
    b = ops.p_sample_step(x.cuda(), pred_dev, z.cuda(), t.cuda(), s, objective="eps", dyn_scale=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a = ops.ddim_step(x.cuda(), pred_dev, z.cuda(), t.cuda(), tn.cuda(), s, 1.0)
    b = ops.ddim_step(x.cuda(), pred_dev, z.cuda(), t.cuda(), tn.cuda(), s, 1.0, objective="eps", dyn_scale=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------
# quantile kernel
# ---------------------------------------------------------------------------
QUANT_SHAPES = {45: (3, 3, 1, 3, 5), 384: (3, 3, 2, 8, 8), 12288: (3, 3, 4, 32, 32)}


def _quantile64(v, p):
    return torch.quantile(v.flatten(1).abs().double(), p, dim=-1).clamp(min=1.0)


@pytest.mark.parametrize("p", [0.5, 0.95, 1.0])
@pytest.mark.parametrize("n", [45, 384, 12288])
@pytest.mark.parametrize("data", ["normal", "ties"])
def test_quantile_vs_torch_quantile(parity_log, data, n, p):
    """objective x0: x0_u is the prediction itself, so the kernel's input
    values are exactly the f32 values torch.quantile gets.  `ties`: 16 levels."""
    from dalle2_video import ops

    s = _sched("cosine")
    shape = QUANT_SHAPES[n]
    assert shape[1] * shape[2] * shape[3] * shape[4] == n
    g = torch.Generator().manual_seed(n)
    if data == "ties":
        pred = torch.randint(0, 16, shape, generator=g).float() * 0.5 - 3.75
    else:
        pred = torch.randn(shape, generator=g) * torch.tensor([0.5, 2.0, 3.0]).reshape(3, 1, 1, 1, 1)
    x = torch.randn(shape, generator=g)
    t = torch.tensor([3, 537, 999])
    want = _quantile64(pred, p)
    for form in ("ncthw", "cl_f32", "cl_bf16"):
        pred_dev, held = _pred_forms(pred, form)
        want = _quantile64(held, p)
        for ddim in (False, True):
            got = ops.dynamic_threshold_scale(x.cuda(), pred_dev, t.cuda(), s, "x0", p, ddim=ddim)
            err = ((got.double().cpu() - want).abs() / want).max().item()
            parity_log(data=data, n=n, p=p, form=form, ddim=ddim, s=got.tolist(), rel=err)
            assert err <= 1e-6
    if p == 1.0:
        assert torch.equal(got.cpu(), held.flatten(1).abs().max(dim=1).values.clamp(min=1.0))


@pytest.mark.parametrize("objective", ["eps", "v"])
@pytest.mark.parametrize("ddim", [False, True])
def test_quantile_recomputes_x0_from_the_objective(parity_log, objective, ddim):
    """x0_u derived in the kernel (N = 384): the float64 x0_u of the
    restatement, rounded to f32, goes to torch.quantile.  The kernel's f32 x0_u
    is within a few ulp of that, and an order statistic moves by no more than
    the largest change of an element, so the 1e-6 bar on s >= 1 holds."""
    from dalle2_video import ops

    s = _sched("cosine")
    g = torch.Generator().manual_seed(5)
    shape = QUANT_SHAPES[384]
    x = torch.randn(shape, generator=g) * 2
    pred = torch.randn(shape, generator=g) * 2
    t = torch.tensor([3, 537, 999])
    x0u = x0_from(x.double(), pred.double(), s, t, objective, torch.float64, ddim)
    want = _quantile64(x0u.float(), 0.95)
    got = ops.dynamic_threshold_scale(x.cuda(), pred.cuda(), t.cuda(), s, objective, 0.95, ddim=ddim)
    err = ((got.double().cpu() - want).abs() / want).max().item()
    parity_log(objective=objective, ddim=ddim, s=got.tolist(), rel=err)
    assert err <= 1e-6


@functools.lru_cache(maxsize=None)
def _mixed_batch():
    """Sample 0 small (quantile < 1), samples 1 and 2 large (quantile > 1)."""
    g = torch.Generator().manual_seed(23)
    shape = (3, 3, 2, 8, 8)
    scale = torch.tensor([0.2, 3.0, 4.0]).reshape(3, 1, 1, 1, 1)
    x = torch.randn(shape, generator=g) * scale
    pred = torch.randn(shape, generator=g) * scale
    z = torch.randn(shape, generator=g)
    return x, pred, z, torch.tensor([300, 537, 800]), torch.tensor([250, 500, 700])


@pytest.mark.parametrize("kernel", ["ddpm", "ddim"])
@pytest.mark.parametrize("objective", ["eps", "x0", "v"])
def test_dynamic_threshold_in_the_updates(parity_log, objective, kernel):
    from dalle2_video import ops

    s = _sched("cosine")
    x, pred, z, t, tn = _mixed_batch()
    ddim, p = kernel == "ddim", 0.95
    q = torch.quantile(x0_from(x.double(), pred.double(), s, t, objective, torch.float64, ddim).flatten(1).abs(),
                       p, dim=-1)
    assert q[0] < 1 and q[1] > 1 and q[2] > 1, q  # the premise, on the CPU
    dev = lambda v: v.cuda()
    sc = ops.dynamic_threshold_scale(dev(x), dev(pred), dev(t), s, objective, p, ddim=ddim)
    assert sc[0] == 1.0 and (sc[1:] > 1).all()
    if ddim:
        run = lambda ds: ops.ddim_step(dev(x), dev(pred), dev(z), dev(t), dev(tn), s, 1.0, objective=objective,
                                       dyn_scale=ds)
        want = ddim_restatement(x, pred, z, t, tn, s, 1.0, objective, True, p, torch.float64)
        f32 = ddim_restatement(x, pred, z, t, tn, s, 1.0, objective, True, p, torch.float32)
    else:
        run = lambda ds: ops.p_sample_step(dev(x), dev(pred), dev(z), dev(t), s, objective=objective, dyn_scale=ds)
        want = ddpm_restatement(x, pred, z, t, s, objective, True, p, torch.float64)
        f32 = ddpm_restatement(x, pred, z, t, s, objective, True, p, torch.float32)
    dyn, static = run(sc), run(None)
    # s = 1: bit-equal to the static clamp.  (For eps the static clamp is the
    # kernel instantiation that predates the objectives, kept as it was compiled;
    # the compiler contracts its multiply-adds differently, so that pair is held
    # to the rounding of f32 arithmetic, 1e-6, instead.)
    if objective == "eps":
        assert rel(dyn[0][0], static[0][0]) <= 1e-6 and rel(dyn[1][0], static[1][0]) <= 1e-6
    else:
        assert torch.equal(dyn[0][0], static[0][0]) and torch.equal(dyn[1][0], static[1][0])
    assert dyn[1][1:].abs().max() <= 1 and torch.isfinite(dyn[0]).all()
    assert not torch.equal(dyn[1][1:], static[1][1:])
    _check(parity_log, dyn, want, f32, kernel=kernel, objective=objective, dynamic=True)


@pytest.mark.parametrize("kernel", ["ddpm", "ddim"])
def test_out_of_schedule_sample_is_nan_and_neighbours_are_untouched(kernel):
    from dalle2_video import ops

    s = _sched("cosine")
    x, pred, z, t, tn = _mixed_batch()
    ddim = kernel == "ddim"
    bad_t = torch.tensor([300, 1000, 800])
    dev = lambda v: v.cuda()

    def run(tt):
        sc = ops.dynamic_threshold_scale(dev(x), dev(pred), dev(tt), s, "v", 0.95, ddim=ddim)
        if ddim:
            return sc, ops.ddim_step(dev(x), dev(pred), dev(z), dev(tt), dev(tn), s, 1.0, objective="v", dyn_scale=sc)
        return sc, ops.p_sample_step(dev(x), dev(pred), dev(z), dev(tt), s, objective="v", dyn_scale=sc)

    (sc_b, (out_b, x0_b)), (sc_g, (out_g, x0_g)) = run(bad_t), run(t)
    assert torch.isnan(sc_b[1]) and torch.isnan(out_b[1]).all() and torch.isnan(x0_b[1]).all()
    for i in (0, 2):
        assert sc_b[i] == sc_g[i] and torch.equal(out_b[i], out_g[i]) and torch.equal(x0_b[i], x0_g[i])
    # a non-finite x0_u inside the schedule poisons its sample only
    xi = x.clone()
    xi[2, 1, 0, 3, 3] = float("inf")
    sc = ops.dynamic_threshold_scale(dev(xi), dev(pred), dev(t), s, "v", 0.95, ddim=ddim)
    assert torch.isnan(sc[2]) and sc[0] == sc_g[0] and sc[1] == sc_g[1]


def test_dyn_scale_needs_clip():
    from dalle2_video import _lib, ops

    s = _sched("cosine")
    x, pred, z, t, tn = _mixed_batch()
    sc = torch.ones(3, device="cuda")
    with pytest.raises(_lib.DVError, match="clip"):
        ops.p_sample_step(x.cuda(), pred.cuda(), z.cuda(), t.cuda(), s, clip_denoised=False, dyn_scale=sc)
    with pytest.raises(_lib.DVError, match="objective"):
        ops.p_sample_step(x.cuda(), pred.cuda(), z.cuda(), t.cuda(), s, objective="x_start")


_X = "(3, 3, 2, 8, 8)"  # _mixed_batch's clip: 6 frames of 8 x 8 x 3
_OUT = "p_sample: out must be a contiguous f32 tensor shaped like x"
_MALFORMED = {  # case: (objective, the argument that is wrong, the whole message)
    "eps_out_dtype": ("eps", dict(out=lambda: torch.empty(3, 3, 2, 8, 8, dtype=torch.bfloat16)), _OUT),
    "eps_out_shape": ("eps", dict(out=lambda: torch.empty(3, 3, 2, 8, 4)), _OUT),
    "v_out_dtype": ("v", dict(out=lambda: torch.empty(3, 3, 2, 8, 8, dtype=torch.bfloat16)), _OUT),
    "v_out_shape": ("v", dict(out=lambda: torch.empty(3, 3, 2, 8, 4)), _OUT),
    # the eps entry names the channels-last prediction "eps", the objective entry "pred"
    "eps_cl_frames": ("eps", dict(eps=lambda: torch.zeros(5, 8, 8, 3)),
                      f"p_sample: eps (5, 8, 8, 3) does not match x {_X}"),
    "eps_cl_channels": ("eps", dict(eps=lambda: torch.zeros(6, 8, 8, 2)),
                        f"p_sample: eps (6, 8, 8, 2) does not match x {_X}"),
    "v_cl_frames": ("v", dict(eps=lambda: torch.zeros(5, 8, 8, 3)),
                    f"p_sample: pred (5, 8, 8, 3) does not match x {_X}"),
    "v_cl_channels": ("v", dict(eps=lambda: torch.zeros(6, 8, 8, 2)),
                      f"p_sample: pred (6, 8, 8, 2) does not match x {_X}"),
    "v_cl_hw": ("v", dict(eps=lambda: torch.zeros(6, 4, 16, 3)),
                f"p_sample: pred (6, 4, 16, 3) does not match x {_X}"),
    "v_ncthw_shape": ("v", dict(eps=lambda: torch.zeros(3, 3, 2, 4, 16)),
                      f"p_sample: pred (3, 3, 2, 4, 16) does not match x {_X}"),
    "eps_dyn_scale_length": ("eps", dict(dyn_scale=lambda: torch.ones(2)),
                             "p_sample: dyn_scale holds one contiguous f32 value per sample"),
    "v_dyn_scale_length": ("v", dict(dyn_scale=lambda: torch.ones(2)),
                           "p_sample: dyn_scale holds one contiguous f32 value per sample"),
}


@pytest.mark.parametrize("case", sorted(_MALFORMED))
def test_p_sample_step_rejects_malformed_inputs(case):
    """Each entry of ops.p_sample_step (dv_p_sample for a plain eps step,
    dv_p_sample_obj otherwise) refuses a malformed argument before any launch,
    with the message it has always had."""
    from dalle2_video import _lib, ops

    objective, wrong, message = _MALFORMED[case]
    x, pred, z, t, _ = _mixed_batch()
    kw = dict(eps=pred.cuda(), objective=objective)
    kw.update({k: make().cuda() for k, make in wrong.items()})
    with pytest.raises(_lib.DVError) as e:
        ops.p_sample_step(x.cuda(), kw.pop("eps"), z.cuda(), t.cuda(), _sched("cosine"), **kw)
    assert str(e.value) == message


# ---------------------------------------------------------------------------
# decoder step vs the oracle Unet3D
# ---------------------------------------------------------------------------
def _mk_unet(mod, dim=64):
    return mod.Unet3D(dim, video_embed_dim=512, channels=3, dim_mults=(1, 2, 4, 8)).cast_model_parameters(
        lowres_cond=False, lowres_noise_cond=False, channels=3, channels_out=3, cond_on_image_embeds=True,
        cond_on_text_encodings=False)


@functools.lru_cache(maxsize=None)
def _decoder_step_case():
    """The Unet3D and shape of test_ddim_gpu's decoder step (1x3x8x32x32, f32);
    one oracle forward shared by every case below."""
    from dalle2_video import dalle2_video as D

    ou = R.deterministic_fill_(_mk_unet(R))
    dec = D.VideoDecoder(_mk_unet(D), frame_sizes=(32,), frame_numbers=(8,), timesteps=1000, learned_variance=False,
                         predict_v=True, dynamic_thres_percentile=0.9)
    dec.unets[0].load_state_dict(ou.state_dict(), strict=True)
    g = torch.Generator().manual_seed(43)
    x = torch.randn(1, 3, 8, 32, 32, generator=g)
    z = torch.randn(x.shape, generator=g)
    t, tn = torch.tensor([537]), torch.tensor([500])
    with torch.no_grad():
        pred = ou.forward_with_cond_scale(x, t, video_embed=None, lowres_cond_video=None, cond_scale=1.0)
    return dec.cuda(), x, z, t, tn, pred


@pytest.mark.parametrize("dynamic", [False, True])
@pytest.mark.parametrize("kernel", ["ddpm", "ddim"])
def test_decoder_step_v_objective_vs_oracle_unet(parity_log, kernel, dynamic):
    dec, x, z, t, tn, pred = _decoder_step_case()
    dec.use_dynamic_thres = dynamic
    sched = dec.noise_schedulers[0]
    p = dec.dynamic_thres_percentile if dynamic else None
    if dynamic:  # the threshold is active: the check is not vacuous
        x0u = x0_from(x.double(), pred.double(), sched, t, "v", torch.float64, kernel == "ddim")
        assert torch.quantile(x0u.flatten(1).abs(), p, dim=-1)[0] > 1
    if kernel == "ddim":
        want = ddim_restatement(x, pred, z, t, tn, sched, 1.0, "v", True, p, torch.float64)
        got = dec.p_sample_ddim(dec.unets[0], x.cuda(), t.cuda(), tn.cuda(), video_embed=None, noise_scheduler=sched,
                                eta=1.0, clip_denoised=True, noise=z.cuda(), predict_v=True)
    else:
        want = ddpm_restatement(x, pred, z, t, sched, "v", True, p, torch.float64)
        got = dec.p_sample(dec.unets[0], x.cuda(), t.cuda(), video_embed=None, noise_scheduler=sched,
                           clip_denoised=True, noise=z.cuda(), predict_v=True)
    dec.use_dynamic_thres = False
    e_out, e_x0 = rel(got[0], want[0]), rel(got[1], want[1])
    parity_log(kernel=kernel, dynamic=dynamic, out_rel=e_out, x0_rel=e_x0)
    assert e_out <= 1e-4 and e_x0 <= 1e-4


# ---------------------------------------------------------------------------
# sampling loops
# ---------------------------------------------------------------------------
def _loop_decoder(ddim):
    from dalle2_video import dalle2_video as D
    from dalle2_video.utils import deterministic_fill_

    u = D.Unet3D(16, video_embed_dim=512, channels=3, dim_mults=(1, 2, 4, 8))
    kw = dict(timesteps=20, sample_timesteps=6, ddim_sampling_eta=0.0) if ddim else dict(timesteps=12)
    dec = D.VideoDecoder(u, frame_sizes=(32,), frame_numbers=(4,), learned_variance=False, predict_v=True,
                         use_dynamic_thres=True, dynamic_thres_percentile=0.9, **kw)
    deterministic_fill_(dec.unets[0])
    return dec.cuda().eval()


@pytest.mark.parametrize("ddim", [False, True])
def test_loop_v_dynamic_graph_replay_is_bit_equal_to_eager(ddim):
    """DDPM (12 steps) and DDIM (six of 20, eta 0) with the reproducible
    elementwise stand-in of test_ddim_gpu as the denoiser (cond_scale = 2: the
    captured step calls forward_with_cond_scale): the captured step — noise
    draw, quantile kernel, update — replays to the bits of the eager loop."""
    dec = _loop_decoder(ddim)
    shape = (2, 3, 4, 32, 32)
    outs = []
    for graphs in (False, True):
        dec.sample_graphs = graphs
        torch.cuda.manual_seed(9)
        kw = dict(video_embed=None, noise_scheduler=dec.noise_schedulers[0], predict_v=True, cond_scale=2.0)
        if ddim:
            outs.append(dec.p_sample_loop_ddim(TD._ElementwiseDenoiser(), shape, timesteps=6, **kw))
        else:
            outs.append(dec.p_sample_loop_ddpm(TD._ElementwiseDenoiser(), shape, **kw))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("ddim", [False, True])
def test_loop_v_dynamic_unet3d_graph_matches_eager(parity_log, ddim):
    dec = _loop_decoder(ddim)
    outs = []
    for graphs in (False, True):
        dec.sample_graphs = graphs
        torch.cuda.manual_seed(77)
        outs.append(dec.sample(video_embed=torch.zeros(2, 512, device="cuda")))
    eager, graph = outs
    assert eager.shape == (2, 3, 4, 32, 32) and torch.isfinite(eager).all() and torch.isfinite(graph).all()
    e = rel(graph, eager)
    parity_log(ddim=ddim, graph_vs_eager_rel=e)
    assert e < 1e-5


def test_cascade_gives_each_unet_its_objective(monkeypatch):
    """predict_v=(False, True), sample_timesteps=(4, None) of 12: the base
    unet's four DDIM updates get "eps", the second unet's twelve DDPM updates
    get "v" (eager loops; the calls are observed at ops)."""
    from dalle2_video import dalle2_video as D
    from dalle2_video import ops

    base = D.Unet3D(8, video_embed_dim=512, channels=3, dim_mults=(1, 2))
    sr = D.Unet3D(8, video_embed_dim=512, channels=3, dim_mults=(1, 2, 4, 8, 16), cond_on_text_encodings=False)
    dec = D.VideoDecoder((base, sr), frame_sizes=(32, 64), frame_numbers=(2, 2), timesteps=12,
                         sample_timesteps=(4, None), beta_schedule=("cosine", "cosine"), predict_v=(False, True),
                         learned_variance=False).cuda()
    dec.sample_graphs = False
    seen = {"ddim": [], "ddpm": []}
    ddim_step, p_sample_step = ops.ddim_step, ops.p_sample_step

    def spy_ddim(*a, objective="eps", **kw):
        seen["ddim"].append(objective)
        return ddim_step(*a, objective=objective, **kw)

    def spy_ddpm(*a, objective="eps", **kw):
        seen["ddpm"].append(objective)
        return p_sample_step(*a, objective=objective, **kw)

    monkeypatch.setattr(ops, "ddim_step", spy_ddim)
    monkeypatch.setattr(ops, "p_sample_step", spy_ddpm)
    torch.cuda.manual_seed(3)
    vid = dec.sample(video_embed=torch.zeros(1, 512, device="cuda"))
    assert vid.shape == (1, 3, 2, 64, 64) and torch.isfinite(vid).all()
    assert seen == {"ddim": ["eps"] * 4, "ddpm": ["v"] * 12}
    # the same cascade through the captured step graphs
    monkeypatch.undo()
    dec.sample_graphs = True
    torch.cuda.manual_seed(3)
    vid_g = dec.sample(video_embed=torch.zeros(1, 512, device="cuda"))
    assert vid_g.shape == (1, 3, 2, 64, 64) and torch.isfinite(vid_g).all()


# ---------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------
def _train_pair(**flags):
    from dalle2_video import dalle2_video as D

    ou = R.deterministic_fill_(_mk_unet(R, 16))
    dec = D.VideoDecoder(_mk_unet(D, 16), frame_sizes=(32,), frame_numbers=(4,), timesteps=1000,
                         learned_variance=False, **flags)
    dec.unets[0].load_state_dict(ou.state_dict(), strict=True)
    return ou, dec.cuda()


@pytest.mark.parametrize("objective", ["v", "x0"])
def test_decoder_training_loss_vs_oracle(parity_log, objective):
    """decoder(video, unet_number=1) on the tiny Unet3D (2x3x4x32x32, f32): the
    decoder draws times and noise from the device generator (regenerated here
    from the seed, as tests/test_cfg2_trainer_gpu.py does); the oracle Unet3D
    runs on the CPU and the target is the restatement's."""
    ou, dec = _train_pair(predict_v=objective == "v", predict_x_start=objective == "x0")
    g = torch.Generator().manual_seed(1234)
    video = torch.rand(2, 3, 4, 32, 32, generator=g).cuda()
    torch.cuda.manual_seed(7)
    loss = dec(video, video_embed=None, unet_number=1)
    loss.backward()
    torch.cuda.manual_seed(7)
    times = torch.randint(0, 1000, (2,), device="cuda", dtype=torch.long).cpu()
    noise = torch.randn_like(video).cpu()
    sched = R.NoiseScheduler(beta_schedule="cosine", timesteps=1000, loss_type="l2")
    xs = video.cpu() * 2 - 1
    pred = ou(sched.q_sample(xs, times, noise), times, video_embed=None, lowres_cond_video=None,
              video_cond_drop_prob=0.0, text_cond_drop_prob=0.0)
    if objective == "v":
        target = H.calculate_v(xs, noise, bc(sched.sqrt_alphas_cumprod[times]),
                               bc(sched.sqrt_one_minus_alphas_cumprod[times]))
    else:
        target = xs
    lo = ((pred - target) ** 2).flatten(1).mean(dim=1).mean()
    lo.backward()
    e_loss = abs(loss.item() - lo.item()) / abs(lo.item())
    e_w = rel(dec.unets[0].to_out.weight.grad, ou.to_out.weight.grad)
    e_b = rel(dec.unets[0].to_out.bias.grad, ou.to_out.bias.grad)
    parity_log(objective=objective, times=times.tolist(), loss=loss.item(), loss_oracle=lo.item(), loss_rel=e_loss,
               to_out_weight_grad_rel=e_w, to_out_bias_grad_rel=e_b)
    assert e_loss < 1e-4
    assert e_w < 1e-3 and e_b < 1e-3


def test_trainer_v_objective_graph_replay_matches_eager(parity_log):
    from dalle2_video.trainer import VideoDecoderTrainer

    _, dec = _train_pair(predict_v=True)
    tr = VideoDecoderTrainer(dec, lr=3e-4, wd=1e-2, use_ema=False, amp=False, use_graphs=True)
    g = torch.Generator().manual_seed(1234)
    video = torch.rand(2, 3, 4, 32, 32, generator=g).cuda()
    torch.cuda.manual_seed(1)
    tr(video=video, unet_number=1)
    tr.update(1)  # builds the flat buffers (the first call is never captured)
    opt = tr.optim0
    res = {}
    # A, B: the two eager warm-up calls; C captures and replays; D replays
    for tag, seed in (("A", 7), ("B", 8), ("C", 7), ("D", 8)):
        opt.zero_grad()
        torch.cuda.manual_seed(seed)
        loss = tr(video=video, unet_number=1)
        torch.cuda.synchronize()
        res[tag] = (loss, opt.flat_grad.clone())
    ent = next(iter(tr._graphs.values()))
    assert len(tr._graphs) == 1 and "graph" in ent, "the training step was not captured"
    errs = {}
    for e, r in (("A", "C"), ("B", "D")):
        errs[f"loss_{e}{r}"] = abs(res[e][0] - res[r][0]) / abs(res[e][0])
        errs[f"grad_{e}{r}"] = rel(res[r][1], res[e][1])
    parity_log(**errs)
    assert all(v <= 1e-5 for v in errs.values()), errs
    # the v loss is not the eps loss: the objective reached the captured step
    _, dec_eps = _train_pair()
    torch.cuda.manual_seed(7)
    l_eps = dec_eps(video, video_embed=None, unet_number=1).item()
    assert abs(l_eps - float(res["C"][0])) / abs(l_eps) > 1e-2
