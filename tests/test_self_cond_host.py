"""Self-conditioning (Unet3D(self_cond=True), Analog Bits, arXiv 2208.04202):
what needs no GPU, and the float64 restatements tests/test_self_cond_gpu.py
evaluates.

The restatements are the reference's arithmetic written out in plain PyTorch
(dalle2_video.py:738-745 the input concat, :1969-1983 the two-pass training
step, :1727 / :1830 the sampling loops carrying x_start) around a pluggable
`net(x6, t)`: any callable from the NCTHW concat [ x | self_cond ] and the
timesteps to the prediction.  With `oracle.dv_ref.Unet3D(channels=2C,
channels_out=C)` it is the network a self-conditioned Unet3D is arithmetically
equal to; with an elementwise function it is exact.
"""
import random

import pytest
import torch

import test_objectives_host as H

bc = H.bc


# ---- restatements ----------------------------------------------------------


def training_loss(net, sched, x_start, times, noise, hit, objective="eps", dtype=torch.float64):
    """p_losses of a self-conditioned unet (:1947-2002, l2, no p2 weights):
    `hit` is the outcome of `random.random() < 0.5`.  On a hit the first pass
    runs under no_grad on the zero self-cond input and its raw output,
    detached, is the self-conditioning of the second pass."""
    xs = x_start.to(dtype) * 2 - 1
    noise = noise.to(dtype)
    sa = bc(sched.sqrt_alphas_cumprod.to(dtype)[times])
    s1m = bc(sched.sqrt_one_minus_alphas_cumprod.to(dtype)[times])
    x_noisy = sa * xs + s1m * noise
    sc = torch.zeros_like(x_noisy)
    if hit:
        with torch.no_grad():
            sc = net(torch.cat((x_noisy, sc), dim=1), times).detach()
    pred = net(torch.cat((x_noisy, sc), dim=1), times)
    target = {"eps": noise, "x0": xs, "v": H.calculate_v(xs, noise, sa, s1m)}[objective]
    return ((pred - target) ** 2).flatten(1).mean(dim=-1).mean()


def _x0(sched, x, pred, t, objective, dtype):
    a = bc(sched.alphas_cumprod.to(dtype)[t])
    if objective == "v":
        return H.predict_start_from_v(x, pred, a.sqrt(), (1 - a).sqrt())
    if objective == "x0":
        return pred
    return H.predict_start_from_noise(x, pred, (1 / a).sqrt(), (1 / a - 1).sqrt())


def ddpm_steps(net, sched, x, times, noises, objective="eps", clip=True, dtype=torch.float64):
    """Consecutive p_sample steps (:1707-1744): times[i] is the (B,) timestep
    tensor of step i and noises[i] its draw.  Returns [(x_next, x0)] per step;
    step i + 1 reads step i's clamped x0 as its self-conditioning, step 0 zeros."""
    x = x.to(dtype)
    x_start, out = None, []
    for t, z in zip(times, noises):
        sc = torch.zeros_like(x) if x_start is None else x_start
        pred = net(torch.cat((x, sc), dim=1), t)
        x0 = _x0(sched, x, pred, t, objective, dtype)
        if clip:
            x0 = x0.clamp(-1.0, 1.0)
        mean = bc(sched.posterior_mean_coef1.to(dtype)[t]) * x0 + bc(sched.posterior_mean_coef2.to(dtype)[t]) * x
        logvar = bc(sched.posterior_log_variance_clipped.to(dtype)[t])
        nonzero = bc((t != 0).to(dtype))
        x, x_start = mean + nonzero * (0.5 * logvar).exp() * z.to(dtype), x0
        out.append((x, x_start))
    return out


def ddim_steps(net, sched, x, pairs, noises, eta, objective="eps", clip=True, dtype=torch.float64):
    """Consecutive DDIM steps (:1811-1876): pairs[i] = (t, t_next) tensors."""
    x = x.to(dtype)
    x_start, out = None, []
    for (t, tn), z in zip(pairs, noises):
        sc = torch.zeros_like(x) if x_start is None else x_start
        pred = net(torch.cat((x, sc), dim=1), t)
        a, an = bc(sched.alphas_cumprod.to(dtype)[t]), bc(sched.alphas_cumprod.to(dtype)[tn])
        x0 = _x0(sched, x, pred, t, objective, dtype)
        if clip:
            x0 = x0.clamp(-1.0, 1.0)
        pred_noise = H.predict_noise_from_start(x, x0, (1 / a).sqrt(), (1 / a - 1).sqrt())
        c1 = eta * ((1 - a / an) * (1 - an) / (1 - a)).sqrt()
        c2 = ((1 - an) - c1 ** 2).sqrt()
        z = torch.where(bc(tn == 0), torch.zeros_like(x), z.to(dtype))
        x, x_start = x0 * an.sqrt() + c1 * z + c2 * pred_noise, x0
        out.append((x, x_start))
    return out


def elementwise_net(x6, t):
    """A stand-in that reads all six input channels, elementwise and exact in
    float64: out_c = tanh(x_c)/2 + sc_(c+1)/4 + t/100."""
    x, sc = x6[:, :3], x6[:, 3:]
    return 0.5 * torch.tanh(x) + 0.25 * sc.roll(-1, dims=1) + 0.01 * bc(t).to(x6.dtype)


# ---- construction / plumbing -----------------------------------------------


def _unet(**kw):
    from dalle2_video import dalle2_video as D

    return D.Unet3D(16, dim_mults=(1, 2, 4, 8), channels=3, **kw)


def test_self_cond_unet_constructs():
    u = _unet(self_cond=True)
    assert u.self_cond and u.channels == 3 and u.channels_out == 3
    assert all(c.weight.shape[1] == 6 for c in u.init_conv.convs)
    assert all(c.weight.shape[1] == 3 for c in _unet().init_conv.convs)


def test_state_dict_is_the_six_channel_oracle_unets():
    from oracle import dv_ref as R

    u = _unet(self_cond=True)
    o = R.Unet3D(16, dim_mults=(1, 2, 4, 8), channels=6, channels_out=3)
    ours = {k: tuple(v.shape) for k, v in u.state_dict().items()}
    theirs = {k: tuple(v.shape) for k, v in o.state_dict().items()}
    assert list(ours) == list(theirs)
    assert ours == theirs


def test_cast_model_parameters_keeps_self_cond():
    from dalle2_video import dalle2_video as D

    u = _unet(self_cond=True)
    v = u.cast_model_parameters(lowres_cond=False, lowres_noise_cond=False, channels=2, channels_out=2,
                                cond_on_image_embeds=True, cond_on_text_encodings=False)
    assert v is not u and v.self_cond and v.channels == 2
    assert all(c.weight.shape[1] == 4 for c in v.init_conv.convs)
    dec = D.VideoDecoder(u, frame_sizes=(32,), frame_numbers=(4,), learned_variance=False)
    assert dec.unets[0].self_cond and dec.forced_self_cond is None
    assert all(c.weight.shape[1] == 6 for c in dec.unets[0].init_conv.convs)
    # 2 channels: x, self_cond and the low-res clip are 6 <= 8 input channels
    w = D.Unet3D(16, dim_mults=(1, 2), channels=2, self_cond=True, lowres_cond=True)
    assert all(c.weight.shape[1] == 6 for c in w.init_conv.convs)


def test_nine_input_channels_raise_at_construction():
    from dalle2_video import dalle2_video as D

    with pytest.raises(NotImplementedError, match=r"3 \* \(1 \+ 1 \+ 1\) = 9"):
        _unet(self_cond=True, lowres_cond=True)
    # the cascade's second unet is rebuilt with lowres_cond=True by the decoder
    with pytest.raises(NotImplementedError, match="9 input channels"):
        D.VideoDecoder((_unet(), _unet(self_cond=True)), frame_sizes=(32, 64), frame_numbers=(4, 4),
                       learned_variance=False)
    # without self_cond nothing changed: 3 + 3 channels build as before
    _unet(lowres_cond=True)


def test_plain_unet_draws_nothing_from_the_host_rng(monkeypatch):
    """p_losses consumes random.random() for self-conditioned unets only.  The
    call is cut short at the first device op (a CPU tensor raises DVError), past
    the point of the draw for a self-conditioned unet."""
    from dalle2_video import dalle2_video as D
    from dalle2_video._lib import DVError

    class Drew(Exception):
        pass

    def boom():
        raise Drew

    monkeypatch.setattr(random, "random", boom)
    x = torch.rand(1, 3, 4, 32, 32)
    t = torch.tensor([5])
    for sc, forced, want in ((False, None, DVError), (True, None, Drew), (True, False, DVError),
                             (True, True, DVError)):
        dec = D.VideoDecoder(_unet(self_cond=sc), frame_sizes=(32,), frame_numbers=(4,), learned_variance=False)
        dec.forced_self_cond = forced
        with pytest.raises(want):
            dec.p_losses(dec.unets[0], x, t, video_embed=None, noise_scheduler=dec.noise_schedulers[0],
                         noise=torch.randn(x.shape))


def test_bf16_is_refused_before_any_launch():
    """Self-conditioned unets run in f32 only: every
    entry point raises NotImplementedError before it touches a device (the
    tensors here are on the CPU, where a launch would raise DVError instead)."""
    from dalle2_video import dalle2_video as D

    dec = D.VideoDecoder(_unet(self_cond=True), frame_sizes=(32,), frame_numbers=(4,), learned_variance=False)
    u = dec.unets[0]
    u.compute_dtype = torch.bfloat16
    x, t = torch.rand(1, 3, 4, 32, 32), torch.tensor([5])
    with pytest.raises(NotImplementedError, match="f32 only"):
        u(x, t)
    with pytest.raises(NotImplementedError, match="f32 only"):
        u.forward_cl(torch.zeros(4, 32, 32, 8, dtype=torch.bfloat16), t, batch=1)
    dec.forced_self_cond = False
    with pytest.raises(NotImplementedError, match="f32 only"):
        dec.p_losses(u, x, t, video_embed=None, noise_scheduler=dec.noise_schedulers[0], noise=torch.randn(x.shape))
    u.compute_dtype = None
    with pytest.raises(NotImplementedError, match="captured"):  # no captured step in any dtype
        D._DenoiseStepGraph(dec, u, x, None, dec.noise_schedulers[0], 1.0, None, True)
    u.compute_dtype = torch.bfloat16
    # a plain unet is not affected: it gets as far as the device check
    from dalle2_video._lib import DVError
    plain = _unet()
    plain.compute_dtype = torch.bfloat16
    with pytest.raises(DVError):
        plain(x, t)


# ---- the restatements themselves -------------------------------------------


def _sched():
    from dalle2_video import dalle2_video as D

    return D.NoiseScheduler(beta_schedule="cosine", timesteps=1000, loss_type="l2")


def test_training_restatement_detaches_the_first_pass():
    """A linear net out = w * (x + sc): on a hit the loss depends on w through
    both passes, but the gradient sees the second only."""
    s = _sched()
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, 1, 2, 2, generator=g)
    z = torch.randn(x.shape, generator=g)
    t = torch.tensor([10, 700])
    w = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    net = lambda x6, t: w * (x6[:, :3] + x6[:, 3:])
    miss = training_loss(net, s, x, t, z, hit=False)
    hit = training_loss(net, s, x, t, z, hit=True)
    assert miss.item() != hit.item()
    (gh,) = torch.autograd.grad(hit, w)
    # the same loss with the first pass's output as a constant
    xs = x.double() * 2 - 1
    xn = bc(s.sqrt_alphas_cumprod.double()[t]) * xs + bc(s.sqrt_one_minus_alphas_cumprod.double()[t]) * z.double()
    const = (0.3 * xn).detach()
    w2 = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    l2 = ((w2 * (xn + const) - z.double()) ** 2).flatten(1).mean(-1).mean()
    (g2,) = torch.autograd.grad(l2, w2)
    assert abs(l2.item() - hit.item()) < 1e-14 and abs(gh.item() - g2.item()) < 1e-14


@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_sampling_restatement_carries_the_clamped_x0(kind):
    s = _sched()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 1, 2, 2, generator=g)
    zs = [torch.randn(x.shape, generator=g) for _ in range(2)]
    seen = []

    def net(x6, t):
        seen.append(x6[:, 3:].clone())
        return elementwise_net(x6, t)

    if kind == "ddpm":
        ts = [torch.tensor([999, 999]), torch.tensor([998, 998])]
        steps = ddpm_steps(net, s, x, ts, zs)
    else:
        pairs = [(torch.tensor([999, 999]), torch.tensor([500, 500])), (torch.tensor([500, 500]), torch.tensor([0, 0]))]
        steps = ddim_steps(net, s, x, pairs, zs, eta=1.0)
    assert torch.count_nonzero(seen[0]) == 0
    assert torch.equal(seen[1], steps[0][1]) and steps[0][1].abs().max() <= 1.0
    assert (steps[0][1].abs() == 1.0).any()  # t = 999: the clamp is active
