"""DDIM few-step sampling: the fused update kernel (ops.ddim_step /
dv_ddim_step), one decoder step, the loop (eager and graph replay) and the
cascade dispatch.

Expected values come from `ddim_restatement` below: the arithmetic of the
reference's p_sample_loop_ddim (dalle2_video.py:1811-1876) restated literally
in plain PyTorch and evaluated in float64 on the CPU, on the same f32
alphas_cumprod table the kernel reads.

Tolerances (norm-wise relative error per sample, checked below):
  kernel out / x0 vs float64         <= max(1e-6, 4 * e32), e32 = the error of
                                        the same restatement evaluated in f32
                                        (1e-6: the bar of the posterior update;
                                        4x: FMA contraction / operation order)
  coefficient probes (all t)         <= 1e-6 per element.  The kernel derives
                                        its coefficients from alphas_cumprod[t]
                                        and alphas_cumprod[t_next] on the device
                                        and gathers no precomputed table, so
                                        these are rel comparisons, not bit-equal
  decoder step vs oracle Unet3D      <= 1e-4 (forward bar)
  loop, graph replay vs eager        <  1e-5 (the DDPM graph test's bar)
The observed values are printed and appended to $DV_PARITY_LOG.
"""
import functools
import math

import pytest
import torch

from oracle import dv_ref as R

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def rel_per_sample(a, b):
    return [rel(a[i], b[i]) for i in range(b.shape[0])]


def ddim_restatement(x, eps, z, t, t_next, alphas_cumprod, eta, clip, dtype):
    """(x_next, x0) of one DDIM step, every operation in `dtype` on the CPU."""
    x, eps, z = x.cpu().to(dtype), eps.cpu().to(dtype), z.cpu().to(dtype)
    t, t_next = t.cpu(), t_next.cpu()
    bc = lambda v: v.reshape(-1, 1, 1, 1, 1)
    a = bc(alphas_cumprod.cpu().to(dtype)[t])
    a_next = bc(alphas_cumprod.cpu().to(dtype)[t_next])
    sqrt_recip, sqrt_recipm1 = (1 / a).sqrt(), (1 / a - 1).sqrt()
    x0 = sqrt_recip * x - sqrt_recipm1 * eps
    if clip:
        x0 = x0.clamp(-1.0, 1.0)
    pred_noise = (sqrt_recip * x - x0) / sqrt_recipm1
    c1 = eta * ((1 - a / a_next) * (1 - a_next) / (1 - a)).sqrt()
    c2 = ((1 - a_next) - c1 ** 2).sqrt()
    z = torch.where(bc(t_next == 0), torch.zeros_like(z), z)  # the last step takes no noise
    return x0 * a_next.sqrt() + c1 * z + c2 * pred_noise, x0


@functools.lru_cache(maxsize=None)
def _sched(kind, timesteps=1000):
    from dalle2_video import dalle2_video as D

    return D.NoiseScheduler(beta_schedule=kind, timesteps=timesteps, loss_type="l2").cuda()


@functools.lru_cache(maxsize=None)
def _kernel_inputs():
    g = torch.Generator().manual_seed(41)
    x = torch.randn(4, 3, 4, 8, 8, generator=g)
    eps = torch.randn(x.shape, generator=g)
    z = torch.randn(x.shape, generator=g)
    return x, eps, z, torch.tensor([1, 3, 537, 999]), torch.tensor([0, 1, 500, 958])


@pytest.mark.parametrize("form", ["ncthw", "cl_f32", "cl_bf16"])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("kind", ["cosine", "linear"])
def test_ddim_step_vs_float64_restatement(parity_log, kind, eta, clip, form):
    """t = 1 -> 0 (no noise, clamp active, the badly conditioned pred_noise),
    3 -> 1, 537 -> 500 and 999 -> 958 (clamp active) in one batch."""
    from dalle2_video import ops

    s = _sched(kind)
    x, eps, z, t, tn = _kernel_inputs()
    if form == "ncthw":
        eps_dev = eps.cuda()
    elif form == "cl_f32":
        eps_dev = ops.to_cl(eps.cuda(), torch.float32)
    else:
        eps_dev = ops.to_cl(eps.cuda(), torch.bfloat16)
        eps = eps.bfloat16().float()  # the restatement gets the rounded eps
    noise = None
    if eta != 0:
        noise = z.clone()
        noise[0] = float("nan")  # t_next == 0: the kernel must not touch this sample's noise
        noise = noise.cuda()
    out, x0 = ops.ddim_step(x.cuda(), eps_dev, noise, t.cuda(), tn.cuda(), s, eta, clip_denoised=clip)
    assert torch.isfinite(out).all() and torch.isfinite(x0).all()
    ac = s.alphas_cumprod
    out64, x064 = ddim_restatement(x, eps, z, t, tn, ac, eta, clip, torch.float64)
    out32, x032 = ddim_restatement(x, eps, z, t, tn, ac, eta, clip, torch.float32)
    for name, got, want, f32 in (("out", out, out64, out32), ("x0", x0, x064, x032)):
        e32 = rel_per_sample(f32, want)
        err = rel_per_sample(got, want)
        # a non-finite f32 restatement (its c2 can cancel below zero) allows nothing extra
        tol = [max(1e-6, 4 * e) if math.isfinite(e) else 1e-6 for e in e32]
        parity_log(kind=kind, eta=eta, clip=clip, form=form, what=name, rel=err, e32=e32, tol=tol)
        assert all(e <= b for e, b in zip(err, tol)), (name, err, tol)
    if eta == 0 and form == "ncthw":
        # eta == 0 reads no noise: a given tensor changes nothing
        out_z, _ = ops.ddim_step(x.cuda(), eps_dev, z.cuda(), t.cuda(), tn.cuda(), s, eta, clip_denoised=clip)
        assert torch.equal(out_z, out)
        # and the update may run in place
        xin = x.cuda().clone()
        out_ip, _ = ops.ddim_step(xin, eps_dev, None, t.cuda(), tn.cuda(), s, eta, clip_denoised=clip, out=xin,
                                  want_x0=False)
        assert out_ip is xin and torch.equal(xin, out)


@pytest.mark.parametrize("kind", ["cosine", "linear"])
def test_ddim_coefficients_every_pair(kind):
    """Every pair (t, t - 1), t in [1, 1000), clip off, eta = 0: probe inputs
    make x0 / out a single coefficient of the gathered entries.  The kernel
    computes sqrt(1/a), sqrt(1/a - 1), sqrt(a_next) and sqrt(1 - a_next) from
    the f32 alphas_cumprod table on the device (no precomputed table is
    gathered), so each is compared with rel < 1e-6 instead of bit-equal; a
    wrong gather of t or t_next is off by far more (adjacent entries of
    sqrt_recip_alphas_cumprod differ by > 1e-5 relative over most of the
    schedule, and the comparison runs over all 999 pairs)."""
    from dalle2_video import ops

    s = _sched(kind)
    t = torch.arange(1, 1000, device="cuda")
    tn = t - 1
    B = t.numel()
    one = torch.ones(B, 3, 1, 2, 2, device="cuda")
    zero = torch.zeros_like(one)
    a = s.alphas_cumprod.double().cpu()[t.cpu()]
    an = s.alphas_cumprod.double().cpu()[tn.cpu()]
    flat = lambda v: v.reshape(B, -1).double().cpu()
    col = lambda v: v[:, None].expand(B, 12)
    relmax = lambda got, want: ((got - want).abs() / want.abs()).max().item()
    # x = 1, eps = 0: x0 = sqrt(1/a[t]) (the table entry), out = sqrt(a[t-1]) sqrt(1/a[t])
    out, x0 = ops.ddim_step(one, zero, None, t, tn, s, 0.0, clip_denoised=False)
    table = s.sqrt_recip_alphas_cumprod.double().cpu()[t.cpu()]
    assert relmax(flat(x0), col(table)) < 1e-6
    assert relmax(flat(x0), col((1 / a).sqrt())) < 1e-6
    assert relmax(flat(out), col(an.sqrt() * (1 / a).sqrt())) < 1e-6
    # x = 0, eps = -1: x0 = sqrt(1/a[t] - 1); out = sqrt(a[t-1]) x0 - sqrt(1 - a[t-1]).
    # The two terms of out nearly cancel for neighbouring steps: the bound is
    # 1e-6 of their magnitudes.
    out, x0 = ops.ddim_step(zero, -one, None, t, tn, s, 0.0, clip_denoised=False)
    srm1 = (1 / a - 1).sqrt()
    assert relmax(flat(x0), col(srm1)) < 1e-6
    want, mag = an.sqrt() * srm1 - (1 - an).sqrt(), an.sqrt() * srm1 + (1 - an).sqrt()
    assert ((flat(out) - col(want)).abs() / col(mag)).max().item() < 1e-6
    # x = 0, eps = 0, eta = 1, noise = 1: out = c1 (exactly 0 where t_next == 0)
    out, _ = ops.ddim_step(zero, zero, one, t, tn, s, 1.0, clip_denoised=False)
    c1 = ((1 - a / an) * (1 - an) / (1 - a)).sqrt()
    got = flat(out)
    assert (got[0] == 0).all()
    assert relmax(got[1:], col(c1)[1:]) < 1e-6


def test_ddim_out_of_schedule_pairs_poison_output():
    """t or t_next outside [0, num_timesteps), or t_next >= t: NaN for that
    sample, nothing read past the table; the good pair is untouched."""
    from dalle2_video import ops

    s = _sched("cosine")
    x = torch.rand(6, 3, 2, 4, 4, device="cuda")
    t = torch.tensor([5, 1000, 5, 5, 3, -2], device="cuda")
    tn = torch.tensor([2, 3, -1, 5, 7, -3], device="cuda")
    for eta, noise in ((1.0, x), (0.0, None)):
        out, x0 = ops.ddim_step(x, x, noise, t, tn, s, eta)
        assert torch.isfinite(out[0]).all() and torch.isfinite(x0[0]).all()
        assert torch.isnan(out[1:]).all() and torch.isnan(x0[1:]).all()


def test_ddim_step_rejects_missing_noise():
    from dalle2_video import _lib, ops

    s = _sched("cosine")
    x = torch.rand(1, 3, 2, 4, 4, device="cuda")
    t, tn = torch.tensor([5], device="cuda"), torch.tensor([2], device="cuda")
    with pytest.raises(_lib.DVError, match="noise"):
        ops.ddim_step(x, x, None, t, tn, s, 0.5)


def _unet1_pair():
    from dalle2_video import dalle2_video as D

    mk = lambda mod: mod.Unet3D(64, video_embed_dim=512, channels=3, dim_mults=(1, 2, 4, 8)).cast_model_parameters(
        lowres_cond=False, lowres_noise_cond=False, channels=3, channels_out=3, cond_on_image_embeds=True,
        cond_on_text_encodings=False)
    ou = R.deterministic_fill_(mk(R))
    dec = D.VideoDecoder(mk(D), frame_sizes=(32,), frame_numbers=(8,), timesteps=1000, learned_variance=False)
    dec.unets[0].load_state_dict(ou.state_dict(), strict=True)
    return ou, dec.cuda()


def test_decoder_ddim_step_vs_oracle_unet(parity_log):
    """One DDIM step 537 -> 500 at Cfg1 (unet1, 1x3x8x32x32, f32): the oracle
    Unet3D forward on the CPU, then the float64 restatement."""
    ou, dec = _unet1_pair()
    g = torch.Generator().manual_seed(43)
    x = torch.randn(1, 3, 8, 32, 32, generator=g)
    z = torch.randn(x.shape, generator=g)
    t, tn = torch.tensor([537]), torch.tensor([500])
    sched = dec.noise_schedulers[0]
    with torch.no_grad():
        eps = ou.forward_with_cond_scale(x, t, video_embed=None, lowres_cond_video=None, cond_scale=1.0)
    outr, x0r = ddim_restatement(x, eps, z, t, tn, sched.alphas_cumprod, 1.0, True, torch.float64)
    out, x0 = dec.p_sample_ddim(dec.unets[0], x.cuda(), t.cuda(), tn.cuda(), video_embed=None,
                                noise_scheduler=sched, eta=1.0, clip_denoised=True, noise=z.cuda())
    e_out, e_x0 = rel(out, outr), rel(x0, x0r)
    parity_log(pair=[537, 500], out_rel=e_out, x0_rel=e_x0)
    assert e_out <= 1e-4 and e_x0 <= 1e-4


def _small_decoder(eta):
    from dalle2_video import dalle2_video as D
    from dalle2_video.utils import deterministic_fill_

    u = D.Unet3D(16, video_embed_dim=512, channels=3, dim_mults=(1, 2, 4, 8))
    dec = D.VideoDecoder(u, frame_sizes=(32,), frame_numbers=(4,), timesteps=20, sample_timesteps=6,
                         ddim_sampling_eta=eta, learned_variance=False)
    deterministic_fill_(dec.unets[0])
    return dec.cuda()


@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("cond_scale", [1.0, 2.0])
def test_ddim_loop_graph_replay_matches_eager(parity_log, cond_scale, eta):
    """sample() with sample_timesteps=6 of 20: six DDIM steps, with the
    captured denoise-step graph two eager, one capture + replay, three
    replays; same seed -> the eager loop's result."""
    dec = _small_decoder(eta)
    outs = []
    for graphs in (False, True):
        dec.sample_graphs = graphs
        torch.cuda.manual_seed(77)
        outs.append(dec.sample(video_embed=torch.zeros(2, 512, device="cuda"), cond_scale=cond_scale))
    eager, graph = outs
    assert eager.shape == (2, 3, 4, 32, 32) and graph.shape == (2, 3, 4, 32, 32)
    assert torch.isfinite(eager).all()
    e = rel(graph, eager)
    parity_log(cond_scale=cond_scale, eta=eta, graph_vs_eager_rel=e)
    assert e < 1e-5


class _ElementwiseDenoiser(torch.nn.Module):
    """A bit-reproducible stand-in for the unet: eps is an elementwise function
    of (x, t).  Unet3D's forward is not reproducible to the bit from run to run
    (its GroupNorm statistics are float atomic sums), so a bit-equality check
    of the loop needs a denoiser that is."""

    def forward_with_cond_scale(self, x, t, video_embed=None, cond_scale=1.0, lowres_cond_video=None):
        return 0.5 * torch.tanh(x) + 0.01 * t.reshape(-1, 1, 1, 1, 1).float()


def _eta_zero_runs(dec, unet, graphs, **kw):
    """The eta = 0 loop twice from one fixed start tensor; the second time the
    device generator is advanced by a dummy draw before the loop.  Asserts that
    the loop leaves the generator state untouched; returns both results."""
    dec.sample_graphs = graphs
    shape = (2, 3, 4, 32, 32)
    outs = []
    for extra_draw in (False, True):
        torch.cuda.manual_seed(5)
        start = torch.randn(shape, device="cuda")
        if extra_draw:
            torch.randn(4096, device="cuda")
        before = torch.cuda.get_rng_state()
        outs.append(dec.p_sample_loop_ddim(unet, shape, noise_scheduler=dec.noise_schedulers[0], timesteps=6,
                                           init_noise=start, **kw))
        torch.cuda.synchronize()
        assert torch.equal(torch.cuda.get_rng_state(), before), "the eta == 0 loop drew from the generator"
    assert torch.isfinite(outs[0]).all()
    return outs


@pytest.mark.parametrize("graphs", [False, True])
def test_ddim_eta_zero_draws_no_noise(graphs):
    """At eta == 0 the loop consumes nothing from the device generator: an
    extra draw between the start tensor and the loop changes no bit of the
    result, and the generator state after the loop is the state before it.
    Run with the reproducible stand-in denoiser (cond_scale = 2: the captured
    step calls forward_with_cond_scale), six steps of 20."""
    dec = _small_decoder(0.0).eval()
    a, b = _eta_zero_runs(dec, _ElementwiseDenoiser(), graphs, video_embed=None, cond_scale=2.0)
    assert torch.equal(a, b)


@pytest.mark.parametrize("graphs", [False, True])
def test_ddim_eta_zero_draws_no_noise_unet3d(parity_log, graphs):
    """The same two runs through Unet3D: the generator state is untouched, and
    the results agree to the forward's run-to-run floor (atomic sums; the bar
    is the graph-vs-eager test's 1e-5, not bit equality)."""
    dec = _small_decoder(0.0).eval()
    a, b = _eta_zero_runs(dec, dec.unets[0], graphs, video_embed=torch.zeros(2, 512, device="cuda"))
    e = rel(a, b)
    parity_log(graphs=graphs, run_to_run_rel=e, bit_equal=bool(torch.equal(a, b)))
    assert e < 1e-5


def test_cascade_mixes_ddim_and_ddpm():
    """sample_timesteps=(4, None) of 12: unet1 takes 4 DDIM steps, unet2 the 12
    DDPM steps (counted Unet3D forwards, eager loops).

    Both unets get the cosine schedule here.  The default gives the last unet
    of a cascade the linear schedule, whose betas are (1000 / T) * [1e-4, 0.02]:
    above 1 for T < 20, so at T = 12 alphas_cumprod turns negative and the
    schedule tables hold NaN for either sampler.

    The forwards are counted by wrapping each unet's `forward`:
    forward_with_cond_scale calls self.forward directly, which
    nn.Module forward hooks (attached to __call__) never see."""
    from dalle2_video import dalle2_video as D

    base = D.Unet3D(8, video_embed_dim=512, channels=3, dim_mults=(1, 2))
    sr = D.Unet3D(8, video_embed_dim=512, channels=3, dim_mults=(1, 2, 4, 8, 16), cond_on_text_encodings=False)
    dec = D.VideoDecoder((base, sr), frame_sizes=(32, 64), frame_numbers=(2, 2), timesteps=12,
                         sample_timesteps=(4, None), beta_schedule=("cosine", "cosine"),
                         learned_variance=False).cuda()
    dec.sample_graphs = False  # graph replays run no Python: count the eager forwards
    counts = [0, 0]

    def counted(i, fwd):
        def forward(*args, **kwargs):
            counts[i] += 1
            return fwd(*args, **kwargs)
        return forward

    for i, u in enumerate(dec.unets):
        u.forward = counted(i, u.forward)
    torch.cuda.manual_seed(3)
    vid = dec.sample(video_embed=torch.zeros(1, 512, device="cuda"))
    for u in dec.unets:
        del u.forward
    assert vid.shape == (1, 3, 2, 64, 64)
    assert torch.isfinite(vid).all() and vid.min() >= 0 and vid.max() <= 1
    assert counts == [4, 12]
    # the same cascade through the captured step graphs
    dec.sample_graphs = True
    torch.cuda.manual_seed(3)
    vid_g = dec.sample(video_embed=torch.zeros(1, 512, device="cuda"))
    assert vid_g.shape == (1, 3, 2, 64, 64) and torch.isfinite(vid_g).all()
