"""Self-conditioning on the GPU: dv_q_sample_sc, Unet3D(self_cond=True)
against the oracle, the two-pass training step, the (eager) sampling loops and
the trainer's two captured variants.  All in f32: self-conditioned unets refuse
bf16, and their sampling step is not captured.

Oracle: `oracle.dv_ref.Unet3D(channels=6, channels_out=3)` with the same
weights is arithmetically the self-conditioned 3-channel network on
cat(x, self_cond); the restatements of tests/test_self_cond_host.py drive it.

Bars (norm-wise relative error unless "equal"):
  dv_q_sample_sc                   equal (bit patterns)
  forward vs oracle, f32           <= 1e-4  (test_unet_gpu's forward bar)
  training loss / gradients, f32   <= 1e-4 / <= 1e-3  (test_p_losses_forward_backward_vs_oracle)
  two sampling steps vs oracle     <= 1e-4  (test_decoder_ddim_step_vs_oracle_unet)
  loops                            equal to step-by-step calls with the
                                   elementwise stand-in
  trainer replay vs eager, f32     <= 1e-5 loss and flat gradient
                                   (test_cfg2_trainer_graph_replay_vs_eager_vs_oracle)
"""
import functools
import json
import os
import random

import pytest
import torch

import test_self_cond_host as H
from oracle import dv_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_step_launches.json")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def bits_equal(a, b):
    """torch.equal on the bit patterns (so -0 differs from 0), except that NaN
    equals NaN whatever its payload (an out-of-schedule sample)."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    both_nan = a.isnan() & b.isnan()
    a, b = a.masked_fill(both_nan, 0).contiguous(), b.masked_fill(both_nan, 0).contiguous()
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.view(it), b.view(it))


def cl_of(x):
    """(B, C, T, H, W) -> channels-last frames (B*T, H, W, C)."""
    b, c, t, h, w = x.shape
    return x.permute(0, 2, 3, 4, 1).reshape(b * t, h, w, c).contiguous()


@functools.lru_cache(maxsize=None)
def _sched():
    from dalle2_video import dalle2_video as D

    return D.NoiseScheduler(beta_schedule="cosine", timesteps=1000, loss_type="l2").cuda()


def _source(kind, stride, npix_shape, csc, gen):
    """(tensor given to the kernel, its values as f32 frames) for a source kind."""
    if kind == "null":
        return None, torch.zeros(*npix_shape, csc)
    buf = torch.randn(*npix_shape, stride, generator=gen)
    buf = (buf.bfloat16() if kind == "bf16" else buf).cuda()
    view = buf[..., :csc]
    return view, view.float().cpu()


# ---------------------------------------------------------------------------
# 3. dv_q_sample_sc
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["null", "f32", "bf16"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_q_sample_sc(dtype, kind):
    from dalle2_video import ops

    s = _sched()
    shape = (2, 3, 2, 5, 7)
    g = torch.Generator().manual_seed(9)
    x0, z = torch.rand(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
    t = torch.tensor([3, 999], device="cuda")
    src, vals = _source(kind, 8, (4, 5, 7), 3, g)
    plain = ops.q_sample_cl(x0, z, t, s.sqrt_alphas_cumprod, s.sqrt_one_minus_alphas_cumprod, dtype)
    y = ops.q_sample_cl(x0, z, t, s.sqrt_alphas_cumprod, s.sqrt_one_minus_alphas_cumprod, dtype,
                        self_cond_cl=src, csc=3)
    assert y.shape == (4, 5, 7, 8)
    assert bits_equal(y[..., :3], plain[..., :3])
    assert torch.equal(y[..., 3:6].cpu(), vals.to(dtype))
    assert (y[..., 6:] == 0).all()


# ---------------------------------------------------------------------------
# 4-6. Unet3D(self_cond=True) and the decoder against the 6 -> 3 oracle unet
# ---------------------------------------------------------------------------

MK = dict(dim_mults=(1, 2, 4, 8))


@functools.lru_cache(maxsize=None)
def _pair():
    """(oracle 6 -> 3 unet on the CPU, decoder holding our self-conditioned unet
    with the same weights).  Shared and never modified."""
    from dalle2_video import dalle2_video as D

    ou = R.deterministic_fill_(R.Unet3D(16, channels=6, channels_out=3, **MK))
    dec = D.VideoDecoder(D.Unet3D(16, channels=3, self_cond=True, **MK), frame_sizes=(32,), frame_numbers=(4,),
                         timesteps=1000, learned_variance=False)
    dec.unets[0].load_state_dict(ou.state_dict(), strict=True)
    return ou, dec.cuda()


@functools.lru_cache(maxsize=None)
def _clip_inputs():
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(2, 3, 4, 32, 32, generator=g)
    sc = torch.randn(x.shape, generator=g).clamp(-1, 1)
    zs = tuple(torch.randn(x.shape, generator=g) for _ in range(2))
    return x, sc, zs


def _oracle_net(ou):
    return lambda x6, t: ou(x6.float(), t)


def test_forward_vs_oracle(parity_log):
    ou, dec = _pair()
    u = dec.unets[0]
    x, sc, _ = _clip_inputs()
    t = torch.tensor([537, 3])
    with torch.no_grad():
        want = ou(torch.cat((x, sc), dim=1), t)
        want0 = ou(torch.cat((x, torch.zeros_like(sc)), dim=1), t)
        got = u(x.cuda(), t.cuda(), self_cond=sc.cuda())
        got0 = u(x.cuda(), t.cuda())
        gotz = u(x.cuda(), t.cuda(), self_cond=torch.zeros_like(sc).cuda())
    e, e0, ez = rel(got, want), rel(got0, want0), rel(gotz, got0)
    parity_log(forward_rel=e, none_rel=e0, none_vs_zero_rel=ez, moved=rel(want, want0))
    assert e <= 1e-4 and e0 <= 1e-4 and ez <= 1e-5
    assert rel(want, want0) > 1e-3  # the self-conditioning channels reach the output


def _graph_size(loss):
    seen, stack = set(), [loss.grad_fn]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        stack += [f for f, _ in fn.next_functions]
    return len(seen)


@pytest.mark.parametrize("hit", [False, True])
def test_training_loss_vs_oracle(parity_log, hit):
    """p_losses with the decision pinned against the two-pass restatement on
    the oracle unet (f32 on the CPU).  No gradient flows through the first
    pass: what it feeds is a detached tensor, and the autograd graph of the
    loss has the size of the single-pass call's (the first pass adds no node)."""
    from dalle2_video import dalle2_video as D, ops

    ou, _ = _pair()
    dec = D.VideoDecoder(D.Unet3D(16, channels=3, self_cond=True, **MK), frame_sizes=(32,), frame_numbers=(4,),
                         timesteps=1000, learned_variance=False)
    dec.unets[0].load_state_dict(ou.state_dict(), strict=True)
    dec = dec.cuda()
    u = dec.unets[0]
    g = torch.Generator().manual_seed(77)
    xs = torch.rand(2, 3, 4, 32, 32, generator=g)
    noise = torch.randn(xs.shape, generator=g)
    t = torch.tensor([537, 3])
    ou.zero_grad()
    sched_cpu = D.NoiseScheduler(beta_schedule="cosine", timesteps=1000, loss_type="l2")
    lo = H.training_loss(_oracle_net(ou), sched_cpu, xs, t, noise, hit, dtype=torch.float32)
    lo.backward()

    fed = []
    orig = ops.q_sample_cl

    def spy(*a, **kw):
        fed.append(kw.get("self_cond_cl"))
        return orig(*a, **kw)

    sizes = {}
    for forced in (hit, False):
        dec.forced_self_cond = forced
        u.zero_grad()
        fed.clear()
        ops.q_sample_cl = spy
        try:
            loss = dec.p_losses(u, xs.cuda(), t.cuda(), video_embed=None, noise_scheduler=dec.noise_schedulers[0],
                                noise=noise.cuda())
        finally:
            ops.q_sample_cl = orig
        sizes[forced] = _graph_size(loss)
        if forced == hit:
            assert len(fed) == (2 if hit else 1) and fed[0] is None
            if hit:
                assert fed[1] is not None and not fed[1].requires_grad and fed[1].grad_fn is None
            loss.backward()
            errs = {"loss": abs(loss.item() - lo.item()) / abs(lo.item()),
                    "to_out": rel(u.to_out.weight.grad, ou.to_out.weight.grad)}
            for i, (c, co) in enumerate(zip(u.init_conv.convs, ou.init_conv.convs)):
                errs[f"init_conv{i}"] = rel(c.weight.grad, co.weight.grad)
    assert sizes[hit] == sizes[False], sizes
    parity_log(hit=hit, **errs)
    assert errs.pop("loss") <= 1e-4
    assert all(v <= 1e-3 for v in errs.values()), errs
    ou.zero_grad()


def test_no_gradient_flows_through_the_first_pass(parity_log):
    """A parameter gradient is unchanged when the first pass's conditioning is
    perturbed.  The parameters are null_video_embed / null_video_hiddens of a
    video-conditioned self-conditioned unet: they enter a forward only for
    samples whose conditioning is dropped.  The real pass keeps every sample
    (drop probability 0), so their gradient is exactly zero.  The perturbed run
    drops the conditioning of every sample in the FIRST pass, which now goes
    through those parameters: the self-conditioning it feeds changes (and with
    it the other gradients), but theirs stays exactly zero, since nothing
    flows back through that pass."""
    from dalle2_video import dalle2_video as D
    from dalle2_video.utils import deterministic_fill_

    u = D.Unet3D(8, video_embed_dim=512, channels=3, dim_mults=(1, 2), cond_on_video_embeds=True, self_cond=True)
    dec = D.VideoDecoder(u, frame_sizes=(32,), frame_numbers=(2,), timesteps=1000, learned_variance=False,
                         video_cond_drop_prob=0.0, text_cond_drop_prob=0.0)
    assert dec.unets[0] is u
    deterministic_fill_(u)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in u.named_parameters():  # the video projections get no deterministic fill
            if n.startswith(("video_to_tokens.", "to_video_hiddens.")):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.05)
    dec = dec.cuda()
    dec.forced_self_cond = True
    xs = torch.rand(2, 3, 2, 32, 32, generator=gen).cuda()
    noise = torch.randn(xs.shape, generator=gen).cuda()
    emb = torch.randn(2, 512, generator=gen).cuda()
    t = torch.tensor([537, 3], device="cuda")
    orig = u._forward_cl
    first_pass_calls = []

    def perturbed(x, time, **kw):
        if not torch.is_grad_enabled():  # the first pass
            first_pass_calls.append(1)
            kw["video_cond_drop_prob"] = 1.0
        return orig(x, time, **kw)

    grads = {}
    for tag in ("plain", "perturbed"):
        u.zero_grad()
        if tag == "perturbed":
            u._forward_cl = perturbed
        try:
            loss = dec.p_losses(u, xs, t, video_embed=emb, noise_scheduler=dec.noise_schedulers[0], noise=noise)
            loss.backward()
        finally:
            u.__dict__.pop("_forward_cl", None)
        grads[tag] = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in u.named_parameters()}
    assert first_pass_calls == [1]
    for tag in grads:
        for n in ("null_video_embed", "null_video_hiddens"):
            g = grads[tag][n]
            assert g is None or torch.count_nonzero(g) == 0, (tag, n)
    moved = rel(grads["perturbed"]["to_out.weight"], grads["plain"]["to_out.weight"])
    parity_log(to_out_grad_moved=moved)
    assert moved > 1e-4  # the perturbation did reach the real pass, through the value it feeds


def _two_steps_ours(dec, kind, objective, x, zs, ts):
    u, s = dec.unets[0], dec.noise_schedulers[0]
    kw = dict(video_embed=None, noise_scheduler=s, predict_x_start=objective == "x0", predict_v=objective == "v")
    x0, out = None, []
    x = x.cuda()
    for step, z in zip(ts, zs):
        if kind == "ddpm":
            x, x0 = dec.p_sample(u, x, step.cuda(), self_cond=x0, noise=z.cuda(), **kw)
        else:
            x, x0 = dec.p_sample_ddim(u, x, step[0].cuda(), step[1].cuda(), eta=1.0, self_cond=x0, noise=z.cuda(),
                                      **kw)
        out.append((x, x0))
    return out


@pytest.mark.parametrize("objective", ["eps", "v"])
@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_two_sampling_steps_vs_oracle(parity_log, kind, objective):
    """Two consecutive steps with fixed noise through VideoDecoder.p_sample /
    p_sample_ddim, carrying x0 as the loops do."""
    from dalle2_video import dalle2_video as D

    ou, dec = _pair()
    x, _, zs = _clip_inputs()
    s = dec.noise_schedulers[0]
    scpu = D.NoiseScheduler(beta_schedule="cosine", timesteps=1000, loss_type="l2")
    net = _oracle_net(ou)
    if kind == "ddpm":
        ts = [torch.tensor([537, 999]), torch.tensor([536, 998])]
    else:
        ts = [(torch.tensor([537, 999]), torch.tensor([500, 958])), (torch.tensor([500, 958]), torch.tensor([460, 917]))]
    steps = lambda ts_, zs_: (H.ddpm_steps(net, scpu, x, ts_, zs_, objective=objective) if kind == "ddpm"
                              else H.ddim_steps(net, scpu, x, ts_, zs_, 1.0, objective=objective))
    with torch.no_grad():
        want = steps(ts, zs)
        got = _two_steps_ours(dec, kind, objective, x, zs, ts)
    errs = {"x1": rel(got[0][0], want[0][0]), "x0_1": rel(got[0][1], want[0][1]),
            "x2": rel(got[1][0], want[1][0]), "x0_2": rel(got[1][1], want[1][1])}
    parity_log(kind=kind, objective=objective, **errs)
    assert all(v <= 1e-4 for v in errs.values()), errs
    # the second step read the first step's x0: with zeros instead it lands elsewhere
    with torch.no_grad():
        if kind == "ddpm":
            alt, _ = dec.p_sample(dec.unets[0], got[0][0], ts[1].cuda(), video_embed=None, noise_scheduler=s,
                                  predict_v=objective == "v", noise=zs[1].cuda())
        else:
            alt, _ = dec.p_sample_ddim(dec.unets[0], got[0][0], ts[1][0].cuda(), ts[1][1].cuda(), video_embed=None,
                                       noise_scheduler=s, eta=1.0, predict_v=objective == "v", noise=zs[1].cuda())
    assert rel(alt, got[1][0]) > 1e-3


# ---------------------------------------------------------------------------
# 7. loops: the x0 of one step is the self-conditioning of the next
# ---------------------------------------------------------------------------


class _ElementwiseSelfCond(torch.nn.Module):
    """A bit-reproducible self-conditioned stand-in (H.elementwise_net): reads
    all six input channels."""
    self_cond = True
    channels = 3

    @staticmethod
    def _f(x, sc, tt, rolled_dim, drop):
        return 0.5 * torch.tanh(x) + 0.25 * sc.roll(-1, dims=rolled_dim) + (0.005 if drop else 0.01) * tt

    def forward(self, x, t, self_cond=None, video_cond_drop_prob=0.0, **kw):
        sc = torch.zeros_like(x) if self_cond is None else self_cond
        return self._f(x, sc, t.float().reshape(-1, 1, 1, 1, 1), 1, video_cond_drop_prob == 1.0)

    def forward_with_cond_scale(self, x, t, video_embed=None, cond_scale=1.0, lowres_cond_video=None, self_cond=None):
        logits = self.forward(x, t, self_cond=self_cond)
        if cond_scale == 1:
            return logits
        null = self.forward(x, t, self_cond=self_cond, video_cond_drop_prob=1.0)
        return null + (logits - null) * cond_scale


def _loop_decoder(unet, ddim, eta=1.0):
    from dalle2_video import dalle2_video as D
    from dalle2_video.utils import deterministic_fill_

    kw = dict(timesteps=20, sample_timesteps=6, ddim_sampling_eta=eta) if ddim else dict(timesteps=6)
    dec = D.VideoDecoder(unet, frame_sizes=(32,), frame_numbers=(4,), learned_variance=False, **kw)
    deterministic_fill_(dec.unets[0])
    return dec.cuda().eval()


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("cond_scale", [1.0, 2.0])
@pytest.mark.parametrize("ddim", [False, True])
def test_loops_carry_x0_with_elementwise_denoiser(ddim, cond_scale, graphs):
    """Six steps, DDPM and DDIM eta = 1, against the same steps taken one by one
    with p_sample / p_sample_ddim handing x0 over by hand: equal to the bit.
    sample_graphs changes nothing for a self-conditioned denoiser (its step is
    not captured); a loop that dropped the self-conditioning would differ."""
    from dalle2_video import dalle2_video as D

    dec = _loop_decoder(D.Unet3D(8, channels=3, dim_mults=(1, 2)), ddim)
    dec.sample_graphs = graphs
    net, s, shape = _ElementwiseSelfCond(), dec.noise_schedulers[0], (2, 3, 4, 32, 32)
    torch.cuda.manual_seed(77)
    if ddim:
        got = dec.p_sample_loop_ddim(net, shape, None, s, 6, cond_scale=cond_scale)
    else:
        got = dec.p_sample_loop_ddpm(net, shape, None, s, cond_scale=cond_scale)

    def by_hand(carry):
        torch.cuda.manual_seed(77)
        vid, x0 = torch.randn(shape, device="cuda"), None
        steps = D.ddim_time_pairs(20, 6) if ddim else [(t, None) for t in reversed(range(6))]
        for time, time_next in steps:
            tt = torch.full((2,), time, device="cuda", dtype=torch.long)
            sc = x0 if carry else None
            if ddim:
                tn = torch.full((2,), time_next, device="cuda", dtype=torch.long)
                vid, x0 = dec.p_sample_ddim(net, vid, tt, tn, None, s, 1.0, cond_scale=cond_scale, self_cond=sc)
            else:
                vid, x0 = dec.p_sample(net, vid, tt, None, s, cond_scale=cond_scale, self_cond=sc)
        return dec.unnormalize_video(vid)

    assert torch.isfinite(got).all()
    assert torch.equal(got, by_hand(True))
    assert not torch.equal(got, by_hand(False))


@pytest.mark.parametrize("ddim", [False, True])
def test_sample_runs_with_unet3d_and_is_reproducible(parity_log, ddim):
    """sample() of a self-conditioned Unet3D: the loops run eagerly whatever
    sample_graphs says, and two runs from one seed agree to the forward's
    run-to-run floor (< 1e-5, the bar of the graph-vs-eager tests)."""
    from dalle2_video import dalle2_video as D

    dec = _loop_decoder(D.Unet3D(16, channels=3, self_cond=True, **MK), ddim)
    outs = []
    for graphs in (False, True):
        dec.sample_graphs = graphs
        torch.cuda.manual_seed(77)
        outs.append(dec.sample(batch_size=2, video_embed=torch.zeros(2, 512, device="cuda")))
    assert outs[0].shape == (2, 3, 4, 32, 32) and torch.isfinite(outs[0]).all()
    e = rel(outs[1], outs[0])
    parity_log(ddim=ddim, rerun_rel=e)
    assert e < 1e-5
    with pytest.raises(NotImplementedError, match="captured"):
        D._DenoiseStepGraph(dec, dec.unets[0], outs[0], None, dec.noise_schedulers[0], 1.0, None, True)


def test_guidance_with_video_conditioned_self_cond_unet(parity_log):
    """cond_scale = 2 with a video-conditioned self-conditioned unet: both
    guidance forwards read the same self-conditioning."""
    from dalle2_video import dalle2_video as D

    u = D.Unet3D(8, video_embed_dim=512, channels=3, dim_mults=(1, 2), cond_on_video_embeds=True, self_cond=True)
    dec = _loop_decoder(u, True, eta=0.0)
    with torch.no_grad():
        for n, p in dec.unets[0].named_parameters():  # the video projections get no deterministic fill
            if n.startswith(("video_to_tokens.", "to_video_hiddens.")):
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n))).cuda() * 0.05)
    emb = torch.randn(2, 512, generator=torch.Generator().manual_seed(5)).cuda()
    outs = []
    for cs in (2.0, 2.0, 1.0):
        torch.cuda.manual_seed(77)
        outs.append(dec.sample(video_embed=emb, cond_scale=cs))
    e = rel(outs[1], outs[0])
    parity_log(rerun_rel=e, guidance_moved=rel(outs[2], outs[0]))
    assert torch.isfinite(outs[0]).all() and e < 1e-5 and rel(outs[2], outs[0]) > 1e-4


# ---------------------------------------------------------------------------
# 8. trainer: one captured graph per pinned decision
# ---------------------------------------------------------------------------


def test_trainer_two_variants_replay_vs_eager(parity_log, monkeypatch):
    from dalle2_video import dalle2_video as D
    from dalle2_video.trainer import VideoDecoderTrainer
    from dalle2_video.utils import deterministic_fill_

    dec = D.VideoDecoder(D.Unet3D(16, channels=3, self_cond=True, **MK), frame_sizes=(32,), frame_numbers=(4,),
                         timesteps=1000, learned_variance=False)
    deterministic_fill_(dec.unets[0])
    dec = dec.cuda()
    tr = VideoDecoderTrainer(dec, lr=3e-4, wd=1e-2, use_ema=False, amp=False, use_graphs=True)
    video = torch.rand(2, 3, 4, 32, 32, generator=torch.Generator().manual_seed(1234)).cuda()
    torch.cuda.manual_seed(1)
    tr(video=video, unet_number=1)
    tr.update(1)  # builds the flat buffers (the first call is never captured)
    opt = tr.optim0
    errs, losses = {}, {}
    for variant in (False, True):
        dec.forced_self_cond = variant
        res = {}
        # A, B: the two eager warm-up calls; C captures and replays; D replays
        for tag, seed in (("A", 7), ("B", 8), ("C", 7), ("D", 8)):
            opt.zero_grad()
            torch.cuda.manual_seed(seed)
            loss = tr(video=video, unet_number=1)
            torch.cuda.synchronize()
            res[tag] = (loss, opt.flat_grad.clone())
        assert dec.forced_self_cond is variant  # a pinned decision stays pinned
        for e, r in (("A", "C"), ("B", "D")):
            errs[f"loss_{variant}_{e}{r}"] = abs(res[e][0] - res[r][0]) / abs(res[e][0])
            errs[f"grad_{variant}_{e}{r}"] = rel(res[r][1], res[e][1])
        losses[variant] = res["A"][0]
    parity_log(**errs, loss_plain=losses[False], loss_self_cond=losses[True])
    assert len(tr._graphs) == 2 and all("graph" in ent for ent in tr._graphs.values())
    assert all(v <= 1e-5 for v in errs.values()), errs
    assert abs(losses[True] - losses[False]) > 1e-5 * abs(losses[False])  # the variants are two computations
    # unpinned: the trainer draws the coin once per call on the host and un-pins it after
    dec.forced_self_cond = None
    draws = []
    monkeypatch.setattr(random, "random", lambda: draws.append(1) or 0.25)
    opt.zero_grad()
    torch.cuda.manual_seed(7)
    loss = tr(video=video, unet_number=1)
    assert draws == [1] and dec.forced_self_cond is None and len(tr._graphs) == 2
    assert abs(loss - losses[True]) <= 1e-5 * abs(losses[True])  # 0.25 < 0.5: the self-conditioned graph replayed


# ---------------------------------------------------------------------------
# 9. decoders without self_cond launch what they launched
# ---------------------------------------------------------------------------


def record_plain_step_launches():
    """{case: {"kernels": names timed by ops.TIMER, "calls": C-ABI entry points}}
    of one eager sampling step of a decoder WITHOUT self-conditioning, through
    the step object of the captured loops (cond_scale 1 and 2, DDPM and DDIM)."""
    from dalle2_video import dalle2_video as D, ops

    dec = _loop_decoder(D.Unet3D(16, channels=3, **MK), True)
    x = torch.randn(2, 3, 4, 32, 32, generator=torch.Generator().manual_seed(3)).cuda()
    out = {}
    for name, eta, cs in (("ddpm_cs1", None, 1.0), ("ddim_cs1", 1.0, 1.0), ("ddpm_cs2", None, 2.0)):
        calls, orig = [], ops.call

        def spy(fn, *a):
            calls.append(fn)
            return orig(fn, *a)

        with torch.no_grad(), ops.private_pack_cache():
            step = D._DenoiseStepGraph(dec, dec.unets[0], x.clone(), None, dec.noise_schedulers[0], cs, None, True,
                                       ddim_eta=eta)
            step(15, 11)  # warm: lazily packed weights / workspaces exist afterwards
            ops.TIMER, ops.call = ops.KernelTimer(), spy
            try:
                step(11, 7)
                torch.cuda.synchronize()
                kernels = [r[0] for r in ops.TIMER.records]
            finally:
                ops.TIMER, ops.call = None, orig
        out[name] = {"kernels": kernels, "calls": calls}
    return out


def test_plain_decoder_step_launches_are_unchanged():
    """Compared with the sequences recorded from the commit before
    self-conditioning existed (tests/golden/sample_step_launches.json)."""
    want = json.load(open(GOLDEN))
    got = record_plain_step_launches()
    assert set(got) == set(want)
    for case in want:
        assert got[case]["calls"] == want[case]["calls"], case
        assert got[case]["kernels"] == want[case]["kernels"], case
        assert not any(c.endswith("_sc") or c == "dv_unet_input" for c in got[case]["calls"])
