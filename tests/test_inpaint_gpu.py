"""Inpainting on the GPU: the fused blend kernel (ops.inpaint_blend /
dv_inpaint_blend) on every element, the RePaint loops (eager and captured), a
real Unet3D, the cascade, and what a call without the arguments launches.

Expected values come from tests/inpaint_cases.py: the four branches restated
in float64 on the f32 tables the kernel reads.

Tolerances:
  copied elements (unmasked without renoise; masked with final)   bit-equal
  noised / renoised elements, per element                         <= 4 * 2^-24 * (|c1 a| + |c2 b|)
      out = c1 a + c2 b with (c1, a, c2, b) = (sqrt_ac[t], k, sqrt_1m_ac[t], noise) on the mask and
      (a_t/a_u, x, (s_t a_u - s_u a_t)/a_u, noise) off it.  The kernel rounds at most: k = 2 known - 1
      (one rounding of a), c1 and c2 to f32 (one each; they are formed in double from the f32 table
      entries), c2 b, and the final fused multiply-add -- never more than 3 roundings on either term's
      path, each relative 2^-24 to that term or to the sum, which |c1 a| + |c2 b| bounds.  4 leaves room
      for the second-order terms.  No fitted constant.
  loops with the elementwise denoiser                             bit-equal (graph vs eager, known region)
  Unet3D, graph replay vs eager                                   rel < 1e-5 (the bar of test_ddim_gpu.py)
"""
import functools

import pytest
import torch

import inpaint_cases as IC

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NT = 1000


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def _sched(timesteps=NT):
    from dalle2_video import dalle2_video as D

    return D.NoiseScheduler(beta_schedule="cosine", timesteps=timesteps, loss_type="l2").cuda()


def _tables(s):
    return s.sqrt_alphas_cumprod.cpu(), s.sqrt_one_minus_alphas_cumprod.cpu()


# ---------------------------------------------------------------------------
# 1. the kernel, every element
# ---------------------------------------------------------------------------
SHAPES = {"scalar_5x7": (2, 3, 3, 5, 7), "vector_8x8": (2, 3, 3, 8, 8)}
MASKS = ("all_true", "all_false", "checkerboard", "frame0")


def _mask(kind, shape):
    B, _, T, H, W = shape
    m = torch.zeros(B, T, H, W, dtype=torch.uint8)
    if kind == "all_true":
        m[:] = 1
    elif kind == "checkerboard":  # per pixel, shifted per frame and sample: bits differ inside a 4-wide vector
        b, t, y, x = torch.meshgrid(torch.arange(B), torch.arange(T), torch.arange(H), torch.arange(W), indexing="ij")
        m = ((b + t + y + x) % 2).to(torch.uint8) * 255  # any nonzero byte is "known"
    elif kind == "frame0":
        m[:, 0] = 1
    return m


@functools.lru_cache(maxsize=None)
def _kernel_inputs(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g)
    known = torch.rand(shape, generator=g)
    noise = torch.randn(shape, generator=g)
    return x, known, noise


def _run(x, known, mask, noise, t, t_from, normalize=False, final=False, sched=None):
    from dalle2_video import ops

    dev = lambda v: None if v is None else v.cuda()
    xd = x.cuda().clone()
    before = xd.data_ptr()
    out = ops.inpaint_blend(xd, dev(known), dev(mask), dev(noise), dev(t), sched or _sched(), times_from=dev(t_from),
                            normalize=normalize, final=final)
    torch.cuda.synchronize()
    assert out is xd and xd.data_ptr() == before  # in place: nothing new is returned
    return xd.cpu()


def _check(got, x, known, mask, noise, t, t_from, normalize, final=False):
    """Per element: copied elements to the bit, the others inside the derived bound."""
    want, c1a, c2b = IC.blend_restatement(x, known, mask, noise, t, t_from, *_tables(_sched()), normalize=normalize,
                                          final=final)
    m = IC.bc_mask(mask, x)
    copied = ~m if t_from is None else torch.zeros_like(m)
    assert torch.equal(got[copied], x[copied])  # untouched: the input's bits
    if final:
        k32 = 2 * known - 1 if normalize else known  # f32: one rounding
        assert torch.equal(got[m], k32[m])
        return 0.0
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan)
    live = ~copied & ~nan
    err = (got.double() - want)[live].abs()
    tol = 4 * U * (c1a + c2b)[live]
    assert (err <= tol).all(), (err / tol.clamp_min(1e-300)).max().item()
    return (err / tol.clamp_min(1e-300)).max().item() if err.numel() else 0.0


@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_blend_kernel_every_element(parity_log, shape_name, mask_kind):
    shape = SHAPES[shape_name]
    x, known, noise = _kernel_inputs(shape)
    mask = _mask(mask_kind, shape)
    t, t_from = torch.tensor([537, 1]), torch.tensor([500, 0])  # a different t per sample
    worst = {}
    for normalize in (False, True):
        got = _run(x, known, mask, None, None, None, normalize=normalize, final=True)
        _check(got, x, known, mask, None, None, None, normalize, final=True)
        got = _run(x, known, mask, noise, t, None, normalize=normalize)
        worst[f"blend_n{int(normalize)}"] = _check(got, x, known, mask, noise, t, None, normalize)
        got = _run(x, known, mask, noise, t, t_from, normalize=normalize)
        worst[f"renoise_n{int(normalize)}"] = _check(got, x, known, mask, noise, t, t_from, normalize)
    # neighbouring steps, where s_t a_u - s_u a_t cancels most
    t2, u2 = torch.tensor([999, 500]), torch.tensor([998, 499])
    got = _run(x, known, mask, noise, t2, u2, normalize=True)
    worst["renoise_adjacent"] = _check(got, x, known, mask, noise, t2, u2, True)
    parity_log(shape=shape_name, mask=mask_kind, worst_err_over_bound=worst)


@pytest.mark.parametrize("shape_name", list(SHAPES))
@pytest.mark.parametrize("bad", ["t_eq_nt", "t_neg", "from_eq_t", "from_gt_t"])
def test_blend_kernel_bad_times_mark_that_sample_only(shape_name, bad):
    shape = SHAPES[shape_name]
    x, known, noise = _kernel_inputs(shape)
    mask = _mask("checkerboard", shape)
    t = torch.tensor([{"t_eq_nt": NT, "t_neg": -1}.get(bad, 537), 5])
    t_from = {"from_eq_t": torch.tensor([537, 3]), "from_gt_t": torch.tensor([600, 3])}.get(bad)
    got = _run(x, known, mask, noise, t, t_from, normalize=True)
    m = IC.bc_mask(mask, x)
    written = m if t_from is None else torch.ones_like(m)
    assert got[0][written[0]].isnan().all()  # exactly the written elements of the bad sample
    assert torch.equal(got[0][~written[0]], x[0][~written[0]])
    assert not got[1].isnan().any()
    _check(got, x, known, mask, noise, t, t_from, True)  # and sample 1 is correct


def test_blend_wrapper_rejects_mismatches():
    from dalle2_video import _lib, ops

    s = _sched()
    x = torch.zeros(2, 3, 3, 8, 8, device="cuda")
    mask = torch.zeros(2, 3, 8, 8, dtype=torch.uint8, device="cuda")
    t = torch.zeros(2, dtype=torch.long, device="cuda")
    ok = dict(x=x, known=x.clone(), mask=mask, noise=x.clone(), times=t, sched=s)
    for change in (dict(mask=mask.bool()), dict(mask=mask[:, :2]), dict(known=x[:, :2]), dict(noise=None),
                   dict(noise=x.double()), dict(times=t[:1]), dict(times=t.int()), dict(x=x.transpose(3, 4)),
                   dict(x=x.cpu()), dict(times_from=t[:1])):
        with pytest.raises(_lib.DVError):
            ops.inpaint_blend(**{**ok, **change})
    with pytest.raises(_lib.DVError):
        ops.inpaint_blend(x, x.clone(), mask, None, None, s, times_from=t, final=True)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 2. the loops, with a bit-reproducible denoiser
# ---------------------------------------------------------------------------
class _ElementwiseDenoiser(torch.nn.Module):
    """The stand-in of test_ddim_gpu.py: eps is an elementwise function of
    (x, t), reproducible to the bit (Unet3D's GroupNorm statistics are float
    atomic sums and are not).  Counts its eager calls."""

    lowres_cond = False

    def __init__(self):
        super().__init__()
        self.calls = 0
        self.anchor = torch.nn.Parameter(torch.zeros(1))  # a decoder holding only this denoiser has a device

    def forward_with_cond_scale(self, x, t, video_embed=None, cond_scale=1.0, lowres_cond_video=None):
        self.calls += 1
        return 0.5 * torch.tanh(x) + 0.01 * t.reshape(-1, 1, 1, 1, 1).float()


LOOP_SHAPE = (2, 3, 4, 32, 32)


def _loop_decoder(eta=0.0, unet=None, **kw):
    from dalle2_video import dalle2_video as D
    from dalle2_video.utils import deterministic_fill_

    u = unet or D.Unet3D(16, video_embed_dim=512, channels=3, dim_mults=(1, 2, 4, 8))
    args = dict(frame_sizes=(32,), frame_numbers=(4,), timesteps=20, sample_timesteps=6, ddim_sampling_eta=eta,
                learned_variance=False)
    args.update(kw)
    dec = D.VideoDecoder(u, **args)
    deterministic_fill_(dec.unets[0])
    return dec.cuda().eval()


@functools.lru_cache(maxsize=None)
def _known_pair(shape=LOOP_SHAPE):
    """A known clip whose values are multiples of 2^-8 in [0, 1] (2 k - 1 and
    the un-normalisation are then exact) and the mask "first two frames known"."""
    g = torch.Generator().manual_seed(21)
    video = torch.randint(0, 257, shape, generator=g).float() / 256
    mask = torch.zeros(shape[0], *shape[2:], dtype=torch.bool)
    mask[:, :2] = True
    return video.cuda(), mask.cuda()


class _CallSpy:
    """Counts dv_inpaint_blend among the C-ABI calls ops makes."""

    def __init__(self, monkeypatch):
        from dalle2_video import ops

        self.blends, self.renoises, self.names = 0, 0, []
        orig = ops.call

        def spy(fn, *a):
            self.names.append(fn)
            if fn == "dv_inpaint_blend":
                self.blends += 1
                self.renoises += a[5] is not None  # the t_from pointer
            return orig(fn, *a)

        monkeypatch.setattr(ops, "call", spy)


@pytest.mark.parametrize("resample_times", [1, 3])
@pytest.mark.parametrize("sampler", ["ddpm", "ddim_eta0", "ddim_eta1"])
def test_loop_keeps_the_known_region_and_replays_to_the_bit(monkeypatch, sampler, resample_times):
    dec = _loop_decoder(eta=1.0 if sampler == "ddim_eta1" else 0.0)
    video, mask = _known_pair()
    steps = 20 if sampler == "ddpm" else 6
    kw = dict(video_embed=None, noise_scheduler=dec.noise_schedulers[0], cond_scale=2.0, inpaint_video=video,
              inpaint_mask=mask, inpaint_resample_times=resample_times)
    outs = []
    for graphs in (False, True):
        dec.sample_graphs = graphs
        den = _ElementwiseDenoiser()
        spy = _CallSpy(monkeypatch) if not graphs else None
        torch.cuda.manual_seed(9)
        if sampler == "ddpm":
            outs.append(dec.p_sample_loop_ddpm(den, LOOP_SHAPE, **kw))
        else:
            outs.append(dec.p_sample_loop_ddim(den, LOOP_SHAPE, timesteps=6, **kw))
        torch.cuda.synchronize()
        if not graphs:
            monkeypatch.undo()
            assert den.calls == steps * resample_times
            assert spy.blends == steps * resample_times + 1
            assert spy.renoises == (steps - 1) * (resample_times - 1)
    eager, graph = outs
    m = mask[:, None].expand(-1, 3, -1, -1, -1)
    assert torch.equal(eager[m], video[m])  # the known region, to the bit
    assert torch.isfinite(eager).all()
    assert not torch.equal(eager[~m], video[~m])
    assert torch.equal(eager, graph)


@pytest.mark.parametrize("sampler,resample_times", [("ddim_eta1", 3), ("ddpm", 2)])
def test_eager_loop_matches_the_float64_restatement(parity_log, sampler, resample_times):
    """The whole loop against inpaint_cases.repaint_loop in float64: the same
    elementwise denoiser, the run's own draws regenerated from the seed (per
    pass the blend's, then the update's), the update restated from the schedule
    tables.  A blend at the wrong time, a renoise from the wrong level or a
    pass out of order moves the unknown region by far more than rounding.

    Bound, norm-wise relative over the clip: 1e-4, the f32 forward-parity bar of
    this suite.  Reasoning: a pass is ~10 f32 operations on O(1) values (2^-24 =
    6e-8 each), scaled by sqrt(1/ac[t]) where x0 is formed: on this 20-step
    cosine schedule that factor is 1.0 ... 12.9 for t <= 18, mean 2.6, and 406
    at t = 19, where all but ~0.2 % of the elements are clamped to +-1 exactly
    (their error vanishes; the rest weigh sqrt(0.002) * 406 * 10 * 6e-8 ~ 1e-5
    in the norm).  The clamp, the tanh denoiser and the updates do not expand an
    error carried from pass to pass, so the injected errors add: at most 40
    passes * 10 * 6e-8 * 2.6 = 6e-5 if all had one sign."""
    import test_ddim_gpu as TD
    from dalle2_video import dalle2_video as D

    dec = _loop_decoder(eta=1.0)
    dec.sample_graphs = False
    sched = dec.noise_schedulers[0]
    video, mask = _known_pair()
    ddim = sampler != "ddpm"
    pairs = D.ddim_time_pairs(20, 6) if ddim else [(t, t - 1) for t in reversed(range(20))]
    kw = dict(video_embed=None, noise_scheduler=sched, cond_scale=2.0, inpaint_video=video, inpaint_mask=mask,
              inpaint_resample_times=resample_times)
    den = _ElementwiseDenoiser()
    torch.cuda.manual_seed(12)
    got = (dec.p_sample_loop_ddim(den, LOOP_SHAPE, timesteps=6, **kw) if ddim
           else dec.p_sample_loop_ddpm(den, LOOP_SHAPE, **kw))
    torch.cuda.manual_seed(12)  # the same draws, in the loop's order
    start = torch.randn(LOOP_SHAPE, device="cuda").cpu()
    zb, zu = [], []
    for _ in range(len(pairs) * resample_times):
        zb.append(torch.randn(LOOP_SHAPE, device="cuda").cpu())
        zu.append(torch.randn(LOOP_SHAPE, device="cuda").cpu())
    b = LOOP_SHAPE[0]
    tab = lambda name, t: getattr(sched, name).cpu().double()[t]

    def update(x, t, tn, i):
        eps = 0.5 * torch.tanh(x) + 0.01 * t
        if ddim:
            return TD.ddim_restatement(x, eps, zu[i], torch.full((b,), t), torch.full((b,), tn),
                                       sched.alphas_cumprod, 1.0, True, torch.float64)[0]
        x0 = (tab("sqrt_recip_alphas_cumprod", t) * x - tab("sqrt_recipm1_alphas_cumprod", t) * eps).clamp(-1.0, 1.0)
        mean = tab("posterior_mean_coef1", t) * x0 + tab("posterior_mean_coef2", t) * x
        return mean if t == 0 else mean + (0.5 * tab("posterior_log_variance_clipped", t)).exp() * zu[i].double()

    want = IC.repaint_loop(update, start, video.cpu(), mask.cpu(), pairs, resample_times, zb, *_tables(sched))
    e = rel(got, (want + 1) * 0.5)
    parity_log(sampler=sampler, resample_times=resample_times, loop_vs_float64_rel=e)
    assert e <= 1e-4


# ---------------------------------------------------------------------------
# 3. a real Unet3D
# ---------------------------------------------------------------------------
def test_unet3d_inpainting_graph_matches_eager(parity_log):
    dec = _loop_decoder(eta=1.0)
    video, mask = _known_pair()
    outs = []
    for graphs in (False, True):
        dec.sample_graphs = graphs
        torch.cuda.manual_seed(77)
        outs.append(dec.sample(video_embed=torch.zeros(2, 512, device="cuda"), inpaint_video=video,
                               inpaint_mask=mask, inpaint_resample_times=2))
    eager, graph = outs
    m = mask[:, None].expand(-1, 3, -1, -1, -1)
    for o in outs:
        assert o.shape == LOOP_SHAPE and torch.isfinite(o).all()
        assert torch.equal(o[m], video[m])
    e = rel(graph, eager)
    parity_log(graph_vs_eager_rel=e)
    assert e < 1e-5


def test_unet3d_video_embedding_guidance_with_inpainting():
    from dalle2_video import dalle2_video as D

    torch.manual_seed(1)
    u = D.Unet3D(16, video_embed_dim=512, channels=3, dim_mults=(1, 2, 4, 8), cond_on_video_embeds=True)
    dec = _loop_decoder(eta=1.0, unet=u)
    assert dec.unets[0].cond_on_video_embeds is True
    video, mask = _known_pair()
    emb = torch.randn(2, 512, generator=torch.Generator().manual_seed(5)).cuda()
    video, _ = _known_pair()
    left = torch.zeros(2, 32, 32, dtype=torch.bool, device="cuda")  # a (b, h, w) mask: the left half of every frame
    left[:, :, :16] = True
    torch.cuda.manual_seed(78)
    out = dec.sample(video_embed=emb, cond_scale=2.0, inpaint_video=video, inpaint_mask=left,
                     inpaint_resample_times=2)
    assert out.shape == LOOP_SHAPE and torch.isfinite(out).all()
    assert torch.equal(out[..., :16], video[..., :16])
    assert not torch.equal(out[..., 16:], video[..., 16:])


# ---------------------------------------------------------------------------
# 4. the cascade
# ---------------------------------------------------------------------------
def test_cascade_resizes_the_pair_for_every_unet(monkeypatch):
    from dalle2_video import dalle2_video as D
    from dalle2_video import ops

    base = D.Unet3D(8, video_embed_dim=512, channels=3, dim_mults=(1, 2))
    sr = D.Unet3D(8, video_embed_dim=512, channels=3, dim_mults=(1, 2, 4, 8, 16), cond_on_text_encodings=False)
    dec = D.VideoDecoder((base, sr), frame_sizes=(32, 64), frame_numbers=(2, 2), timesteps=12,
                         sample_timesteps=(4, 4), beta_schedule=("cosine", "cosine"), learned_variance=False).cuda()
    dec.sample_graphs = False
    g = torch.Generator().manual_seed(31)
    video = (torch.randint(0, 257, (1, 3, 2, 64, 64), generator=g).float() / 256).cuda()
    mask = (torch.rand(1, 2, 64, 64, generator=g) < 0.5).cuda()
    seen = []
    blend = ops.inpaint_blend

    def spy(x, known, m, *a, **kw):
        seen.append((known.clone(), m.clone()))
        return blend(x, known, m, *a, **kw)

    monkeypatch.setattr(ops, "inpaint_blend", spy)
    torch.cuda.manual_seed(3)
    out = dec.sample(video_embed=torch.zeros(1, 512, device="cuda"), inpaint_video=video, inpaint_mask=mask,
                     inpaint_resample_times=1)
    assert out.shape == (1, 3, 2, 64, 64) and torch.isfinite(out).all()
    m = mask[:, None].expand(-1, 3, -1, -1, -1)
    assert torch.equal(out[m], video[m])  # exact at the final resolution
    assert len(seen) == 2 * (4 + 1)
    src = torch.arange(32, device="cuda") * 2  # floor(o * 64 / 32)
    for known, mk in seen[:5]:  # unet 1: the nearest-resized pair
        assert torch.equal(known, video[..., src, :][..., src])
        assert mk.dtype == torch.uint8 and torch.equal(mk.bool(), mask[..., src, :][..., src])
    for known, mk in seen[5:]:
        assert torch.equal(known, video) and torch.equal(mk.bool(), mask)


# ---------------------------------------------------------------------------
# 5. nothing changes without the arguments; the trainer forwards them
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("ddim", [False, True])
def test_sampling_without_inpainting_is_what_it_was(monkeypatch, ddim, graphs):
    dec = _loop_decoder(eta=1.0, **({} if ddim else dict(timesteps=8, sample_timesteps=None)))
    dec.sample_graphs = graphs
    den = _ElementwiseDenoiser().cuda()
    dec.unets[0] = den  # sample() hands the loop this denoiser
    spy = _CallSpy(monkeypatch)
    torch.cuda.manual_seed(4)
    a = dec.sample(video_embed=torch.zeros(2, 512, device="cuda"), cond_scale=2.0, one_unet_in_gpu_at_time=False)
    monkeypatch.undo()
    assert spy.blends == 0 and "dv_inpaint_blend" not in spy.names
    torch.cuda.manual_seed(4)
    kw = dict(video_embed=None, noise_scheduler=dec.noise_schedulers[0], cond_scale=2.0)
    b = (dec.p_sample_loop_ddim(den, LOOP_SHAPE, timesteps=6, **kw) if ddim
         else dec.p_sample_loop_ddpm(den, LOOP_SHAPE, **kw))
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_trainer_sample_forwards_the_inpainting_arguments(monkeypatch):
    from dalle2_video.trainer import VideoDecoderTrainer

    dec = _loop_decoder()
    tr = VideoDecoderTrainer(dec, lr=3e-4, wd=1e-2, use_ema=False)
    video, mask = _known_pair()
    got = {}

    def fake_sample(*a, **kw):
        got.update(kw)
        return torch.zeros(1)

    monkeypatch.setattr(dec, "sample", fake_sample)
    tr.sample(video_embed=torch.zeros(2, 512), inpaint_video=video.cpu(), inpaint_mask=mask.cpu(),
              inpaint_resample_times=3)
    assert got["inpaint_resample_times"] == 3
    assert got["inpaint_video"].is_cuda and torch.equal(got["inpaint_video"], video)
    assert got["inpaint_mask"].is_cuda and got["inpaint_mask"].dtype == torch.bool and torch.equal(got["inpaint_mask"], mask)
