"""Inpainting in VideoDecoder.sample() (RePaint, arXiv 2201.09865): what needs
no GPU.  The float64 restatement's defining properties, the argument checks of
sample(), the mask expansion and its nearest resize, and the pass schedule.
"""
import pytest
import torch

import inpaint_cases as IC


def _sched(timesteps=20):
    from dalle2_video import dalle2_video as D

    return D.NoiseScheduler(beta_schedule="cosine", timesteps=timesteps, loss_type="l2")


def _inputs(seed=0, shape=(2, 3, 3, 4, 6)):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    known = torch.rand(shape, generator=g, dtype=torch.float64)
    noise = torch.randn(shape, generator=g, dtype=torch.float64)
    return x, known, noise


# ---- the restatement ---------------------------------------------------------


def test_restatement_all_false_mask_without_renoise_is_identity():
    s = _sched()
    x, known, noise = _inputs()
    mask = torch.zeros(2, 3, 4, 6, dtype=torch.bool)
    out, c1a, c2b = IC.blend_restatement(x, known, mask, noise, torch.tensor([3, 17]), None,
                                         s.sqrt_alphas_cumprod, s.sqrt_one_minus_alphas_cumprod, normalize=True)
    assert torch.equal(out, x) and not c1a.any() and not c2b.any()
    # ... whatever the times are: nothing is written, so nothing turns NaN
    out, _, _ = IC.blend_restatement(x, known, mask, noise, torch.tensor([-1, 20]), None,
                                     s.sqrt_alphas_cumprod, s.sqrt_one_minus_alphas_cumprod)
    assert torch.equal(out, x)


@pytest.mark.parametrize("normalize", [False, True])
def test_restatement_all_true_mask_final_returns_k(normalize):
    s = _sched()
    x, known, _ = _inputs()
    mask = torch.ones(2, 3, 4, 6, dtype=torch.uint8)
    out, _, _ = IC.blend_restatement(x, known, mask, None, None, None, s.sqrt_alphas_cumprod,
                                     s.sqrt_one_minus_alphas_cumprod, normalize=normalize, final=True)
    assert torch.equal(out, 2 * known - 1 if normalize else known)


def test_restatement_renoise_moves_a_q_sample_along_the_schedule():
    """q_sample_from_to's defining identity: the renoise u -> t of
    a_u x0 + s_u e, drawn with the same e, is a_t x0 + s_t e (float64)."""
    s = _sched(1000)
    a, sg = s.sqrt_alphas_cumprod.double(), s.sqrt_one_minus_alphas_cumprod.double()
    x0, _, e = _inputs(1)
    u, t = torch.tensor([0, 499]), torch.tensor([1, 537])
    xu = IC.bc(a[u]) * x0 + IC.bc(sg[u]) * e
    mask = torch.zeros(2, 3, 4, 6, dtype=torch.bool)
    out, _, _ = IC.blend_restatement(xu, x0, mask, e, t, u, a, sg)
    want = IC.bc(a[t]) * x0 + IC.bc(sg[t]) * e
    assert (out - want).abs().max() <= 1e-13 * want.abs().max()


def test_restatement_bad_times_mark_only_the_written_elements_of_that_sample():
    s = _sched()
    x, known, noise = _inputs()
    mask = torch.zeros(2, 3, 4, 6, dtype=torch.bool)
    mask[:, 0] = True
    tabs = (s.sqrt_alphas_cumprod, s.sqrt_one_minus_alphas_cumprod)
    out, _, _ = IC.blend_restatement(x, known, mask, noise, torch.tensor([20, 5]), None, *tabs)
    assert out[0, :, 0].isnan().all() and torch.equal(out[0, :, 1:], x[0, :, 1:]) and not out[1].isnan().any()
    out, _, _ = IC.blend_restatement(x, known, mask, noise, torch.tensor([5, 5]), torch.tensor([4, 5]), *tabs)
    assert out[1].isnan().all() and not out[0].isnan().any()


def test_restatement_pass_schedule_matches_the_decoder():
    from dalle2_video import dalle2_video as D

    pairs = D.ddim_time_pairs(20, 6)
    for r in (1, 3):
        ours = list(D.inpaint_passes(pairs, r))
        theirs = IC.inpaint_passes(pairs, r)
        assert len(ours) == len(theirs) == len(pairs) * r
        # a pass carries time_from exactly when a renoise followed the pass before it
        want_from = [None] + [tn if after else None for _, tn, after in theirs[:-1]]
        assert [p[2] for p in ours] == want_from
        assert [p[:2] for p in ours] == [p[:2] for p in theirs]
        assert sum(p[2] is not None for p in ours) == (len(pairs) - 1) * (r - 1)
        assert all(tf is None or tf < t for t, _, tf in ours)


# ---- sample(): validation and preparation ------------------------------------


def _decoder(self_cond=False, frames=4):
    from dalle2_video import dalle2_video as D

    u = D.Unet3D(8, video_embed_dim=512, channels=3, dim_mults=(1, 2), self_cond=self_cond)
    return D.VideoDecoder(u, frame_sizes=(32,), frame_numbers=(frames,), timesteps=20, sample_timesteps=6,
                          learned_variance=False)


def _pair(b=2, f=4, s=32):
    return torch.rand(b, 3, f, s, s), torch.zeros(b, f, s, s, dtype=torch.bool)


def test_prepare_needs_no_gpu_and_expands_the_mask():
    dec = _decoder()
    assert dec._prepare_inpaint(None, None) is None
    video, mask = _pair()
    v, m = dec._prepare_inpaint(video, mask, 5, batch_size=2)
    assert v.dtype == torch.float32 and torch.equal(v, video) and m.dtype == torch.bool and m.shape == (2, 4, 32, 32)
    m3 = torch.rand(2, 32, 32) < 0.5
    v, m = dec._prepare_inpaint(video, m3, 1, batch_size=2)
    assert m.shape == (2, 4, 32, 32) and all(torch.equal(m[:, f], m3) for f in range(4))


def test_sample_rejects_bad_inpaint_arguments():
    dec = _decoder()
    video, mask = _pair()
    emb = torch.zeros(2, 512)
    with pytest.raises(ValueError, match="together"):
        dec.sample(video_embed=emb, inpaint_video=video)
    with pytest.raises(ValueError, match="together"):
        dec.sample(video_embed=emb, inpaint_mask=mask)
    with pytest.raises(ValueError, match="batch"):
        dec.sample(video_embed=torch.zeros(3, 512), inpaint_video=video, inpaint_mask=mask)
    with pytest.raises(ValueError, match="frames"):
        v5, m5 = _pair(f=5)
        dec.sample(video_embed=emb, inpaint_video=v5, inpaint_mask=m5)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="inpaint_resample_times"):
            dec.sample(video_embed=emb, inpaint_video=video, inpaint_mask=mask, inpaint_resample_times=bad)
    with pytest.raises(ValueError, match="inpaint_mask"):
        dec.sample(video_embed=emb, inpaint_video=video, inpaint_mask=mask[:, :, :16])
    with pytest.raises(ValueError, match="bool"):
        dec.sample(video_embed=emb, inpaint_video=video, inpaint_mask=mask.float())
    with pytest.raises(NotImplementedError, match="self-conditioned"):
        _decoder(self_cond=True).sample(video_embed=emb, inpaint_video=video, inpaint_mask=mask)


def test_sample_rejects_non_square_frames_and_fractional_pass_counts():
    dec = _decoder()
    emb = torch.zeros(2, 512)
    video, mask = torch.rand(2, 3, 4, 32, 48), torch.zeros(2, 4, 32, 48, dtype=torch.bool)
    with pytest.raises(ValueError, match="square"):
        dec.sample(video_embed=emb, inpaint_video=video, inpaint_mask=mask)
    video, mask = _pair()
    kw = dict(video_embed=None, noise_scheduler=dec.noise_schedulers[0], inpaint_video=video, inpaint_mask=mask)
    for call in (lambda: dec.sample(video_embed=emb, inpaint_video=video, inpaint_mask=mask,
                                    inpaint_resample_times=2.5),
                 lambda: dec.p_sample_loop_ddpm(dec.unets[0], (2, 3, 4, 32, 32), inpaint_resample_times=2.5, **kw),
                 lambda: dec.p_sample_loop_ddim(dec.unets[0], (2, 3, 4, 32, 32), timesteps=6,
                                                inpaint_resample_times=0, **kw)):
        with pytest.raises(ValueError, match="inpaint_resample_times"):
            call()


def test_loops_reject_a_pair_at_another_resolution():
    dec = _decoder()
    video, mask = _pair(s=64)
    kw = dict(video_embed=None, noise_scheduler=dec.noise_schedulers[0], inpaint_video=video, inpaint_mask=mask)
    with pytest.raises(ValueError, match="do not match"):
        dec.p_sample_loop_ddpm(dec.unets[0], (2, 3, 4, 32, 32), **kw)
    with pytest.raises(ValueError, match="do not match"):
        dec.p_sample_loop_ddim(dec.unets[0], (2, 3, 4, 32, 32), timesteps=6, **kw)


# ---- the mask's nearest resize -------------------------------------------------


@pytest.mark.parametrize("n_in,n_out", [(64, 32), (32, 64), (64, 64)])
def test_mask_resize_keeps_the_nearest_index_rule(n_in, n_out):
    from dalle2_video import dalle2_video as D

    g = torch.Generator().manual_seed(n_in + n_out)
    mask = torch.rand(2, 3, n_in, n_in, generator=g) < 0.5
    out = D.resize_mask_nearest(mask, n_out)
    assert out.dtype == torch.bool and out.shape == (2, 3, n_out, n_out)
    src = [(o * n_in) // n_out for o in range(n_out)]  # floor(o * in / out)
    want = mask[:, :, src][:, :, :, src]
    assert torch.equal(out, want)
    # the rule F.interpolate(mode="nearest") applies to the clip itself
    ref = torch.nn.functional.interpolate(mask.float(), size=(n_out, n_out), mode="nearest").bool()
    assert torch.equal(out, ref)


def test_nearest_index_matches_interpolate_for_odd_ratios():
    from dalle2_video import dalle2_video as D

    for n_in, n_out in ((7, 5), (5, 7), (48, 20), (20, 48), (3, 64)):
        ramp = torch.arange(n_in, dtype=torch.float32).reshape(1, 1, 1, n_in)
        want = torch.nn.functional.interpolate(ramp, size=(1, n_out), mode="nearest").reshape(-1).long()
        assert torch.equal(D._nearest_index(n_in, n_out), want), (n_in, n_out)


# ---- the captured step keeps its positional signature --------------------------


def test_step_graph_inpaint_inputs_are_keyword_only():
    import inspect

    from dalle2_video import dalle2_video as D

    params = inspect.signature(D._DenoiseStepGraph.__init__).parameters
    names = list(params)
    assert names[:12] == ["self", "decoder", "unet", "x", "video_embed", "noise_scheduler", "cond_scale",
                          "lowres_cond_vid", "clip_denoised", "ddim_eta", "objective", "dyn_percentile"]
    for n in ("inpaint_known", "inpaint_mask", "inpaint_normalize"):
        assert params[n].kind is inspect.Parameter.KEYWORD_ONLY


_REQ = "required"
_SAMPLING_SIGNATURES = {  # the callers' contract: parameter names, order and defaults
    "p_sample": [
        ("self", _REQ), ("unet", _REQ), ("x", _REQ), ("t", _REQ), ("video_embed", _REQ), ("noise_scheduler", _REQ),
        ("text_encodings", None), ("cond_scale", 1.0), ("lowres_cond_vid", None), ("self_cond", None),
        ("predict_x_start", False), ("predict_v", False), ("learned_variance", False), ("clip_denoised", True),
        ("lowres_noise_level", None), ("noise", None)],
    "p_sample_ddim": [
        ("self", _REQ), ("unet", _REQ), ("x", _REQ), ("t", _REQ), ("t_next", _REQ), ("video_embed", _REQ),
        ("noise_scheduler", _REQ), ("eta", _REQ), ("cond_scale", 1.0), ("lowres_cond_vid", None),
        ("clip_denoised", True), ("noise", None), ("predict_x_start", False), ("predict_v", False),
        ("self_cond", None)],
    "p_sample_loop_ddpm": [
        ("self", _REQ), ("unet", _REQ), ("shape", _REQ), ("video_embed", _REQ), ("noise_scheduler", _REQ),
        ("predict_x_start", False), ("predict_v", False), ("learned_variance", False), ("clip_denoised", True),
        ("lowres_cond_vid", None), ("text_encodings", None), ("cond_scale", 1), ("is_latent_diffusion", False),
        ("lowres_noise_level", None), ("inpaint_video", None), ("inpaint_mask", None),
        ("inpaint_resample_times", 5)],
    "p_sample_loop_ddim": [
        ("self", _REQ), ("unet", _REQ), ("shape", _REQ), ("video_embed", _REQ), ("noise_scheduler", _REQ),
        ("timesteps", _REQ), ("eta", 1.0), ("predict_x_start", False), ("predict_v", False),
        ("learned_variance", False), ("clip_denoised", True), ("lowres_cond_vid", None), ("text_encodings", None),
        ("cond_scale", 1), ("is_latent_diffusion", False), ("lowres_noise_level", None), ("init_noise", None),
        ("inpaint_video", None), ("inpaint_mask", None), ("inpaint_resample_times", 5)],
    "_DenoiseStepGraph.__init__": [
        ("self", _REQ), ("decoder", _REQ), ("unet", _REQ), ("x", _REQ), ("video_embed", _REQ),
        ("noise_scheduler", _REQ), ("cond_scale", _REQ), ("lowres_cond_vid", _REQ), ("clip_denoised", _REQ),
        ("ddim_eta", None), ("objective", "eps"), ("dyn_percentile", None), ("inpaint_known", None),
        ("inpaint_mask", None), ("inpaint_normalize", False)],
}


@pytest.mark.parametrize("name", sorted(_SAMPLING_SIGNATURES))
def test_sampling_entry_points_keep_their_signatures(name):
    import inspect

    from dalle2_video import dalle2_video as D

    fn = D._DenoiseStepGraph.__init__ if name.startswith("_Denoise") else getattr(D.VideoDecoder, name)
    params = inspect.signature(fn).parameters.values()
    got = [(p.name, _REQ if p.default is inspect.Parameter.empty else p.default) for p in params]
    assert got == _SAMPLING_SIGNATURES[name]
    # equal defaults of another type (1 == 1.0 == True) are not the same default
    assert [type(d) for _, d in got] == [type(d) for _, d in _SAMPLING_SIGNATURES[name]]
    kinds = {p.name: p.kind for p in params}
    keyword_only = {"inpaint_known", "inpaint_mask", "inpaint_normalize"} if name.startswith("_Denoise") else set()
    assert {n for n, k in kinds.items() if k is inspect.Parameter.KEYWORD_ONLY} == keyword_only
    assert all(k is inspect.Parameter.POSITIONAL_OR_KEYWORD for n, k in kinds.items() if n not in keyword_only)


def test_abi_is_9_and_declares_the_blend():
    from dalle2_video import _lib

    assert "dv_inpaint_blend" in _lib._SIGS
    assert _lib.lib().dv_abi_version() == 9
