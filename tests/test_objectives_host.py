"""x0 / v prediction objectives and dynamic thresholding: what needs no GPU.

The restatements below are the reference's arithmetic written out literally
in plain PyTorch (NoiseScheduler.calculate_v / predict_start_from_v /
predict_noise_from_start of dalle2-pytorch, as called at
dalle2_video.py:1585-1598, :1843-1867 and :1988-1995, and
VideoDecoder.dynamic_threshold at :1531-1549).  tests/test_objectives_gpu.py
evaluates them in float64 (the expected values) and in float32 (the error
scale of the tolerance) on the same f32 schedule tables the kernels read.
"""
import pytest
import torch


def bc(v):
    return v.reshape(-1, 1, 1, 1, 1)


def calculate_v(x_start, noise, sqrt_ac, sqrt_1m_ac):
    return sqrt_ac * noise - sqrt_1m_ac * x_start


def predict_start_from_v(x_t, v, sqrt_ac, sqrt_1m_ac):
    return sqrt_ac * x_t - sqrt_1m_ac * v


def predict_start_from_noise(x_t, noise, sqrt_recip_ac, sqrt_recipm1_ac):
    return sqrt_recip_ac * x_t - sqrt_recipm1_ac * noise


def predict_noise_from_start(x_t, x0, sqrt_recip_ac, sqrt_recipm1_ac):
    return (sqrt_recip_ac * x_t - x0) / sqrt_recipm1_ac


def dynamic_threshold(x0, percentile):
    """percentile None: the static clamp (s = 1)."""
    if percentile is None:
        return x0.clamp(-1.0, 1.0)
    s = torch.quantile(x0.flatten(1).abs(), percentile, dim=-1).clamp(min=1.0)
    s = bc(s)
    return x0.clamp(-s, s) / s


def _unet(dim=8, mults=(1, 2), **kw):
    from dalle2_video import dalle2_video as D

    return D.Unet3D(dim, video_embed_dim=512, channels=3, dim_mults=mults, **kw)


def _decoder(**kw):
    from dalle2_video import dalle2_video as D

    return D.VideoDecoder(_unet(), frame_sizes=(32,), frame_numbers=(2,), timesteps=20,
                          learned_variance=False, **kw)


def test_decoder_accepts_objectives_and_dynamic_thresholding():
    from dalle2_video import dalle2_video as D

    dec = _decoder(predict_v=True)
    assert dec.predict_v == (True,) and dec.predict_x_start == (False,)
    dec = _decoder(predict_x_start=True)
    assert dec.predict_x_start == (True,) and dec.predict_v == (False,)
    dec = _decoder(use_dynamic_thres=True, dynamic_thres_percentile=0.9)
    assert dec.use_dynamic_thres and dec.dynamic_thres_percentile == 0.9
    sr = _unet(8, (1, 2, 4, 8, 16), cond_on_text_encodings=False)
    dec = D.VideoDecoder((_unet(), sr), frame_sizes=(32, 64), frame_numbers=(2, 2), timesteps=20,
                         predict_x_start=(False, True), learned_variance=False)
    assert dec.predict_x_start == (False, True) and dec.predict_v == (False, False)


def test_latent_diffusion_flag_keeps_its_meaning():
    dec = _decoder(predict_x_start=True, predict_x_start_for_latent_diffusion=True)
    assert dec.predict_x_start == (False,)


def test_both_objective_flags_for_one_unet_raise():
    from dalle2_video import dalle2_video as D

    with pytest.raises(ValueError, match="predict_x_start and predict_v"):
        _decoder(predict_x_start=True, predict_v=True)
    sr = _unet(8, (1, 2, 4, 8, 16), cond_on_text_encodings=False)
    with pytest.raises(ValueError, match="unet 2"):
        D.VideoDecoder((_unet(), sr), frame_sizes=(32, 64), frame_numbers=(2, 2), timesteps=20,
                       predict_x_start=(False, True), predict_v=(True, True), learned_variance=False)
    # one flag each, on different unets, is a valid cascade
    D.VideoDecoder((_unet(), sr), frame_sizes=(32, 64), frame_numbers=(2, 2), timesteps=20,
                   predict_x_start=(True, False), predict_v=(False, True), learned_variance=False)


def test_learned_variance_still_raises():
    with pytest.raises(NotImplementedError):
        from dalle2_video import dalle2_video as D

        D.VideoDecoder(_unet(), frame_sizes=(32,), frame_numbers=(2,), learned_variance=True, predict_v=True)


def test_objective_names():
    from dalle2_video import ops

    assert ops.objective_name() == "eps"
    assert ops.objective_name(predict_x_start=True) == "x0"
    assert ops.objective_name(predict_v=True) == "v"
    assert ops.OBJECTIVES == {"eps": 0, "x0": 1, "v": 2}


def test_v_restatement_round_trips_in_float64():
    """x_t = sqrt(a) x0 + sqrt(1 - a) eps; v = calculate_v(x0, eps):
    predict_start_from_v(x_t, v) = x0, the implied noise
    sqrt(1 - a) x_t + sqrt(a) v = eps (the form the DDIM kernel uses), and
    predict_noise_from_start(x_t, x0) = eps."""
    from dalle2_video import dalle2_video as D

    s = D.NoiseScheduler(beta_schedule="cosine", timesteps=1000, loss_type="l2")
    g = torch.Generator().manual_seed(3)
    x0 = torch.randn(4, 3, 2, 4, 4, generator=g, dtype=torch.float64)
    eps = torch.randn(x0.shape, generator=g, dtype=torch.float64)
    t = torch.tensor([0, 3, 537, 999])
    a = bc(s.alphas_cumprod.double()[t])
    sa, s1m = a.sqrt(), (1 - a).sqrt()
    x_t = sa * x0 + s1m * eps
    v = calculate_v(x0, eps, sa, s1m)
    assert (predict_start_from_v(x_t, v, sa, s1m) - x0).abs().max() < 1e-12
    assert (s1m * x_t + sa * v - eps).abs().max() < 1e-12
    back = predict_noise_from_start(x_t, x0, (1 / a).sqrt(), (1 / a - 1).sqrt())
    assert ((back - eps).abs() / bc(1 / s1m.flatten())).max() < 1e-12  # conditioned by 1/sqrt(1 - a)


def test_dynamic_threshold_restatement():
    x = torch.tensor([[0.1, -0.2, 0.3, -0.4], [1.0, -2.0, 3.0, -4.0]], dtype=torch.float64).reshape(2, 1, 1, 2, 2)
    y = dynamic_threshold(x, 1.0)  # p = 1: the maximum magnitude
    assert torch.equal(y[0], x[0])  # s = max(1, 0.4) = 1: the static clamp
    assert torch.allclose(y[1], x[1] / 4.0)
    y = dynamic_threshold(x, 0.5)  # median of (1, 2, 3, 4) = 2.5
    assert torch.allclose(y[1], (x[1].clamp(-2.5, 2.5)) / 2.5)
    assert torch.equal(dynamic_threshold(x, None), x.clamp(-1, 1))
