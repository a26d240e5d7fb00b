"""Video-embedding conditioning of Unet3D, host side: construction, state-dict
names and the cast_model_parameters flag, plus the plain-PyTorch restatements
the GPU tests (tests/test_video_cond_gpu.py) compare against.

oracle/dv_ref.py has no video-token path, so the expected values are restated
here, in whatever dtype the inputs have (float64 in the tests):
  cross_attention       dalle2-pytorch CrossAttention (8 heads x 64, learned null
                        k/v prepended, logit factor 64^-0.5, gain-only LayerNorm
                        before and after) + the residual of ResnetBlock3D, for any
                        number of context tokens
  conditioning          reference dalle2_video.py:772-809, 852-866: keep-mask
                        select of the video hiddens / tokens against the learned
                        nulls, t + hiddens, cat(time_tokens, video_tokens), the
                        two context LayerNorms
  unet_forward          the oracle Unet3D's own blocks driven with that
                        conditioning (the oracle's forward with c / mid_c of 6
                        tokens and the video term in t)
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import dv_ref as R

E = 512  # video_embed_dim of every case


# ---------------------------------------------------------------------------
# restatements
# ---------------------------------------------------------------------------
def gain_layer_norm(t, g, eps):
    return (t - t.mean(-1, keepdim=True)) * (t.var(-1, unbiased=False, keepdim=True) + eps).rsqrt() * g


def cross_attention(x_tok, ctx, g1, null_kv, wq, wkv, wo, g2, eps):
    """x_tok (b, n, C), ctx (b, m, cond_dim) -> CrossAttention(x, ctx) + x."""
    b, heads, dh = x_tok.shape[0], 8, 64
    q = gain_layer_norm(x_tok, g1, eps) @ wq.t()
    k, v = (ctx @ wkv.t()).chunk(2, dim=-1)
    split = lambda t: t.reshape(t.shape[0], t.shape[1], heads, dh).transpose(1, 2)
    q, k, v = split(q), split(k), split(v)
    k = torch.cat((null_kv[0].expand(b, heads, 1, dh), k), dim=2)
    v = torch.cat((null_kv[1].expand(b, heads, 1, dh), v), dim=2)
    sim = (q * dh ** -0.5) @ k.transpose(-1, -2)
    out = (sim.softmax(dim=-1) @ v).transpose(1, 2).reshape(b, -1, heads * dh)
    return gain_layer_norm(out @ wo.t(), g2, eps) + x_tok


def video_params(unet):
    """The conditioning parameters of a Unet3D (ours) as a dict of tensors."""
    p = dict(tok_w=unet.video_to_tokens[0].weight, tok_b=unet.video_to_tokens[0].bias,
             null_embed=unet.null_video_embed, null_hiddens=unet.null_video_hiddens)
    if unet.to_video_hiddens is not None:
        p.update(hid_w=unet.to_video_hiddens[0].weight, hid_b=unet.to_video_hiddens[0].bias)
    return p


def conditioning(t, time_tokens, video_embed, keep, vp, norm_cond, norm_mid_cond):
    """:772-809, :852-866.  keep: (b,) bool keep-mask; vp: video_params()."""
    if "hid_w" in vp:
        hid = F.gelu(video_embed @ vp["hid_w"].t() + vp["hid_b"])
        t = t + torch.where(keep[:, None], hid, vp["null_hiddens"].to(hid.dtype))
    n = vp["null_embed"].shape[1]
    tok = (video_embed @ vp["tok_w"].t() + vp["tok_b"]).reshape(video_embed.shape[0], n, -1)
    tok = torch.where(keep[:, None, None], tok, vp["null_embed"].to(tok.dtype))
    c = torch.cat((time_tokens, tok), dim=-2)
    return t, norm_cond(c), norm_mid_cond(c)


def unet_forward(ou, vp, x, time, video_embed, keep):
    """The oracle Unet3D `ou` (built without the flag: same blocks) run with
    the restated conditioning; mirrors oracle Unet3D.forward otherwise."""
    x = ou.init_conv(x)
    r = x.clone()
    th = ou.to_time_hiddens(time.type_as(x))
    t, c, mid_c = conditioning(ou.to_time_cond(th), ou.to_time_tokens(th), video_embed, keep, vp,
                               ou.norm_cond, ou.norm_mid_cond)
    hiddens = []
    for _, init_block, blocks, attn, post in ou.downs:
        x = init_block(x, t, c)
        for blk in blocks:
            x = blk(x, t, c)
            hiddens.append(x.contiguous())
        x = attn(x)
        hiddens.append(x.contiguous())
        x = post(x)
    x = ou.mid_block1(x, t, mid_c)
    x = ou.mid_attn(x)
    x = ou.mid_block2(x, t, mid_c)
    skip = lambda f: torch.cat((f, hiddens.pop() * ou.skip_connect_scale), dim=1)
    for init_block, blocks, attn, up in ou.ups:
        x = init_block(skip(x), t, c)
        for blk in blocks:
            x = blk(skip(x), t, c)
        x = up(attn(x))
    x = ou.final_resnet_block(torch.cat((x, r), dim=1), t)
    return ou.to_out(x)


def fill_(module, seed=5, scale=0.05):
    """Non-zero values for every parameter the deterministic fills leave out
    or zero (to_out, the video projections), from a seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.startswith(("to_out.", "video_to_tokens.", "to_video_hiddens.")):
                p.copy_(torch.randn(p.shape, generator=g) * scale)
    return module


def make_pair(dim=8, mults=(1, 2), add_to_time=True, dtype=torch.float64):
    """(ours on the CPU, oracle in `dtype`, video params in `dtype`) with equal
    weights: the oracle is filled deterministically, ours loads its state."""
    from dalle2_video import dalle2_video as D

    ou = R.deterministic_fill_(R.Unet3D(dim, video_embed_dim=E, channels=3, dim_mults=mults))
    u = D.Unet3D(dim, video_embed_dim=E, channels=3, dim_mults=mults, cond_on_video_embeds=True,
                 add_video_embeds_to_time=add_to_time)
    missing, unexpected = u.load_state_dict(ou.state_dict(), strict=False)
    assert not unexpected and all(k.startswith(("video_to_tokens.", "to_video_hiddens.")) for k in missing)
    fill_(u)
    with torch.no_grad():
        ou.to_out.weight.copy_(u.to_out.weight)
        ou.to_out.bias.copy_(u.to_out.bias)
    ou = ou.to(dtype)
    for m in ou.modules():  # the gain-only LayerNorms take eps 1e-3 outside float32: keep the
        if isinstance(m, R.LayerNorm):  # f32 model's 1e-5 when it is restated in float64
            m.fp16_eps = m.eps
    vp = {k: v.detach().to(dtype) for k, v in video_params(u).items()}
    return u, ou, vp


# ---------------------------------------------------------------------------
# construction
# ---------------------------------------------------------------------------
def _unet(**kw):
    from dalle2_video import dalle2_video as D

    return D.Unet3D(8, video_embed_dim=E, channels=3, dim_mults=(1, 2), **kw)


def test_flag_is_accepted_and_state_dict_names_follow_the_reference():
    off, on = _unet(), _unet(cond_on_video_embeds=True)
    assert on.cond_on_video_embeds is True
    extra = ["video_to_tokens.0.weight", "video_to_tokens.0.bias", "to_video_hiddens.0.weight",
             "to_video_hiddens.0.bias"]
    assert sorted(on.state_dict()) == sorted(list(off.state_dict()) + extra)
    sd = on.state_dict()
    assert sd["video_to_tokens.0.weight"].shape == (8 * 4, E)  # cond_dim * num_image_tokens
    assert sd["to_video_hiddens.0.weight"].shape == (8 * 4, E)  # time_cond_dim = 4 * dim
    assert sd["null_video_embed"].shape == (1, 4, 8) and sd["null_video_hiddens"].shape == (1, 32)


def test_without_add_to_time_there_are_no_video_hiddens():
    u = _unet(cond_on_video_embeds=True, add_video_embeds_to_time=False)
    assert u.to_video_hiddens is None
    assert not any(k.startswith("to_video_hiddens") for k in u.state_dict())
    assert "video_to_tokens.0.weight" in u.state_dict()


def test_flag_off_unet_is_unchanged():
    """Module tree and construction RNG draws of today's unet: the same keys as
    the oracle (which has no flag) and the same initial values from a seed."""
    torch.manual_seed(3)
    u = _unet()
    torch.manual_seed(3)
    o = R.Unet3D(8, video_embed_dim=E, channels=3, dim_mults=(1, 2))
    assert list(u.state_dict()) == list(o.state_dict())
    assert isinstance(u.video_to_tokens, torch.nn.Identity) and u.to_video_hiddens is None
    assert all(torch.equal(a, b) for a, b in zip(u.state_dict().values(), o.state_dict().values()))


def test_cast_model_parameters_keeps_the_flag():
    u = _unet(cond_on_video_embeds=True)
    kw = dict(lowres_noise_cond=False, channels=3, channels_out=3, cond_on_text_encodings=False)
    assert u.cast_model_parameters(lowres_cond=False, cond_on_image_embeds=True, **kw) is u
    v = u.cast_model_parameters(lowres_cond=True, cond_on_image_embeds=False, **kw)
    assert v is not u and v.cond_on_video_embeds is True and v.lowres_cond is True
    assert v.to_video_hiddens is not None
    off = _unet().cast_model_parameters(lowres_cond=True, cond_on_image_embeds=True, **kw)
    assert off.cond_on_video_embeds is False  # the decoder's argument is swallowed


def test_decoder_keeps_a_conditioned_unet_and_an_unconditioned_second_one():
    from dalle2_video import dalle2_video as D

    u1 = _unet(cond_on_video_embeds=True)
    u2 = D.Unet3D(8, video_embed_dim=E, channels=3, dim_mults=(1, 2))
    dec = D.VideoDecoder((u1, u2), frame_sizes=(16, 32), frame_numbers=(2, 2), timesteps=10,
                         learned_variance=False)
    assert dec.unets[0].cond_on_video_embeds is True and dec.unets[1].cond_on_video_embeds is False
    assert dec.unets[1].lowres_cond is True


def test_unsupported_token_layouts_raise_clearly():
    from dalle2_video import dalle2_video as D

    with pytest.raises(NotImplementedError, match="video tokens"):  # Identity: one token of cond_dim
        D.Unet3D(8, video_embed_dim=8, channels=3, dim_mults=(1, 2), cond_on_video_embeds=True)
    with pytest.raises(NotImplementedError, match="video tokens"):
        _unet(cond_on_video_embeds=True, num_image_tokens=3)
    with pytest.raises(ValueError, match="video_embed_dim"):
        D.Unet3D(8, channels=3, dim_mults=(1, 2), cond_on_video_embeds=True)


def test_key_count_is_derived_from_the_kv_rows():
    from dalle2_video import _lib, ops

    assert ops.xattn_keys(4, 2) == 3 and ops.xattn_keys(18, 3) == 7
    for rows, nb in ((3, 1), (8, 2), (7, 2)):
        with pytest.raises(_lib.DVError, match="3 or 7 keys"):
            ops.xattn_keys(rows, nb)


# ---------------------------------------------------------------------------
# the restatement is self-consistent
# ---------------------------------------------------------------------------
def test_restated_unet_ignores_a_dropped_embedding_and_follows_a_kept_one():
    _, ou, vp = make_pair()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 3, 2, 16, 16, generator=g, dtype=torch.float64)
    t = torch.tensor([3, 700])
    e1 = torch.randn(2, E, generator=g, dtype=torch.float64)
    e2 = torch.randn(2, E, generator=g, dtype=torch.float64)
    drop, keep = torch.zeros(2, dtype=torch.bool), torch.ones(2, dtype=torch.bool)
    with torch.no_grad():
        d1, d2 = unet_forward(ou, vp, x, t, e1, drop), unet_forward(ou, vp, x, t, e2, drop)
        k1, k2 = unet_forward(ou, vp, x, t, e1, keep), unet_forward(ou, vp, x, t, e2, keep)
        mixed = unet_forward(ou, vp, x, t, e1, torch.tensor([True, False]))
    assert torch.equal(d1, d2)  # video_cond_drop_prob = 1
    assert (k1 - k2).abs().max() > 1e-6 * k1.abs().max()  # drop probability 0
    assert (k1 - d1).abs().max() > 1e-6 * k1.abs().max()
    # samples are independent: a mixed mask picks per sample
    assert torch.allclose(mixed[0], k1[0], rtol=0, atol=1e-12) and torch.allclose(mixed[1], d1[1], rtol=0, atol=1e-12)


def test_restated_cross_attention_is_permutation_invariant_in_the_context():
    g = torch.Generator().manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, ctx = r(2, 10, 16), r(2, 6, 8)
    args = (torch.ones(16, dtype=torch.float64), r(2, 64), r(512, 16), r(1024, 8), r(16, 512),
            torch.ones(16, dtype=torch.float64), 1e-5)
    perm = torch.tensor([4, 2, 0, 5, 1, 3])
    a, b = cross_attention(x, ctx, *args), cross_attention(x, ctx[:, perm], *args)
    assert torch.allclose(a, b, rtol=0, atol=1e-12)
