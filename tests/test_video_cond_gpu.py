"""Video-embedding conditioning on the GPU: the 7-key folded cross attention
(null key + 2 time tokens + 4 video tokens), a conditioned Unet3D, and the
decoder / trainer paths that carry the embedding.

Expected values: the float64 restatements of tests/test_video_cond_host.py,
evaluated on the CPU.

Tolerances (norm-wise relative error of a whole tensor).
  ops.cross_attention, output and every gradient
      tol = min(0.25, max(floor, 8 * e_ref)).  e_ref: the error, against float64 on the
      original inputs, of the SAME restatement evaluated in float32 -- for the
      bf16 cases with every input rounded to bf16 first (the precision the
      kernel's operands have).  It is computed per case and per tensor inside
      the test, from the restatement alone, and printed next to the kernel's
      error.  Measured on the CPU for these inputs: f32 e_ref 2.5e-7 .. 4.5e-7
      (output), 2.1e-7 .. 8.1e-7 (gradients; up to 6.7e-6 in the unequal-logit
      cases); bf16 e_ref 3.1e-3 .. 3.5e-3 (output; up to 1.0e-2 unequal),
      3.0e-3 .. 7.7e-3 (gradients; up to 1.4e-1 unequal, where one rounded
      logit near 30 moves a saturated softmax).
      The multiple: the elementwise kernels of tests/test_objectives_gpu.py get
      4 * e32, one rounding per value on either side.  Here the restatement
      rounds its inputs once, while the kernel rounds at about twice as many
      places along the same chain -- the folded operand images, the stored
      probabilities P, the dO / dS / P' buffers of the token reductions, the
      output -- and evaluates LayerNorm algebraically (s = rs * (S - mu *
      colsum)), so twice that margin: 8.
      The floor is what the multiple cannot express when e_ref is tiny: f32
      1e-5 (fast exp / log / rsqrt intrinsics at a few ulp and the one-pass
      variance; half the 2e-5 bar tests/test_ops_gpu.py sets for the 3-key
      kernel), bf16 2^-8 (one bf16 ulp: the output itself is rounded to bf16).
      The cap: whatever e_ref is, tol <= 0.25, so that every tensor's check can
      fail (an all-zero result scores 1.0; one head of eight missing about
      0.35); it binds only in the bf16 unequal-logit gradients.
  key permutation            <= 1e-5, the f32 floor above (an f32 run)
  3-key call before / after  torch.equal
  Unet3D forward / gradients 1e-4 / 1e-3: the f32 bars of
                             test_unet_gpu.test_p_losses_forward_backward_vs_oracle
  graph replay vs eager      < 1e-5: the Unet3D bar of
                             test_ddim_gpu.test_ddim_loop_graph_replay_matches_eager
  trainer, replayed vs eager loss <= 1e-5: the f32 bar of
                             test_cfg2_trainer_gpu.test_cfg2_trainer_graph_replay_vs_eager_vs_oracle
The observed values are printed and appended to $DV_PARITY_LOG.
"""
import functools

import pytest
import torch

import test_video_cond_host as H

pytestmark = pytest.mark.gpu

E = H.E
FLOOR = {torch.float32: 1e-5, torch.bfloat16: 2.0 ** -8}
MULT = 8
CAP = 0.25


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


# ---------------------------------------------------------------------------
# ops.cross_attention with 7 keys
# ---------------------------------------------------------------------------
# (nb, T, H, W, C): the first three are the issue's; the others are the sizes at
# which the token kernels take another path with two key tiles: 4 waves per tile
# (C >= 128), the LDS-staged operand images (8 waves, C = 256), the unstaged
# 8-wave form (C = 512), the bounded channel loop with a tail under 4 waves (160)
# and channel counts below one 32-channel tile (8, 16: the small Unet3D of the tests below)
SHAPES = [(2, 2, 4, 8, 64), (3, 1, 5, 7, 96), (2, 2, 3, 3, 48), (2, 1, 4, 8, 128), (2, 1, 4, 8, 256),
          (2, 1, 4, 8, 512), (2, 1, 5, 7, 160), (2, 2, 4, 8, 8), (2, 2, 4, 8, 16)]
NAMES = ("x", "ctx", "g1", "null_kv", "wq", "wkv", "wo", "g2")


@functools.lru_cache(maxsize=None)
def _xattn_case(shape, unequal):
    """Inputs (f32, CPU) and the float64 output / gradients, computed once."""
    nb, T, Hh, W, C = shape
    g = torch.Generator().manual_seed(17 + C)
    r = lambda *s: torch.randn(*s, generator=g)
    ins = dict(x=r(nb * T, Hh, W, C), ctx=r(nb, 6, 64), g1=1 + 0.1 * r(C), null_kv=r(2, 64),
               wq=r(512, C) / C ** 0.5, wkv=r(1024, 64) / 8, wo=r(C, 512) / 512 ** 0.5, g2=1 + 0.1 * r(C))
    if unequal:  # one key far from the other six (every head of clip 0 sees it)
        ins["ctx"][0, 3] *= 30
    gy = r(nb * T, Hh, W, C)
    return ins, gy, _restate(ins, gy, shape, torch.float64, None)


def _restate(ins, gy, shape, dtype, round_to):
    nb, T, Hh, W, C = shape
    rnd = (lambda t: t.to(round_to).float()) if round_to is not None else (lambda t: t)
    leaf = {k: rnd(v).to(dtype).detach().clone().requires_grad_(True) for k, v in ins.items()}
    y = H.cross_attention(leaf["x"].reshape(nb, -1, C), *[leaf[k] for k in NAMES[1:]], 1e-5)
    y = y.reshape(nb * T, Hh, W, C)
    (y * gy.to(dtype)).sum().backward()
    return dict(y=y.detach(), **{"d" + k: leaf[k].grad for k in NAMES})


@pytest.mark.parametrize("unequal", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_cross_attention_7_keys_vs_float64(parity_log, shape, dtype, unequal):
    """Forward and backward (dx, dctx / dwkv through to_kv, dnull_kv, dwq, dwo,
    dg1, dg2) of ops.cross_attention with 6 context tokens per clip; every clip
    has its own context.  Tolerance: the module docstring's rule."""
    from dalle2_video import ops

    nb = shape[0]
    ins, gy, want = _xattn_case(shape, unequal)
    ref = _restate(ins, gy, shape, torch.float32, torch.bfloat16 if dtype == torch.bfloat16 else None)
    dev = {k: v.clone().cuda().requires_grad_(True) for k, v in ins.items()}
    xd = ins["x"].to(dtype).cuda().requires_grad_(True)
    y = ops.cross_attention(xd, *[dev[k] for k in NAMES[1:]], nb, 1e-5)
    assert y.dtype == dtype and y.shape == xd.shape
    (y.float() * gy.cuda()).sum().backward()
    got = dict(y=y, dx=xd.grad, **{"d" + k: dev[k].grad for k in NAMES[1:]})
    bad = {}
    for k in want:
        e_ref, err = rel(ref[k], want[k]), rel(got[k].float(), want[k])
        tol = min(CAP, max(FLOOR[dtype], MULT * e_ref))
        print(f"{shape} {dtype} unequal={unequal} {k}: err {err:.3e} e_ref {e_ref:.3e} tol {tol:.3e}")
        parity_log(shape=list(shape), dtype=str(dtype), unequal=unequal, what=k, rel=err, e_ref=e_ref, tol=tol)
        if not err <= tol:
            bad[k] = (err, tol)
    assert not bad, bad


def test_cross_attention_is_invariant_to_the_order_of_the_context_tokens(parity_log):
    """Permuting the 6 context tokens of one clip permutes keys 1..6 of every
    head and must not change the output: a k' mapping error that a symmetric
    context would hide shows here."""
    from dalle2_video import ops

    shape = SHAPES[0]
    ins, _, _ = _xattn_case(shape, False)
    perm = torch.tensor([4, 2, 0, 5, 1, 3])
    ctx2 = ins["ctx"].clone()
    ctx2[1] = ins["ctx"][1, perm]
    with torch.no_grad():
        a = ops.cross_attention(ins["x"].cuda(), ins["ctx"].cuda(), *[ins[k].cuda() for k in NAMES[2:]], shape[0], 1e-5)
        b = ops.cross_attention(ins["x"].cuda(), ctx2.cuda(), *[ins[k].cuda() for k in NAMES[2:]], shape[0], 1e-5)
    e = rel(b, a)
    parity_log(permutation_rel=e)
    assert e <= FLOOR[torch.float32]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_three_key_call_is_the_same_before_and_after_a_seven_key_call(dtype):
    from dalle2_video import ops

    shape = SHAPES[0]
    ins, gy, _ = _xattn_case(shape, False)

    def run(ctx):
        dev = {k: v.clone().cuda().requires_grad_(True) for k, v in ins.items() if k != "ctx"}
        dev["ctx"] = ctx.clone().cuda().requires_grad_(True)
        dev["x"] = ins["x"].to(dtype).cuda().requires_grad_(True)
        y = ops.cross_attention(*[dev[k] for k in NAMES], shape[0], 1e-5)
        (y.float() * gy.cuda()).sum().backward()
        # the output and dx: the parameter gradients are summed by float atomics
        # (dnull_kv over heads and clips, the split token reductions), whose order
        # differs from run to run with or without a 7-key call in between
        return [y.detach(), dev["x"].grad]

    before = run(ins["ctx"][:, :2])
    run(ins["ctx"])
    after = run(ins["ctx"][:, :2])
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_other_key_counts_raise():
    from dalle2_video import _lib, ops

    ins, _, _ = _xattn_case(SHAPES[0], False)
    for m in (1, 3, 5):
        with pytest.raises(_lib.DVError, match="3 or 7 keys"):
            ops.cross_attention(ins["x"].cuda(), ins["ctx"][:, :m].cuda(), *[ins[k].cuda() for k in NAMES[2:]],
                                SHAPES[0][0], 1e-5)


# ---------------------------------------------------------------------------
# Unet3D with conditioning (dim 8, dim_mults (1, 2), clip 2 x 3 x 2 x 32 x 32)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _unet_case():
    u, ou, vp = H.make_pair()
    g = torch.Generator().manual_seed(21)
    x = torch.randn(2, 3, 2, 32, 32, generator=g)
    t = torch.tensor([37, 610])
    e = torch.randn(2, E, generator=g)
    gy = torch.randn(2, 3, 2, 32, 32, generator=g)
    return u.cuda(), ou, vp, x, t, e, gy


VIDEO_PARAMS = ("video_to_tokens.0.weight", "video_to_tokens.0.bias", "to_video_hiddens.0.weight",
                "to_video_hiddens.0.bias", "null_video_embed", "null_video_hiddens")
VP_KEYS = ("tok_w", "tok_b", "hid_w", "hid_b", "null_embed", "null_hiddens")


def _oracle_grads(ou, vp, x, t, e, keep, gy):
    leaf = {k: v.clone().requires_grad_(True) for k, v in vp.items()}
    out = H.unet_forward(ou, leaf, x.double(), t, e.double(), keep)
    (out * gy.double()).sum().backward()
    ou.zero_grad()
    return out.detach(), {n: leaf[k].grad for n, k in zip(VIDEO_PARAMS, VP_KEYS)}


def _ours_grads(u, x, t, e, gy, **kw):
    u.zero_grad()
    out = u(x.cuda(), t.cuda(), video_embed=e.cuda(), **kw)
    (out * gy.cuda()).sum().backward()
    sd = dict(u.named_parameters())
    return out.detach(), {n: sd[n].grad.clone() for n in VIDEO_PARAMS}


def test_unet_forward_and_video_gradients_vs_float64(parity_log):
    u, ou, vp, x, t, e, gy = _unet_case()
    want, gwant = _oracle_grads(ou, vp, x, t, e, torch.ones(2, dtype=torch.bool), gy)
    got, ggot = _ours_grads(u, x, t, e, gy)
    e_out = rel(got, want)
    errs = {n: rel(ggot[n], gwant[n]) for n in ("video_to_tokens.0.weight", "video_to_tokens.0.bias",
                                                 "to_video_hiddens.0.weight", "to_video_hiddens.0.bias")}
    parity_log(out_rel=e_out, **errs)
    print(e_out, errs)
    assert e_out < 1e-4
    assert all(ggot[n].abs().max() > 0 for n in errs)
    assert all(v < 1e-3 for v in errs.values()), errs
    # every sample kept: the nulls are not read
    assert ggot["null_video_embed"].abs().max() == 0 and ggot["null_video_hiddens"].abs().max() == 0


def test_unet_output_follows_the_embedding_unless_it_is_dropped():
    u, _, _, x, t, e, _ = _unet_case()
    e2 = e.flip(0) * 0.5
    with torch.no_grad():
        a, b = u(x.cuda(), t.cuda(), video_embed=e.cuda()), u(x.cuda(), t.cuda(), video_embed=e2.cuda())
        da = u(x.cuda(), t.cuda(), video_embed=e.cuda(), video_cond_drop_prob=1.0)
        db = u(x.cuda(), t.cuda(), video_embed=e2.cuda(), video_cond_drop_prob=1.0)
    assert rel(b, a) > 1e-4
    assert torch.equal(da, db)
    assert rel(da, a) > 1e-4
    with pytest.raises(ValueError, match="video_embed is required"):
        u(x.cuda(), t.cuda())


def test_unet_mixed_keep_mask_routes_the_null_gradients(parity_log):
    """video_cond_drop_prob = 0.5 with the device generator seeded so that
    sample 0 is kept and sample 1 dropped (the mask is the forward's first
    draw, regenerated here from the seed)."""
    u, ou, vp, x, t, e, gy = _unet_case()
    for seed in range(64):
        torch.cuda.manual_seed(seed)
        keep = (torch.empty((2,), device="cuda").uniform_(0, 1) < 0.5).cpu()
        if keep.tolist() == [True, False]:
            break
    else:
        pytest.fail("no seed gives the mixed mask")
    want, gwant = _oracle_grads(ou, vp, x, t, e, keep, gy)
    torch.cuda.manual_seed(seed)
    got, ggot = _ours_grads(u, x, t, e, gy, video_cond_drop_prob=0.5)
    e_out = rel(got, want)
    errs = {n: rel(ggot[n], gwant[n]) for n in VIDEO_PARAMS}
    parity_log(seed=seed, out_rel=e_out, **errs)
    print(e_out, errs)
    assert e_out < 1e-4
    assert all(ggot[n].abs().max() > 0 for n in VIDEO_PARAMS)
    assert all(v < 1e-3 for v in errs.values()), errs
    # a loss that reads only the kept sample leaves the nulls without gradient; one
    # that reads only the dropped sample leaves the projections without
    for only, zero, nonzero in ((0, ("null_video_embed", "null_video_hiddens"), ("video_to_tokens.0.weight",)),
                                (1, ("video_to_tokens.0.weight", "to_video_hiddens.0.weight"), ("null_video_embed",
                                                                                             "null_video_hiddens"))):
        g1 = torch.zeros_like(gy)
        g1[only] = gy[only]
        torch.cuda.manual_seed(seed)
        _, gg = _ours_grads(u, x, t, e, g1, video_cond_drop_prob=0.5)
        assert all(gg[n].abs().max() == 0 for n in zero), (only, zero)
        assert all(gg[n].abs().max() > 0 for n in nonzero), (only, nonzero)


# ---------------------------------------------------------------------------
# decoder, trainer, cascade
# ---------------------------------------------------------------------------
def _decoder(**kw):
    from dalle2_video import dalle2_video as D

    u, _, _ = H.make_pair()
    args = dict(frame_sizes=(32,), frame_numbers=(2,), timesteps=20, sample_timesteps=6, ddim_sampling_eta=0.0,
                learned_variance=False)
    args.update(kw)
    return D.VideoDecoder(u, **args).cuda().eval()


def _embeds():
    g = torch.Generator().manual_seed(5)
    return torch.randn(2, E, generator=g).cuda(), torch.randn(2, E, generator=g).cuda()


def test_sample_guidance_scale_changes_the_result():
    dec = _decoder()
    dec.sample_graphs = False
    e1, _ = _embeds()
    outs = []
    for cs in (1.0, 2.0):
        torch.cuda.manual_seed(11)
        outs.append(dec.sample(video_embed=e1, cond_scale=cs))
    assert outs[0].shape == (2, 3, 2, 32, 32) and all(torch.isfinite(o).all() for o in outs)
    assert rel(outs[1], outs[0]) > 1e-4


@pytest.mark.parametrize("graphs", [False, True])
def test_ddpm_sampling_follows_the_embedding(graphs):
    """DDPM over the whole (6-step) schedule, eager and with the captured step:
    the same seed with two embeddings gives two results."""
    dec = _decoder(timesteps=6, sample_timesteps=None)
    dec.sample_graphs = graphs
    e1, e2 = _embeds()
    outs = []
    for e in (e1, e2):
        torch.cuda.manual_seed(13)
        outs.append(dec.sample(video_embed=e))
    assert outs[0].shape == (2, 3, 2, 32, 32) and all(torch.isfinite(o).all() for o in outs)
    assert rel(outs[1], outs[0]) > 1e-4


@pytest.mark.parametrize("cond_scale", [1.0, 2.0])
def test_ddim_graph_replay_matches_eager_with_an_embedding(parity_log, cond_scale):
    dec = _decoder()
    e1, e2 = _embeds()
    outs = []
    for graphs, e in ((False, e1), (True, e1), (True, e2)):
        dec.sample_graphs = graphs
        torch.cuda.manual_seed(77)
        outs.append(dec.sample(video_embed=e, cond_scale=cond_scale))
    eager, graph, other = outs
    assert torch.isfinite(eager).all() and torch.isfinite(graph).all()
    err = rel(graph, eager)
    parity_log(cond_scale=cond_scale, graph_vs_eager_rel=err)
    assert err < 1e-5
    assert rel(other, graph) > 1e-4  # the embedding reaches the replayed forwards


def test_replayed_step_follows_a_new_embedding_in_its_input_buffer(parity_log):
    from dalle2_video import dalle2_video as D

    dec = _decoder()
    unet, sched = dec.unets[0], dec.noise_schedulers[0]
    e1, e2 = _embeds()
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(2, 3, 2, 32, 32, generator=g).cuda()

    def make(e):
        return D._DenoiseStepGraph(dec, unet, x0.clone(), e, sched, 1.0, None, True, ddim_eta=0.0)

    with torch.no_grad():
        step = make(e1)
        for _ in range(D._DenoiseStepGraph.EAGER_CALLS + 1):  # the last call captures and replays
            step.x.copy_(x0)
            step(15, 11)
        assert step.graph is not None
        r1 = step.x.clone()
        step.x.copy_(x0)
        step.video_embed.copy_(e2)
        step(15, 11)
        r2 = step.x.clone()
        eager = make(e2)
        eager(15, 11)
        assert eager.graph is None
    err = rel(r2, eager.x)
    parity_log(replay_new_embed_vs_eager_rel=err, moved=rel(r2, r1))
    assert err < 1e-5
    assert rel(r2, r1) > 1e-4


def test_trainer_captured_step_takes_the_embedding_as_a_graph_input(parity_log):
    from dalle2_video.trainer import VideoDecoderTrainer

    dec = _decoder(timesteps=1000, sample_timesteps=None).train()
    tr = VideoDecoderTrainer(dec, lr=3e-4, wd=1e-2, use_ema=False, amp=False, use_graphs=True)
    g = torch.Generator().manual_seed(1234)
    video = torch.rand(2, 3, 2, 32, 32, generator=g).cuda()
    e1, e2 = _embeds()
    torch.cuda.manual_seed(1)
    tr(video=video, video_embed=e1, unet_number=1)
    tr.update(1)  # builds the flat buffers (the first call is never captured)
    opt = tr.optim0
    res = {}
    # A, B: the two eager warm-up calls; C captures and replays; D, E replay
    for tag, seed, e in (("A", 7, e1), ("B", 8, e2), ("C", 7, e1), ("D", 8, e2), ("E", 7, e2)):
        opt.zero_grad()
        torch.cuda.manual_seed(seed)
        res[tag] = tr(video=video, video_embed=e, unet_number=1)
        torch.cuda.synchronize()
    ent = next(iter(tr._graphs.values()))
    assert len(tr._graphs) == 1 and "graph" in ent, "the training step was not captured"
    errs = {"AC": abs(res["A"] - res["C"]) / abs(res["A"]), "BD": abs(res["B"] - res["D"]) / abs(res["B"])}
    parity_log(**errs, moved=abs(res["E"] - res["C"]) / abs(res["C"]))
    assert all(v <= 1e-5 for v in errs.values()), (errs, res)
    assert abs(res["E"] - res["C"]) > 1e-5 * abs(res["C"])  # same seed, other embedding


def test_cascade_conditioned_base_and_unconditioned_second_unet():
    from dalle2_video import dalle2_video as D

    u1, _, _ = H.make_pair()
    u2 = D.Unet3D(8, video_embed_dim=E, channels=3, dim_mults=(1, 2))
    dec = D.VideoDecoder((u1, u2), frame_sizes=(32, 64), frame_numbers=(2, 2), timesteps=12,
                         sample_timesteps=(4, 4), beta_schedule=("cosine", "cosine"), learned_variance=False).cuda()
    assert dec.unets[0].cond_on_video_embeds is True and dec.unets[1].cond_on_video_embeds is False
    H.fill_(dec.unets[1])
    e1, _ = _embeds()
    g = torch.Generator().manual_seed(4)
    video = torch.rand(2, 3, 2, 64, 64, generator=g).cuda()
    for k in (1, 2):
        torch.cuda.manual_seed(k)
        loss = dec(video, video_embed=e1, unet_number=k)
        loss.backward()
        assert torch.isfinite(loss)
    assert dec.unets[0].video_to_tokens[0].weight.grad.abs().max() > 0
    dec.eval()
    dec.sample_graphs = False
    torch.cuda.manual_seed(3)
    vid = dec.sample(video_embed=e1, cond_scale=2.0)
    assert vid.shape == (2, 3, 2, 64, 64) and torch.isfinite(vid).all()
