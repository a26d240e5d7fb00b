"""Float64 restatements for the inpainting tests (RePaint, arXiv 2201.09865, as
the reference's DDIM loop carries it: dalle2_video.py:1822-1828 the blend,
:1878-1883 the renoise, :1885-1886 the blend after the loop).  Plain PyTorch on
the CPU; the schedule tables are taken as given (the tests pass the f32 tables
the kernel reads, so their rounding is common to both sides).
"""
import torch


def bc(v):
    return v.reshape(-1, 1, 1, 1, 1)


def blend_restatement(x, known, mask, noise, t, t_from, sqrt_ac, sqrt_1m_ac, normalize=False, final=False,
                      dtype=torch.float64):
    """The four branches of dv_inpaint_blend.  x, known, noise: (b, c, f, h, w);
    mask: (b, f, h, w), nonzero = known; t, t_from: (b,) long or None.

    Returns (out, c1a, c2b): the result and the magnitudes |c1 * a| and |c2 * b|
    of the two terms every noised element is the sum of (zero where the element
    is copied).  A sample whose t is outside the tables, or whose t_from is
    negative or >= t, has every element the call writes set to NaN."""
    x, known = x.cpu().to(dtype), known.cpu().to(dtype)
    m = bc_mask(mask, x)
    k = 2 * known - 1 if normalize else known
    zero = torch.zeros_like(x)
    if final:
        return torch.where(m, k, x), zero, zero
    noise = noise.cpu().to(dtype)
    t = t.cpu()
    nt = sqrt_ac.numel()
    ok = (t >= 0) & (t < nt)
    if t_from is not None:
        t_from = t_from.cpu()
        ok = ok & (t_from >= 0) & (t_from < t)
    ts = torch.where(ok, t, torch.zeros_like(t))
    a, s = sqrt_ac.cpu().to(dtype), sqrt_1m_ac.cpu().to(dtype)
    at, st = bc(a[ts]), bc(s[ts])
    out = torch.where(m, at * k + st * noise, x)
    c1a = torch.where(m, (at * k).abs(), zero)
    c2b = torch.where(m, (st * noise).abs(), zero)
    written = m
    if t_from is not None:
        us = torch.where(ok, t_from, torch.zeros_like(t))
        au, su = bc(a[us]), bc(s[us])
        # NoiseScheduler.q_sample_from_to(x, from_t=u, to_t=t) of dalle2-pytorch
        f1, f2 = at / au, (st * au - su * at) / au
        out = torch.where(m, out, x * f1 + noise * f2)
        c1a = torch.where(m, c1a, (x * f1).abs())
        c2b = torch.where(m, c2b, (noise * f2).abs())
        written = torch.ones_like(m)
    bad = bc(~ok) & written
    nan = torch.full_like(x, float("nan"))
    return torch.where(bad, nan, out), c1a, c2b


def bc_mask(mask, x):
    return mask.cpu().ne(0)[:, None].expand(-1, x.shape[1], -1, -1, -1)


def inpaint_passes(pairs, resample_times):
    """[(time, time_next, renoise_after)] of the loop at :1811-1883: every pair
    runs resample_times passes; every pass except a pair's last and except those
    of the last pair is followed by the renoise time_next -> time."""
    out = []
    for i, (t, tn) in enumerate(pairs):
        for r in reversed(range(resample_times)):
            out.append((t, tn, not (i == len(pairs) - 1 or r == 0)))
    return out


def repaint_loop(update, x, known, mask, pairs, resample_times, blend_noises, sqrt_ac, sqrt_1m_ac,
                 normalize=True, dtype=torch.float64):
    """The whole RePaint loop around a caller-supplied update and caller-
    supplied noise: update(x, time, time_next, pass_index) -> the sampler's
    x_{time_next} (the denoiser and the DDPM / DDIM update); blend_noises[i] is
    the draw of pass i, shared by its blend and by the renoise that precedes it
    (one launch in the kernel, two statements here).  Returns the normalised
    result after the final blend."""
    x = x.cpu().to(dtype)
    b = x.shape[0]
    full = lambda v: torch.full((b,), v, dtype=torch.long)
    none = torch.zeros(mask.shape, dtype=torch.bool)
    pending = None  # the level the previous pass ended on, when a renoise follows it
    for i, (t, tn, renoise_after) in enumerate(inpaint_passes(pairs, resample_times)):
        if pending is not None:  # :1883, with this pass's noise
            x, _, _ = blend_restatement(x, known, none, blend_noises[i], full(t), full(pending), sqrt_ac,
                                        sqrt_1m_ac, normalize, dtype=dtype)
        x, _, _ = blend_restatement(x, known, mask, blend_noises[i], full(t), None, sqrt_ac, sqrt_1m_ac,
                                    normalize, dtype=dtype)  # :1825-1828
        x = update(x, t, tn, i)
        pending = tn if renoise_after else None
    return blend_restatement(x, known, mask, None, None, None, sqrt_ac, sqrt_1m_ac, normalize, final=True,
                             dtype=dtype)[0]
