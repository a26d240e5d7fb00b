"""Inputs with closed-form answers for GroupNorm (+ FiLM, activation, residual)
(ops.group_norm_act / dv_gn_fwd / dv_gn_bwd).

Shared by tests/test_gn_cases_host.py (which proves the closed forms against
torch.nn.functional.group_norm and autograd in float64) and
tests/test_gn_exact_gpu.py (which holds the HIP kernels to them element by
element).  Layout: z, res, dy are (nb, P, C) -- clip, pixel, channel -- i.e. the
kernels' (nb * P, C) rows; the per-clip FiLM tensor ss is (nb, 2C) = scale | shift.

Two-level family.  Group g of clip b has a centre m[b, g] = j * s and a
half-width s[b, g], s a power of two in {1/4, 1/2, 1, 2}, j an integer with
|j| <= 8 (clip 0 / group 0 has j = -8: the offset case); neighbouring clips
and groups differ in both.  Every element is m + sigma * s with sigma = +-1
from a fixed 32-bit hash of (pixel, channel, clip) -- no period in pixels or
channels -- and the last elements of the group (pixel-major order) are flipped
until exactly half of its P * C/G elements sit at each level.  Then, with
eps = 0,
    mean = m,   var = s^2,   rstd = 1 / s,   zhat = sigma      (exactly)
and every per-channel f32 sum of z and z^2 is a sum of integers (in units of
s, s^2) that stays below 2^24, so the kernels' f32 statistics are exact in any
summation order (Case.check_exact asserts the bound).

Parameters are dyadic and hashed from (clip, channel): gamma in +-{1..7}/4,
beta and the FiLM shift in {-4..4}/4, the FiLM scale in {-1/2, 0, 1/2, 1}, the
residual in {2..8}/4 (positive: y = act(v) + res never cancels), dy in
{-3..3}/4.  The pre-activation v = sigma * gamma' + beta' (gamma' = gamma (1 +
scale), beta' = beta (1 + scale) + shift) has |v| <= 6.5.

Gaussian family.  z = 2 randn + 0.5 and Gaussian parameters (fixed seed), the
inputs tests/test_ops_gpu.py uses; the expectation is the same float64 formula
with the statistics computed from the data.
"""
import functools

import torch

ACT_NONE, ACT_SILU = 0, 1
M32 = 0xFFFFFFFF

# the table of tests/test_gn_exact_gpu.py: row -> (nb, P, C, G)
ROWS = {
    "1": (2, 37, 64, 8),
    "2": (2, 4133, 64, 8),
    "3": (2, 3617, 512, 8),
    "4": (3, 1000, 256, 8),
    "5": (2, 50, 48, 8),
    "6": (3, 70, 1024, 32),
    "7": (2, 300, 8, 1),
    "8": (2, 130, 512, 64),
    "8f": (2, 130, 64, 64),  # C / G = 1: f32 only (a bf16 vector holds 8 channels)
}
# pre-summed statistics (part B): (C, G, R), nb = 2, P = 256
PRESUM_NB, PRESUM_P = 2, 256
PRESUM = [(64, 8, 1), (64, 8, 3), (64, 8, 8), (64, 8, 9), (64, 8, 64), (256, 8, 3), (256, 8, 8),
          (512, 8, 3), (512, 8, 8), (1024, 32, 2)]
# single launch (part C): (nb, P, C, G)
COOP = [(16, 100, 64, 8), (16, 1100, 64, 8), (16, 2100, 64, 8), (16, 4200, 64, 8), (16, 8200, 64, 8),
        (2, 70, 512, 8)]


def _mix(x):
    """32-bit avalanche (int64 tensors holding 32-bit values)."""
    x = x & M32
    x = x ^ (x >> 15)
    x = (x * 0x2C1B3C6D) & M32
    x = x ^ (x >> 12)
    x = (x * 0x297A2D39) & M32
    return x ^ (x >> 15)


def hash3(a, b, c, salt):
    return _mix(a * 0x9E3779B1 + b * 0x85EBCA6B + c * 0xC2B2AE35 + salt * 0x27D4EB2F)


def centres(nb, G):
    """j[b, g] = m / s in -8..8 and log2 s in -2..1; (0, 0) is the offset case j = -8."""
    b = torch.arange(nb)[:, None]
    g = torch.arange(G)[None, :]
    j = (5 * g + 7 * b) % 17 - 8
    e = (g + g // 4 + 2 * b) % 4 - 2
    return j.double(), torch.pow(2.0, e.double())


def signs(nb, P, C, G):
    """sigma (nb, P, C) in {-1, +1}: hashed, then balanced per (clip, group)."""
    cg, n = C // G, P * (C // G)
    assert n % 2 == 0, "P * C/G must be even"
    b = torch.arange(nb)[:, None, None]
    p = torch.arange(P)[None, :, None]
    c = torch.arange(C)[None, None, :]
    bit = ((hash3(p, c, b, 1) >> 7) & 1).to(torch.int8)
    rows = bit.reshape(nb, P, G, cg).permute(0, 2, 1, 3).reshape(nb * G, n).clone()
    for row in rows:
        ex = int(row.sum(dtype=torch.int64)) - n // 2
        if ex > 0:
            row[(row == 1).nonzero().flatten()[-ex:]] = 0
        elif ex < 0:
            row[(row == 0).nonzero().flatten()[ex:]] = 1
    sg = rows.reshape(nb, G, P, cg).permute(0, 2, 1, 3).reshape(nb, P, C)
    return (2 * sg.to(torch.int16) - 1).double().contiguous()


def silu(v):
    return v * torch.sigmoid(v)


def silu_grad(v):
    sg = torch.sigmoid(v)
    return sg * (1 + v * (1 - sg))


class Case:
    """Inputs (float64) of one shape; expectations through expect()."""

    def __init__(self, family, nb, P, C, G):
        self.family, self.nb, self.P, self.C, self.G = family, nb, P, C, G
        self.cg = C // G
        self.eps = 0.0 if family == "two" else 1e-5

    def per_channel(self, t):
        """(nb, G) -> (nb, 1, C)"""
        return t.repeat_interleave(self.cg, 1)[:, None, :]

    def film(self, on):
        """(1 + scale, shift), each (nb, C); ones / zeros without FiLM."""
        if not on:
            return torch.ones(self.nb, self.C, dtype=torch.float64), torch.zeros(self.nb, self.C, dtype=torch.float64)
        return 1 + self.ss[:, :self.C], self.ss[:, self.C:]

    def stats(self):
        """mean, rstd (nb, G) and zhat (nb, P, C) in float64: closed form / from the data."""
        if self.family == "two":
            return self.m, 1 / self.s, self.sigma
        zg = self.z.reshape(self.nb, self.P, self.G, self.cg)
        mean = zg.mean((1, 3))
        var = (zg * zg).mean((1, 3)) - mean * mean
        rstd = 1 / torch.sqrt(var + self.eps)
        return mean, rstd, (self.z - self.per_channel(mean)) * self.per_channel(rstd)

    def expect(self, act, film, res):
        """Float64 results of forward and backward (dict).  S is the dz bound's scale:
        rstd (|gamma' dv| + |m1| + |m2|) per element."""
        mean, rstd, zhat = self.stats()
        sc, sh = self.film(film)
        ge, be = self.gamma * sc, self.beta * sc + sh  # (nb, C)
        v = zhat * ge[:, None, :] + be[:, None, :]
        y = silu(v) if act == ACT_SILU else v.clone()
        if res:
            y = y + self.res
        dv = self.dy * silu_grad(v) if act == ACT_SILU else self.dy
        gdv = ge[:, None, :] * dv
        grp = lambda t: t.reshape(self.nb, self.P, self.G, self.cg).mean((1, 3))
        m1, m2 = self.per_channel(grp(gdv)), self.per_channel(grp(gdv * zhat))
        rs = self.per_channel(rstd)
        dz = rs * (gdv - m1 - zhat * m2)
        s1, s2 = dv.sum(1), (dv * zhat).sum(1)  # (nb, C)
        out = dict(mean=mean, rstd=rstd, v=v, y=y, dz=dz, S=rs * (gdv.abs() + m1.abs() + m2.abs()),
                   dgamma=(sc * s2).sum(0), dbeta=(sc * s1).sum(0), s1=s1, s2=s2)
        if film:
            out["dss"] = torch.cat([self.gamma * s2 + self.beta * s1, s1], 1)
        return out

    def check_exact(self):
        """The conditions under which the kernels' f32 sums are exact (two-level family)."""
        assert self.family == "two"
        n = self.P * self.cg
        assert n % 2 == 0
        sg = self.sigma.reshape(self.nb, self.P, self.G, self.cg)
        assert bool((sg.sum((1, 3)) == 0).all()), "half / half"
        # forward: per-channel sums of z / s and (z / s)^2 are sums of integers <= (|j| + 1), (|j| + 1)^2
        zmax = float((self.m / self.s).abs().max()) + 1
        assert zmax <= 9 and self.P * zmax * zmax < 2 ** 24
        # backward, act NONE: 4 dy and 4 dy zhat are integers <= 3; per channel |sum| <= 3 P
        assert float((4 * self.dy).abs().max()) <= 3 and 3 * self.P < 2 ** 24
        # group terms: gamma' s1 in units of 1/32, summed over the group's channels in any order
        for film in (False, True):
            sc, _ = self.film(film)
            k = self.gamma * sc
            for s in (self.dy.sum(1), (self.dy * self.sigma).sum(1)):
                tot = (k * s).abs().reshape(self.nb, self.G, self.cg).sum(-1)
                assert float(tot.max()) * 32 < 2 ** 24
                # dss: gamma s2 + beta s1 in units of 1/16; dgamma / dbeta: the clips' sum in units of 1/8
                assert float((self.gamma.abs() * s.abs()).max() + s.abs().max()) * 16 < 2 ** 24
                assert float((sc * s).abs().sum(0).max()) * 8 < 2 ** 24
        assert n < 2 ** 24  # (float)n is exact


def _params(case):
    nb, C = case.nb, case.C
    c = torch.arange(C)
    b = torch.arange(nb)[:, None]
    z0 = torch.zeros_like(c)
    hg = hash3(c, z0, z0, 2)
    case.gamma = ((hg % 7 + 1) * (2 * ((hg >> 9) & 1) - 1)).double() / 4
    case.beta = (hash3(c, z0, z0, 3) % 9 - 4).double() / 4
    scale = torch.tensor([-0.5, 0.0, 0.5, 1.0], dtype=torch.float64)[hash3(c[None, :], b, z0, 4) % 4]
    shift = (hash3(c[None, :], b, z0, 5) % 9 - 4).double() / 4
    case.ss = torch.cat([scale, shift], 1)


def two_level_case(nb, P, C, G):
    case = Case("two", nb, P, C, G)
    j, s = centres(nb, G)
    case.m, case.s = j * s, s
    case.sigma = signs(nb, P, C, G)
    case.z = case.per_channel(case.m) + case.sigma * case.per_channel(s)
    _params(case)
    b = torch.arange(nb)[:, None, None]
    p = torch.arange(P)[None, :, None]
    c = torch.arange(C)[None, None, :]
    case.res = (hash3(p, c, b, 6) % 7 + 2).double() / 4
    case.dy = (hash3(p, c, b, 7) % 7 - 3).double() / 4
    case.check_exact()
    return case


def gaussian_case(nb, P, C, G):
    case = Case("gauss", nb, P, C, G)
    g = torch.Generator().manual_seed(1000 * C + P)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    case.z = r(nb, P, C) * 2 + 0.5
    case.gamma, case.beta = 1 + 0.1 * r(C), 0.1 * r(C)
    case.ss = 0.3 * r(nb, 2 * C)
    case.res, case.dy = r(nb, P, C), r(nb, P, C)
    # every activation tensor as the narrowest storage type holds it (bf16), so both dtypes see one input
    for name in ("z", "res", "dy"):
        setattr(case, name, getattr(case, name).bfloat16().double())
    return case


@functools.lru_cache(maxsize=4)
def build(family, nb, P, C, G):
    """Cached: treat the tensors as read-only."""
    return two_level_case(nb, P, C, G) if family == "two" else gaussian_case(nb, P, C, G)


def reference(case, act, film, res, dtype=torch.float64):
    """torch.nn.functional.group_norm + FiLM + activation + residual and autograd, in `dtype`."""
    import torch.nn.functional as F
    nb, P, C = case.nb, case.P, case.C
    leaf = lambda t: t.to(dtype).clone().requires_grad_()
    z, gamma, beta, ss = leaf(case.z), leaf(case.gamma), leaf(case.beta), leaf(case.ss)
    y = F.group_norm(z.permute(0, 2, 1), case.G, gamma, beta, eps=case.eps)  # (nb, C, P)
    if film:
        y = y * (1 + ss[:, :C, None]) + ss[:, C:, None]
    if act == ACT_SILU:
        y = F.silu(y)
    y = y.permute(0, 2, 1)
    if res:
        y = y + case.res.to(dtype)
    (y * case.dy.to(dtype)).sum().backward()
    out = dict(y=y.detach(), dz=z.grad, dgamma=gamma.grad, dbeta=beta.grad)
    if film:
        out["dss"] = ss.grad
    return out


def presums(case, R):
    """(R, nb, C, 2) float64: the per-channel (sum z, sum z^2) split unevenly over R replicas.
    Replica r with r % 3 == 1 is all zero (R >= 3); the others get integer shares (in units of
    s, s^2) proportional to r + 1, the last taking the remainder: every part and every partial
    sum of parts is an integer below 2^24, so any summation order gives the total exactly."""
    assert case.family == "two"
    s = case.s.repeat_interleave(case.cg, 1)  # (nb, C)
    u = torch.stack([case.z.sum(1) / s, (case.z * case.z).sum(1) / (s * s)], -1)  # integers
    assert bool((u == u.round()).all())
    live = [r for r in range(R) if not (R >= 3 and r % 3 == 1)]
    wsum = sum(r + 1 for r in live)
    parts = torch.zeros(R, case.nb, case.C, 2, dtype=torch.float64)
    for r in live[:-1]:
        parts[r] = torch.floor(u * (r + 1) / wsum)
    parts[live[-1]] = u - parts.sum(0)
    assert float(parts.abs().sum(0).max()) < 2 ** 24
    unit = torch.stack([s, s * s], -1)
    return parts * unit
