"""Inputs with closed-form answers for the mid self-attention (ops.mqa).

Shared by tests/test_mqa_cases_host.py (which proves the closed forms against
a float64 softmax attention) and tests/test_mqa_exact_gpu.py (which holds the
HIP kernels to them element by element).  D = 32, H = 16, scale = 1/32; every
input value is exactly representable in bf16 (and the V values in e4m3).

Key index j of a clip: 0 is the null key / value (null_kv[0], null_kv[1]),
j >= 1 is token j - 1.

Code book.  A code c < 2048 with bits b0..b10 is the key
    k[d] = +1 if b_d else -1   (d < 11), repeated in dims 11..21, +1 in 22..31
and the value
    v[d] = b_d (d < 11),  1 - b_(d-11) (11 <= d < 22),  1 (22 <= d < 32).
Distinct codes differ in at least 2 key dims; a value row decodes to its code.
Key j of clip 0 carries code j.  Key j >= 1 of every later clip carries code
2047 - j (the 11-bit complement), so a kernel that reads another clip's K / V,
or the same clip at a shifted row, gets a different answer; the null key
(code 0) is shared, as null_kv is.

Flat family, level c: every key is the all-ones vector, every query element is
c, V is the code book.  All N + 1 logits are equal, so every output row is the
column mean of the clip's V rows 0..N -- whatever c is.  A zero pad key has
logit 0: at negative c it outweighs every real key by 2^46 (2^92), at positive
c a dropped mask is invisible and a dropped key is not.

Selection family: K and V are the code book, query row r = n * H + head of
clip b is 256 * k_pi with pi = (a r + 3 + 5 b) mod (N + 1), gcd(a, N + 1) = 1,
so pi runs over every key index and the heads of one token select different
keys.  The selected logit leads every other by 2 dims * 2 * 256 / 32 = 32 nats
(46 log2 units): softmax is one-hot to 1e-14 and output row r is v_pi.

Upstream gradient: integers in {1, 2, 3} (fixed seed).
"""
import functools
import math

import torch

D, H, SCALE = 32, 16, 1.0 / 32
NBITS = 11
FLAT_LEVELS = (0, 32, -32, 64, -64)
SEL_QMAG = 256.0
LOG2E = 1.4426950408889634
# the bf16 forward keeps no running max while |q| max|k'| <= 64 (log2 units)
FIX_BOUND = 64.0


def nkp(N):
    """Keys after padding to whole 32-key tiles."""
    return (N + 1 + 31) // 32 * 32


def key_codes(B, N):
    """(B, N + 1) long: the code that key j of clip b carries."""
    j = torch.arange(N + 1)
    rows = [j if b == 0 else torch.where(j == 0, j, 2 ** NBITS - 1 - j) for b in range(B)]
    return torch.stack(rows)


def _bits(code):
    return ((code.unsqueeze(-1) >> torch.arange(NBITS)) & 1).double()


def code_k(code):
    b = _bits(code)
    pm = 2 * b - 1
    return torch.cat([pm, pm, torch.ones(*code.shape, D - 2 * NBITS, dtype=torch.float64)], -1)


def code_v(code):
    b = _bits(code)
    return torch.cat([b, 1 - b, torch.ones(*code.shape, D - 2 * NBITS, dtype=torch.float64)], -1)


def decode_v(v):
    """The code a value row names (its first 11 dims, rounded)."""
    return (v[..., :NBITS].round().long() << torch.arange(NBITS)).sum(-1)


def sel_a(N):
    """Smallest multiplier from 7 up that is coprime to N + 1 (7 fails at N = 97, 160, 1280)."""
    a = 7
    while math.gcd(a, N + 1) != 1:
        a += 2
    return a


def sel_pi(B, N):
    """(B, N * H) long: the key index that query row r = n * H + head of clip b selects."""
    r = torch.arange(N * H)
    return torch.stack([(sel_a(N) * r + 3 + 5 * b) % (N + 1) for b in range(B)])


@functools.lru_cache(maxsize=None)
def upstream(B, N):
    g = torch.Generator().manual_seed(1234)
    return torch.randint(1, 4, (B * N, H * D), generator=g).double()


def bf16_key_unit():
    """|k'| per unit of |k| on the bf16 path: dv_mqa_prep stores bf16(k * scale * log2 e)."""
    return float((torch.tensor(1.0) * torch.tensor(SCALE * LOG2E, dtype=torch.float32)).bfloat16())


def flat_score_bound(c):
    """|q| max|k'| of the flat family at level c, as the bf16 forward computes it (log2 units)."""
    return abs(c) * math.sqrt(D) * bf16_key_unit() * math.sqrt(D)


def flat_p_rounding(c):
    """Relative error of bf16(p) against p for the flat family's single probability value in
    the bounded regime (p = exp2(score), no max subtracted); 0 where p is a power of two."""
    if flat_score_bound(c) > FIX_BOUND:
        return 0.0  # online regime: p = exp2(s - max) = 1
    s = c * D * bf16_key_unit()  # the score, log2 units: exact in f32
    p = torch.tensor(2.0 ** s, dtype=torch.float32)
    return abs(float(p.bfloat16().double() / p.double()) - 1.0)


class Case:
    """Inputs (float64, ops.mqa layouts) and closed-form results of one family."""

    def __init__(self, name, B, N, q, kv, null_kv, o, pi=None):
        self.name, self.B, self.N = name, B, N
        self.q, self.kv, self.null_kv, self.o, self.pi = q, kv, null_kv, o, pi
        self.dq = self.dkv = self.dnull = None  # closed forms where they exist (else None)
        self.dv = None  # (B * N, 32): dkv[:, 32:]
        self.dnull_v = None  # (32,): dnull[1]


def flat_case(B, N, c):
    codes = key_codes(B, N)
    v = code_v(codes)  # (B, N + 1, 32)
    q = torch.full((B * N, H * D), float(c), dtype=torch.float64)
    kv = torch.cat([torch.ones(B, N, D, dtype=torch.float64), v[:, 1:]], -1).reshape(B * N, 2 * D)
    null_kv = torch.stack([torch.ones(D, dtype=torch.float64), v[0, 0]])
    mean = v.mean(1)  # (B, 32)
    o = mean[:, None, None, :].expand(B, N, H, D).reshape(B * N, H * D).clone()
    case = Case(f"flat{c:+d}", B, N, q, kv, null_kv, o)
    # every key gets the same share 1 / (N + 1) of every row's upstream gradient
    share = upstream(B, N).reshape(B, N * H, D).sum(1) / (N + 1)  # (B, 32)
    case.dv = share[:, None, :].expand(B, N, D).reshape(B * N, D).clone()
    case.dnull_v = share.sum(0)
    if c == 0:  # q = 0: dK = 0; all keys equal and sum_j dS_j = 0: dQ = 0
        case.dq = torch.zeros_like(q)
        case.dkv = torch.cat([torch.zeros(B * N, D, dtype=torch.float64), case.dv], -1)
        case.dnull = torch.stack([torch.zeros(D, dtype=torch.float64), case.dnull_v])
    return case


def selection_case(B, N):
    codes = key_codes(B, N)
    k, v = code_k(codes), code_v(codes)  # (B, N + 1, 32)
    pi = sel_pi(B, N)  # (B, N * H)
    idx = pi.unsqueeze(-1).expand(B, N * H, D)
    q = (SEL_QMAG * k.gather(1, idx)).reshape(B * N, H * D)
    kv = torch.cat([k[:, 1:], v[:, 1:]], -1).reshape(B * N, 2 * D)
    null_kv = torch.stack([k[0, 0], v[0, 0]])
    o = v.gather(1, idx).reshape(B * N, H * D)
    case = Case("select", B, N, q, kv, null_kv, o, pi)
    # one-hot softmax: dS = p (dP - D) = 0, and dV_j collects the rows that selected j
    dvk = torch.zeros(B, N + 1, D, dtype=torch.float64)
    dvk.scatter_add_(1, idx, upstream(B, N).reshape(B, N * H, D))
    case.dv = dvk[:, 1:].reshape(B * N, D).clone()
    case.dnull_v = dvk[:, 0].sum(0)
    case.dq = torch.zeros_like(q)
    case.dkv = torch.cat([torch.zeros(B * N, D, dtype=torch.float64), case.dv], -1)
    case.dnull = torch.stack([torch.zeros(D, dtype=torch.float64), case.dnull_v])
    return case


@functools.lru_cache(maxsize=None)
def build(family, B, N):
    """family: 'select' or a flat level.  Cached: treat the tensors as read-only."""
    return selection_case(B, N) if family == "select" else flat_case(B, N, int(family))


def selection_gap_log2(B, N):
    """Smallest lead (log2 units, bf16-rounded key scale) of a selected key over any other key."""
    k = code_k(key_codes(B, N))
    gram = torch.einsum("bid,bjd->bij", k, k)
    gram -= 2 * D * torch.eye(N + 1, dtype=torch.float64)  # take the key itself out of the max
    lead = D - gram.max(-1).values  # (B, N + 1): k_j . k_j - max_i k_j . k_i
    return float(lead.min()) * SEL_QMAG * bf16_key_unit()


def reference(q, kv, null_kv, B, N):
    """Plain softmax attention in the inputs' precision, null key / value at index 0."""
    qh = q.reshape(B, N, H, D).transpose(1, 2)
    k = torch.cat((null_kv[0].expand(B, 1, D), kv[:, :D].reshape(B, N, D)), dim=1)
    v = torch.cat((null_kv[1].expand(B, 1, D), kv[:, D:].reshape(B, N, D)), dim=1)
    s = torch.einsum("bhid,bjd->bhij", qh, k) * SCALE
    return torch.einsum("bhij,bjd->bhid", s.softmax(-1), v).transpose(1, 2).reshape(B * N, H * D)
