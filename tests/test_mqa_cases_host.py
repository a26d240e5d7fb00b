"""The closed forms of tests/mqa_cases.py against a float64 softmax attention
(forward and autograd backward), on the CPU.  This is what entitles
tests/test_mqa_exact_gpu.py to use the closed forms at clip lengths where a
float64 score matrix would not fit."""
import math

import pytest
import torch

import mqa_cases as mc

B = 2
HOST_NS = (31, 32, 97, 160)
# every clip length the GPU test uses (kept equal to its list by a test below)
GPU_NS = (31, 32, 95, 96, 97, 160, 1279, 1280, 1535, 1536)
FAMILIES = tuple(str(c) for c in mc.FLAT_LEVELS) + ("select",)


def _run_reference(case):
    leaves = [t.clone().requires_grad_() for t in (case.q, case.kv, case.null_kv)]
    o = mc.reference(*leaves, case.B, case.N)
    (o * mc.upstream(case.B, case.N)).sum().backward()
    return o.detach(), [t.grad for t in leaves]


def _maxdiff(a, b):
    return float((a - b).abs().max())


@pytest.mark.parametrize("N", HOST_NS)
@pytest.mark.parametrize("family", FAMILIES)
def test_closed_forms_match_float64_attention(family, N):
    case = mc.build(family, B, N)
    o, (dq, dkv, dnull) = _run_reference(case)
    assert _maxdiff(o, case.o) <= 1e-12
    assert _maxdiff(dkv[:, mc.D:], case.dv) <= 1e-9
    assert _maxdiff(dnull[1], case.dnull_v) <= 1e-9
    if case.dq is not None:
        assert _maxdiff(dq, case.dq) <= 1e-9
        assert _maxdiff(dkv, case.dkv) <= 1e-9
        assert _maxdiff(dnull, case.dnull) <= 1e-9


@pytest.mark.parametrize("family", FAMILIES)
def test_inputs_are_exact_in_bf16_and_values_in_e4m3(family):
    case = mc.build(family, B, 97)
    for t in (case.q, case.kv, case.null_kv, mc.upstream(B, 97)):
        assert torch.equal(t.float().bfloat16().double(), t)
    assert set(case.kv[:, mc.D:].unique().tolist()) <= {0.0, 1.0}


@pytest.mark.parametrize("N", GPU_NS)
def test_selection_covers_every_key_with_a_wide_gap(N):
    pi = mc.sel_pi(B, N)
    assert math.gcd(mc.sel_a(N), N + 1) == 1
    for b in range(B):
        assert torch.equal(pi[b].unique(), torch.arange(N + 1))  # hits every key index 0..N
    assert (pi.reshape(B, N, mc.H).sort(-1).values.diff(dim=-1) != 0).all()  # heads of a token differ
    assert not torch.equal(pi[0], pi[1])
    assert mc.selection_gap_log2(B, N) >= 40.0
    # the online regime: |q| |k'| far past the bounded-score limit
    assert mc.SEL_QMAG * mc.D * mc.bf16_key_unit() > mc.FIX_BOUND
    # value rows decode to the code of the key they sit at, and clips differ past the null key
    codes = mc.key_codes(B, N)
    assert torch.equal(mc.decode_v(mc.code_v(codes)), codes)
    assert (codes[0, 1:] != codes[1, 1:]).all() and codes.max() < 2 ** mc.NBITS
    for b in range(B):
        assert codes[b].unique().numel() == N + 1


def test_flat_levels_sit_on_the_intended_side_of_the_score_bound():
    for c, bounded in ((0, True), (32, True), (-32, True), (64, False), (-64, False)):
        bound = mc.flat_score_bound(c)
        assert (bound <= mc.FIX_BOUND) == bounded, (c, bound)
        assert abs(bound - abs(c) * 46.25 / 32) < 1e-9  # 46.25 / 92.5 log2 units
    # the only probability value that is no power of two: exp2(+-46.25) in the bounded regime
    assert mc.flat_p_rounding(0) == 0 and mc.flat_p_rounding(64) == 0 and mc.flat_p_rounding(-64) == 0
    assert 1e-3 < mc.flat_p_rounding(32) < 2.0 ** -8 and 1e-3 < mc.flat_p_rounding(-32) < 2.0 ** -8


def test_gpu_test_uses_the_lengths_checked_here():
    import test_mqa_exact_gpu as g

    assert tuple(g.NS) == GPU_NS and g.B == B
    assert {mc.nkp(N) for N in GPU_NS if mc.nkp(N) == N + 1} == {32, 96, 1280, 1536}  # no pad keys
