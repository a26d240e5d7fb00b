"""The closed forms of tests/gn_cases.py against torch.nn.functional.group_norm
in float64 (FiLM, activation and residual applied, gradients by autograd), the
exactness conditions of the two-level family, and the kernels' forward
arithmetic evaluated in f32 on the CPU -- which is what entitles
tests/test_gn_exact_gpu.py to ask for bit-exact results."""
import numpy as np
import pytest
import torch

import gn_cases as gc

ROW_IDS = sorted(gc.ROWS)
VARIANTS = [(act, film, res) for act in (gc.ACT_NONE, gc.ACT_SILU) for film in (False, True) for res in (False, True)]


def _relmax(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("row", ROW_IDS)
def test_two_level_closed_forms_match_float64_group_norm(row):
    case = gc.build("two", *gc.ROWS[row])
    for act, film, res in VARIANTS:
        exp, ref = case.expect(act, film, res), gc.reference(case, act, film, res)
        for k in ref:
            assert _relmax(exp[k], ref[k]) <= 1e-12, (row, act, film, res, k, _relmax(exp[k], ref[k]))
    # mean / rstd: the closed form is the data's own statistics
    zg = case.z.reshape(case.nb, case.P, case.G, case.cg)
    assert torch.equal(zg.mean((1, 3)), case.m)
    assert torch.equal((zg * zg).mean((1, 3)) - case.m * case.m, case.s * case.s)


@pytest.mark.parametrize("shape", [gc.ROWS["1"], gc.ROWS["5"], gc.ROWS["8f"]])
def test_gaussian_formula_matches_float64_group_norm(shape):
    case = gc.build("gauss", *shape)
    for act, film, res in VARIANTS:
        exp, ref = case.expect(act, film, res), gc.reference(case, act, film, res)
        for k in ref:
            assert _relmax(exp[k], ref[k]) <= 1e-10, (shape, act, film, res, k)


@pytest.mark.parametrize("shape", [gc.ROWS[r] for r in ROW_IDS] + [(gc.PRESUM_NB, gc.PRESUM_P, C, G) for C, G, _ in
                                                                    gc.PRESUM[::3]] + gc.COOP)
def test_exactness_conditions(shape):
    nb, P, C, G = shape
    case = gc.build("two", *shape)
    case.check_exact()  # half / half, the 2^24 bounds, P * C/G even
    j = case.m / case.s
    assert float(j.abs().max()) == 8 and bool((j == j.round()).all())  # the offset case is present
    assert set(case.s.unique().tolist()) <= {0.25, 0.5, 1.0, 2.0}
    # neighbouring clips and groups differ in centre and in width
    for t in (case.m, case.s):
        assert bool((t[:, 1:] != t[:, :-1]).all()) and bool((t[1:] != t[:-1]).all())
    # every input is exact in bf16, |v| <= 8 (the SiLU bound's range)
    for t in (case.z, case.res, case.dy):
        assert torch.equal(t.bfloat16().double(), t)
    assert float(case.expect(gc.ACT_NONE, True, False)["v"].abs().max()) <= 8
    # the sign pattern has no period in rows per pass, 64 lanes or 8 channels: shifted copies agree on about half
    sg = case.sigma
    for dp in (1, 2, 4, 8, 32, 42, 64, 128, 256):
        if dp < P:
            agree = float((sg[:, dp:] == sg[:, :-dp]).double().mean())
            assert 0.4 < agree < 0.6, (dp, agree)
    for dc in (1, 4, 8, 64):
        if dc < C and P * (C - dc) >= 2000:
            agree = float((sg[:, :, dc:] == sg[:, :, :-dc]).double().mean())
            assert 0.4 < agree < 0.6, (dc, agree)
    # parameters vary with clip and channel
    assert case.gamma.unique().numel() >= 4 and not torch.equal(case.ss[0], case.ss[1])
    assert float(case.res.min()) >= 0.5


@pytest.mark.parametrize("row", ROW_IDS)
def test_kernel_forward_arithmetic_is_exact_in_f32(row):
    """A = rs g (1 + sc), B = (beta - mu rs g)(1 + sc) + sh, y = fma(z, A, B) (+ res), every
    step rounded to f32 as the kernels do: equal to the closed form bit for bit (act NONE).
    z A is exact, so the fused and the unfused multiply-add agree."""
    case = gc.build("two", *gc.ROWS[row])
    f = np.float32
    for film in (False, True):
        for res in (False, True):
            sc, sh = case.film(film)
            rs = f(case.per_channel(1 / case.s).numpy())
            mu = f(case.per_channel(case.m).numpy())
            g, bt = f(case.gamma.numpy())[None, None, :], f(case.beta.numpy())[None, None, :]
            sc, sh = f(sc.numpy())[:, None, :], f(sh.numpy())[:, None, :]
            A = rs * g * sc
            B = (bt - mu * rs * g) * sc + sh
            z = f(case.z.numpy())
            prod = z * A
            assert prod.dtype == f and np.array_equal(prod.astype(np.float64), z.astype(np.float64) * A.astype(np.float64))
            y = prod + B
            if res:
                y = y + f(case.res.numpy())
            assert y.dtype == f
            want = case.expect(gc.ACT_NONE, film, res)["y"].numpy()
            assert np.array_equal(y.astype(np.float64), want), (row, film, res)
            # the statistics the kernels derive in double from exact sums
            n = float(case.P * case.cg)
            zg = case.z.reshape(case.nb, case.P, case.G, case.cg)
            s1, s2 = zg.sum((1, 3)).numpy(), (zg * zg).sum((1, 3)).numpy()
            m = s1 / n
            assert np.array_equal(f(m), f(case.m.numpy()))
            assert np.array_equal(f(1.0 / np.sqrt(s2 / n - m * m)), f((1 / case.s).numpy()))


@pytest.mark.parametrize("C,G,R", gc.PRESUM)
def test_presummed_statistics_are_exact_and_uneven(C, G, R):
    case = gc.build("two", gc.PRESUM_NB, gc.PRESUM_P, C, G)
    parts = gc.presums(case, R)
    assert parts.shape == (R, case.nb, C, 2)
    assert torch.equal(parts.float().double(), parts)  # every part is an f32 value
    assert torch.equal(parts.sum(0)[..., 0], case.z.sum(1))
    assert torch.equal(parts.sum(0)[..., 1], (case.z * case.z).sum(1))
    # f32 summation in the two orders the kernels use (ascending; 8 at a time) is exact
    p32 = parts.float()
    acc = torch.zeros_like(p32[0])
    for r in range(R):
        acc = acc + p32[r]
    assert torch.equal(acc.double(), parts.sum(0))
    if R >= 3:
        assert float(parts[1].abs().max()) == 0 and float(parts[0].abs().max()) > 0
        assert not torch.equal(parts[0], parts[2])


def test_gpu_test_uses_the_cases_checked_here():
    import test_gn_exact_gpu as g

    assert g.gc is gc and sorted(g.ROW_DTYPES) == ROW_IDS
    assert set(g.PRESUM_DQ) == set(gc.PRESUM) and {s[:3] for s in gc.COOP} == set(g.COOP_PLAN)
    g.test_rows_reach_the_paths_the_table_names()  # the launch facts need no GPU
