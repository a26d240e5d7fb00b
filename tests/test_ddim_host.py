"""ddim_time_pairs (host code, no GPU): the (time, time_next) pairs of the DDIM
loop.  The expected lists are what the reference's expression gives
(dalle2_video.py:1787-1791: linspace(0, T, S + 2)[:-1] -> int -> reversed ->
consecutive pairs with time > time_next)."""
import pytest


def test_pairs_20_over_6():
    from dalle2_video.dalle2_video import ddim_time_pairs

    assert ddim_time_pairs(20, 6) == [(17, 14), (14, 11), (11, 8), (8, 5), (5, 2), (2, 0)]


def test_pairs_7_over_6_are_consecutive_steps():
    from dalle2_video.dalle2_video import ddim_time_pairs

    assert ddim_time_pairs(7, 6) == [(6, 5), (5, 4), (4, 3), (3, 2), (2, 1), (1, 0)]


def test_pairs_1000_over_250():
    from dalle2_video.dalle2_video import ddim_time_pairs

    pairs = ddim_time_pairs(1000, 250)
    assert len(pairs) == 250
    assert pairs[:3] == [(996, 992), (992, 988), (988, 984)]
    assert pairs[-2:] == [(7, 3), (3, 0)]


@pytest.mark.parametrize("T", [2, 7, 12, 20, 250, 1000])
def test_pairs_strictly_decreasing_and_end_at_zero(T):
    from dalle2_video.dalle2_video import ddim_time_pairs

    for S in sorted({1, 2, 3, 4, T // 3, T // 2, T - 2, T - 1}):
        if not 1 <= S < T:
            continue
        pairs = ddim_time_pairs(T, S)
        assert 1 <= len(pairs) <= S, (T, S)
        assert all(isinstance(t, int) and isinstance(tn, int) for t, tn in pairs)
        assert all(0 <= tn < t < T for t, tn in pairs), (T, S, pairs)
        assert all(a[1] == b[0] for a, b in zip(pairs[:-1], pairs[1:])), (T, S, pairs)
        assert pairs[-1][1] == 0, (T, S, pairs)
