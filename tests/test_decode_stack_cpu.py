"""CPU: hop_decode_stack_schedule (host/hop_decode.cpp, hop_dec_plan_stack) -- the plan hop_decode_stack runs, on the partition data the CPU spine gives three
192x128 pictures (test_spine_cpu.frame).

Every picture is planned alone and the plans are merged by level: picture k's levels are hop_decode_schedule's of that picture, the number of launches is the maximum
over the pictures (not the sum), raster order runs CTU a of every picture in launch a, and a malformed unit is refused with its picture in the text."""
import numpy as np
import pytest

from test_decode_host import coded, hophip

W, H = 192, 128
SEEDS = (7, 5, 1234)                      # (7 is one of test_decode_host's own cases: coded() keeps it)


@pytest.fixture(scope="module")
def stack_parts():
    return np.concatenate([coded(("frame", W, H, seed, False))[2] for seed in SEEDS])


def test_levels_are_each_pictures_own_and_the_count_is_the_maximum(stack_parts):
    n = stack_parts.shape[0] // len(SEEDS)
    assert n == 6
    for schedule in (0, 1):
        lv, nl = hophip.decode_stack_schedule(W, H, len(SEEDS), stack_parts, schedule)
        alone = [hophip.decode_schedule(W, H, stack_parts[k * n:(k + 1) * n], schedule) for k in range(len(SEEDS))]
        assert lv.shape == (len(SEEDS), n)
        for k, (want, _) in enumerate(alone):
            assert np.array_equal(lv[k], want), (schedule, k, lv[k], want)
        assert nl == max(a[1] for a in alone), (schedule, nl, [a[1] for a in alone])
        assert nl < sum(a[1] for a in alone)
        if schedule == 1:
            assert nl == n and all(np.array_equal(lv[k], np.arange(n)) for k in range(len(SEEDS)))
    # one picture: hop_decode_schedule itself
    lv1, nl1 = hophip.decode_stack_schedule(W, H, 1, stack_parts[:n], 0)
    want, nw = hophip.decode_schedule(W, H, stack_parts[:n], 0)
    assert np.array_equal(lv1[0], want) and nl1 == nw


def test_a_malformed_unit_names_its_picture(stack_parts):
    n = stack_parts.shape[0] // len(SEEDS)
    intra = np.argwhere(stack_parts[2 * n:]["pred_mode"] == 1)
    assert len(intra)
    a, u = intra[0]
    bad = stack_parts.copy()
    bad[2 * n + a]["luma_dir"][u] = 35
    with pytest.raises(hophip.HopError) as e:
        hophip.decode_stack_schedule(W, H, len(SEEDS), bad, 0)
    assert "picture 2" in str(e.value) and "CTU %d unit %d" % (a, u) in str(e.value), e.value
    # the same unit in a stack of one carries hop_decode_schedule's own text: no picture to name
    with pytest.raises(hophip.HopError) as e:
        hophip.decode_stack_schedule(W, H, 1, bad[2 * n:], 0)
    assert "picture" not in str(e.value) and "CTU %d unit %d" % (a, u) in str(e.value), e.value
    hophip.decode_stack_schedule(W, H, len(SEEDS), stack_parts, 0)
    with pytest.raises(hophip.HopError):
        hophip.decode_stack_schedule(W, H, len(SEEDS), stack_parts, 2)
    with pytest.raises(hophip.HopError):
        hophip.decode_stack_schedule(W, H, 0, stack_parts[:0], 0)
