"""The forced alignment kernels' formulation on the CPU (tests/align_formulation.py): the
lane-by-lane restatements of both kernel forms equal the plain rule bit for bit, and the plain
rule finds the best path (brute-force enumeration on tiny cases)."""
import numpy as np
import pytest

import align_formulation as AF


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return np.array_equal(a[0], b[0]) and np.float32(a[1]).tobytes() == np.float32(b[1]).tobytes()


def test_plain_rule_is_the_best_path_on_tiny_cases():
    rng = np.random.default_rng(7)
    n_checked = 0
    for T in range(1, 7):
        for L in range(0, 4):
            for _ in range(6):
                logp, y = AF.random_case(rng, T, L, 3, repeats=0.4)
                got = AF.ctc_align(logp, y)
                ref = AF.brute_force(logp, y)
                if ref is None:
                    assert got is None and not AF.feasible(T, y)
                    continue
                assert got is not None
                best, paths = ref
                assert AF.collapse(got[0]) == y
                assert abs(got[1] - best) < 1e-4
                if len(paths) == 1:
                    assert tuple(got[0]) == paths[0]
                # fp64 gives the same path: no decision hangs on fp32 rounding here
                assert np.array_equal(AF.ctc_align(logp, y, dt=np.float64)[0], got[0])
                n_checked += 1
    assert n_checked > 60


def test_ties_go_to_stay_then_step_then_skip_and_to_the_last_label():
    # constant rows: every path has the same score; the rule must pick one deterministically
    logp = np.full((6, 4), np.float32(np.log(0.25)), np.float32)
    path, score = AF.ctc_align(logp, [1, 2])
    # ends in the last label (the trailing blank is not strictly better); stays as long as it can
    assert AF.collapse(path) == [1, 2]
    assert path[-1] == 2
    assert _same(AF.wave_form(logp, [1, 2]), (path, score))
    assert _same(AF.block_form(logp, [1, 2]), (path, score))


@pytest.mark.parametrize('NS', [1, 2, 4])
def test_wave_form_equals_the_plain_rule(NS):
    rng = np.random.default_rng(100 + NS)
    max_L = (64 * NS - 1) // 2
    cases = [(1, 0), (5, 0), (1, 1), (2, 1), (3, 2), (40, 7), (70, 31), (90, min(max_L, 40)),
             (160, max_L), (2 * max_L + 1, max_L)]
    for T, L in cases:
        if L > max_L:
            continue
        logp, y = AF.random_case(rng, T, L, 11)
        assert _same(AF.wave_form(logp, y, NS=NS), AF.ctc_align(logp, y)), (T, L)
    # exactly feasible, and one frame short (status 1)
    for L in (1, 2, 9, max_L):
        logp, y = AF.random_case(rng, 400, L, 5, repeats=0.5)
        need = L + AF.repeats_of(y)
        ok = AF.wave_form(logp[:need], y, NS=NS)
        assert ok is not None and _same(ok, AF.ctc_align(logp[:need], y))
        assert AF.collapse(ok[0]) == y
        assert AF.wave_form(logp[:need - 1], y, NS=NS) is None
        assert AF.ctc_align(logp[:need - 1], y) is None


def test_wave_form_with_a_nonzero_blank():
    rng = np.random.default_rng(5)
    logp, y = AF.random_case(rng, 50, 12, 9, blank=4)
    assert 4 not in y
    assert _same(AF.wave_form(logp, y, blank=4), AF.ctc_align(logp, y, blank=4))
    assert _same(AF.block_form(logp, y, blank=4), AF.ctc_align(logp, y, blank=4))


def test_block_form_equals_the_plain_rule_beyond_the_fast_form():
    rng = np.random.default_rng(11)
    for T, L in [(1, 0), (3, 1), (30, 9), (300, 128), (420, 200), (333, 150)]:
        logp, y = AF.random_case(rng, T, L, 13)
        assert 2 * L + 1 > AF.FAST_S or L < 128
        # what the kernel never writes (back pointers outside the band, frame 0) is never read
        assert _same(AF.block_form(logp, y, junk=rng), AF.ctc_align(logp, y)), (T, L)
    logp, y = AF.random_case(rng, 600, 140, 6, repeats=0.5)
    need = 140 + AF.repeats_of(y)
    assert _same(AF.block_form(logp[:need], y, junk=rng), AF.ctc_align(logp[:need], y))
    assert AF.block_form(logp[:need - 1], y) is None


def test_dispatch_picks_the_form_by_the_state_count():
    rng = np.random.default_rng(3)
    for L in (127, 128):
        logp, y = AF.random_case(rng, 300, L, 7)
        assert _same(AF.kernel_form(logp, y), AF.ctc_align(logp, y))
