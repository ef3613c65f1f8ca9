"""dp_model.checkpoint_plan / checkpoint_steps_for: the pure planning half of the checkpointed rollout adjoint (no GPU, no library)."""
import random

import pytest

import helpers  # noqa: F401  (puts the package on sys.path)


def _plan(T, frames, K):
    from diffphys_amd.dp_model import checkpoint_plan

    return checkpoint_plan(T, frames, K)


def test_plan_T_a_multiple_of_K():
    launch, segs = _plan(12, [0, 6, 12], 4)
    assert launch == [0, 6, 12, 4, 8]
    assert segs == [(0, 4, [0, 4], [0], True), (4, 8, [2, 4], [1], True), (8, 12, [4], [2], False)]


def test_plan_T_not_a_multiple_and_K_not_a_multiple_of_4():
    launch, segs = _plan(10, [3, 10, 7], 7)   # caller order is kept, frame 7 sits ON the boundary: state 0 of the later segment
    assert launch == [3, 10, 7]
    assert segs == [(0, 7, [3, 7], [0], True), (7, 10, [3, 0], [1, 2], False)]
    launch, segs = _plan(16, [0, 16], 5)
    assert launch == [0, 16, 5, 10, 15]
    assert [s[:2] for s in segs] == [(0, 5), (5, 10), (10, 15), (15, 16)]
    assert segs[0] == (0, 5, [0, 5], [0], True) and segs[1] == (5, 10, [5], [], True)
    assert segs[3] == (15, 16, [1], [1], False)


def test_plan_frames_on_boundaries_at_zero_and_at_T():
    launch, segs = _plan(8, [0, 4, 8], 4)
    assert launch == [0, 4, 8]                  # every boundary is a frame already: nothing added
    assert segs == [(0, 4, [0, 4], [0], True), (4, 8, [0, 4], [1, 2], False)]
    # the boundary frame is seeded once, by the later segment; the earlier one sees only the carry there
    assert sum(1 in s[3] for s in segs) == 1


def test_plan_empty_frame_list():
    launch, segs = _plan(9, [], 4)
    assert launch == [4, 8]
    assert segs == [(0, 4, [4], [], True), (4, 8, [4], [], True), (8, 9, [], [], False)]


@pytest.mark.parametrize("K", [10, 11, 1000])
def test_plan_K_at_least_T_is_todays_call(K):
    frames = [0, 5, 10, 2]
    launch, segs = _plan(10, frames, K)
    assert launch == frames
    assert segs == [(0, 10, frames, [0, 1, 2, 3], False)]


def test_plan_refuses_nonsense():
    for T, frames, K in ((10, [0], 0), (10, [0], -3), (10, [11], 4), (10, [2, 2], 4), (10, [-1], 4)):
        with pytest.raises(ValueError):
            _plan(T, frames, K)


def test_plan_invariants_on_random_cases():
    rng = random.Random(7)
    for _ in range(400):
        T = rng.randint(1, 120)
        K = rng.randint(1, T + 5)
        frames = rng.sample(range(T + 1), rng.randint(0, min(T + 1, 9)))
        launch, segs = _plan(T, frames, K)
        # the segments tile [0, T)
        assert segs[0][0] == 0 and segs[-1][1] == T
        assert all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
        assert all(0 < e - s <= K for s, e, _, _, _ in segs)
        assert all(e - s == K for s, e, _, _, _ in segs[:-1])
        # every caller frame is seeded in exactly one segment, at its own step
        seen = []
        for i, (s, e, local, idx, carry) in enumerate(segs):
            assert carry == (i < len(segs) - 1)
            assert len(local) == len(idx) + (1 if carry else 0)
            assert [frames[j] - s for j in idx] == local[:len(idx)]
            if carry:
                assert local[-1] == e - s
            assert len(set(local)) == len(local) and all(0 <= x <= e - s for x in local)   # a list the library accepts
            assert idx == sorted(idx)                                                       # the caller's order
            seen += idx
        assert sorted(seen) == list(range(len(frames)))
        # the launch list: the caller's frames first and in order, then the missing boundaries; no step twice, all in range
        assert launch[:len(frames)] == frames
        assert len(set(launch)) == len(launch) and all(0 <= x <= T for x in launch)
        assert set(launch) == set(frames) | set(range(K, T, K))


def test_steps_for_edges_and_monotony():
    from diffphys_amd.dp_model import checkpoint_steps_for

    T, a, b = 100, 1000, 50
    need = lambda K: K * a + -(-T // K) * b
    assert checkpoint_steps_for(T, a, b, need(100)) == 100          # the whole horizon fits exactly
    assert checkpoint_steps_for(T, a, b, need(100) - 1) == 99
    assert checkpoint_steps_for(T, a, b, 10 ** 12) == 100           # never more than the horizon
    for K in (1, 7, 33, 50):
        got = checkpoint_steps_for(T, a, b, need(K))
        assert got >= K and need(got) <= need(K)                   # exact at the edge: K itself fits, nothing larger is passed over
        assert all(need(k) > need(K) for k in range(got + 1, T + 1))
    prev = 0
    for budget in range(need(1), need(100) + 2000, 777):
        K = checkpoint_steps_for(T, a, b, budget)
        assert K >= prev and need(K) <= budget
        prev = K


def test_steps_for_names_the_shortfall():
    from diffphys_amd.dp_model import checkpoint_steps_for

    T, a, b = 100, 1000, 50
    cheapest = min(K * a + -(-T // K) * b for K in range(1, T + 1))
    with pytest.raises(ValueError) as e:
        checkpoint_steps_for(T, a, b, cheapest - 123)
    assert "123 bytes short" in str(e.value)
    assert checkpoint_steps_for(T, a, b, cheapest) >= 1
    with pytest.raises(ValueError):
        checkpoint_steps_for(0, a, b, 10 ** 9)
