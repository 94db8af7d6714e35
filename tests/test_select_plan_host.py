"""What the epsilon-greedy selection reads, without a GPU (toric-rl-decoder_amd/csrc/select_plan.hpp built with g++ through
tests/host_select_plan_shim.cpp), against the oracle's selection on the full Q-table: the plan lists exactly the rows the
oracle reads, and the selection over the compact table of those rows gives the oracle's actions and q_values in bits.
Exact; test-only build: the product itself has no CPU path."""
import numpy as np
import pytest

import select_plan_cases as S

D = 7
NQ = 2 * D * D
SEED = 90210
COUNTS = (0, 1, 63, 64, 65, NQ)               # perspectives per lattice: none, one, around the wavefront's 64, all 2 d^2


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return S.load_shim(tmp_path_factory)


@pytest.fixture(scope="module")
def case():
    """48 lattices, every count of COUNTS eight times in a shuffled order, with (episode, step) counters of their own; a
    Q-table of few distinct values, so that every slice has its maximum many times (forced ties), a third of the
    slices' maxima in the last row as well."""
    rng = np.random.default_rng(48)
    counts = rng.permutation(np.repeat(COUNTS, 8))
    n = counts.size
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    P = int(offsets[-1])
    q = rng.integers(-3, 4, (P, 3)).astype(np.float32) * 0.25
    for i in range(0, n, 3):
        if counts[i]:
            q[offsets[i + 1] - 1, 2] = 1.0                   # a later, larger maximum: the first maximum is not always early
    pos = rng.integers(0, D, (P, 3)).astype(np.int32)
    return dict(n=n, counts=counts, offsets=offsets, q=q, pos=pos, env_ids=np.arange(n) + 1000,
                episodes=rng.integers(0, 50, n).astype(np.uint32), steps=rng.integers(0, 75, n).astype(np.uint32))


def eps_settings(n):
    return {"all 0": np.zeros(n), "all 1": np.ones(n), "0.3": np.full(n, 0.3), "reference schedule": S.reference_eps(n)}


def test_need(shim):
    for n in (0, 1, 2, 63, 64, 65, NQ):
        assert shim.shim_need(n, 1) == n
        assert shim.shim_need(n, 0) == (1 if n else 0)


@pytest.mark.parametrize("name", list(eps_settings(1)))
def test_plan_is_what_the_oracle_reads_and_selects_the_same(shim, case, name):
    c = case
    eps = eps_settings(c["n"])[name]
    act, qv, reads = S.oracle_reads(c["q"], c["offsets"], c["pos"], eps, SEED, c["env_ids"], c["episodes"], c["steps"])
    need, poff, rows, R = S.host_plan(shim, c["offsets"], eps, c["episodes"], c["steps"], SEED, first_env=1000)
    assert R == int(need.sum()) == int(poff[-1]) == reads.size
    assert np.array_equal(poff, np.concatenate([[0], np.cumsum(need)]))
    assert np.array_equal(rows[:R], reads)
    assert (np.diff(rows[:R]) > 0).all()
    assert (rows[R:] == S.ROWS_UNWRITTEN).all()
    greedy = S.oracle_greedy(eps, SEED, c["env_ids"], c["episodes"], c["steps"])
    assert np.array_equal(need, np.where(c["counts"] == 0, 0, np.where(greedy, c["counts"], 1)))
    if name == "all 0":
        assert greedy.all() and np.array_equal(rows[:R], np.arange(c["offsets"][-1]))
    if name == "all 1":
        assert not greedy.any() and R == int((c["counts"] > 0).sum())
    if name in ("0.3", "reference schedule"):
        multi = c["counts"] > 1
        assert greedy[multi].any() and not greedy[multi].all() and R < c["offsets"][-1]
    got_act, got_qv, bad = S.host_select_planned(shim, c["q"][rows[:R]], c["offsets"], poff, c["pos"], eps, c["episodes"],
                                                 c["steps"], SEED, first_env=1000)
    assert bad == 0
    assert np.array_equal(got_act, act)
    assert np.array_equal(got_qv.view(np.uint32), qv.view(np.uint32))
    assert (got_act[c["counts"] == 0] == 0).all() and (got_qv[c["counts"] == 0] == 0).all()


def test_the_ties_and_the_late_maxima_are_there(case):
    """the greedy lattices' choice is a first maximum that the table holds more than once, and not always in row 0"""
    c = case
    act, qv, chosen = S.O.select_action_batch(c["q"], c["offsets"], c["pos"], 0.0, SEED, c["env_ids"], c["episodes"], c["steps"])
    tied = late = 0
    for i in range(c["n"]):
        sl = c["q"][c["offsets"][i]:c["offsets"][i + 1]]
        if sl.size:
            tied += int((sl == sl.max()).sum() > 1)
            late += int(chosen[i] > c["offsets"][i])
    assert tied >= 20 and late >= 10


def test_a_short_row_buffer_leaves_the_tail_unwritten(shim, case):
    c = case
    eps = S.reference_eps(c["n"])
    _, _, full, R = S.host_plan(shim, c["offsets"], eps, c["episodes"], c["steps"], SEED, first_env=1000)
    _, poff, rows, R2 = S.host_plan(shim, c["offsets"], eps, c["episodes"], c["steps"], SEED, first_env=1000, rows_cap=R - 1)
    assert R2 == R == int(poff[-1]) and rows.size == R - 1
    assert np.array_equal(rows, full[:R - 1])


def test_a_plan_made_with_another_eps_or_before_a_step_is_detected(shim, case):
    c = case
    n = c["n"]
    eps_a, eps_b = S.reference_eps(n), S.reference_eps(n)[::-1].copy()
    need_a, poff, rows, R = S.host_plan(shim, c["offsets"], eps_a, c["episodes"], c["steps"], SEED, first_env=1000)
    need_b = S.host_plan(shim, c["offsets"], eps_b, c["episodes"], c["steps"], SEED, first_env=1000)[0]
    differ = need_a != need_b
    assert differ.sum() >= 3
    act_a, qv_a, bad_a = S.host_select_planned(shim, c["q"][rows[:R]], c["offsets"], poff, c["pos"], eps_a, c["episodes"],
                                               c["steps"], SEED, first_env=1000)
    act, qv, bad = S.host_select_planned(shim, c["q"][rows[:R]], c["offsets"], poff, c["pos"], eps_b, c["episodes"], c["steps"],
                                         SEED, first_env=1000)
    assert bad_a == 0 and bad == int(differ.sum())
    assert (act[differ] == 0).all() and (qv[differ] == 0).all()
    # a step between plan and selection: the counters moved on, the draws are others
    need_c = S.host_plan(shim, c["offsets"], eps_a, c["episodes"], c["steps"] + 1, SEED, first_env=1000)[0]
    moved = need_a != need_c
    assert moved.sum() >= 3
    act, qv, bad = S.host_select_planned(shim, c["q"][rows[:R]], c["offsets"], poff, c["pos"], eps_a, c["episodes"],
                                         c["steps"] + 1, SEED, first_env=1000)
    assert bad == int(moved.sum()) and (act[moved] == 0).all()


def test_the_shim_decides_greedy_like_the_oracle(shim):
    rng = np.random.default_rng(5)
    n = 4000
    env, ep, st = rng.integers(0, 2 ** 32, n), rng.integers(0, 1000, n), rng.integers(0, 76, n)
    eps = rng.random(n)
    want = S.oracle_greedy(eps, SEED, env, ep, st)
    got = np.array([shim.shim_greedy(SEED, int(env[i]), int(ep[i]), int(st[i]), float(eps[i])) for i in range(n)], bool)
    assert np.array_equal(got, want) and 0.3 < want.mean() < 0.7
