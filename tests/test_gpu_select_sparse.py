"""The planned selection on the GPU (tq_select_plan, tq_nn11_forward_rows, tq_select_action_planned and the Python surface
over them): the device plan against the g++ build of csrc/select_plan.hpp, the gathering forward against the plain one,
and sparse against dense end to end -- everything in bits."""
import ctypes as C
import os

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")             # no exhaustive solver search per batch shape on a fresh box

import numpy as np
import pytest
import torch

import nn11_cases as K
import select_plan_cases as S

pytestmark = pytest.mark.gpu
DTYPES = (torch.uint8, torch.float32, torch.float16, torch.bfloat16)
FIRST_ENV = 5000


@pytest.fixture(scope="module")
def T():
    import toric_rl_decoder_amd as T
    assert torch.cuda.is_available()
    T.load()
    return T


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return S.load_shim(tmp_path_factory)


def make_envs(T, d, n, seed, first_env_id=0, probe=False):
    envs = T.EnvSet(T.make("toric-code-v0", {"size": d, "p_error": 0.1}), n, seed=seed, first_env_id=first_env_id, numpy_io=False)
    if not probe:
        envs.REUSED_PROBE_CANDIDATES = 0                        # generatePerspectiveReused without its one-off buffer probe
    envs.resetAll()
    return envs


def counters(envs):
    ep, st = envs.getCounters()
    return ep.cpu().numpy().astype(np.uint32), st.cpu().numpy().astype(np.uint32)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------ 1. the plan
@pytest.mark.parametrize("d,n", [(d, n) for d in (3, 5, 7) for n in (1, 64, 65, 2049)])
def test_device_plan_is_the_shims(T, shim, d, n):
    """2049 lattices are one past the scan's chunk of 2048.  Two exploration steps give the lattices counters of their
    own; every fifth lattice (not the first) is emptied."""
    seed = 1000 * d + n
    envs = make_envs(T, d, n, seed, first_env_id=FIRST_ENV)
    for _ in range(2):
        envs.actorStep(None)
    q = envs.getQubits().clone()
    empty = np.arange(n) % 5 == 4
    q[torch.from_numpy(empty).cuda()] = 0
    envs.setQubits(q)
    counts, offsets = envs.perspectiveCounts()
    counts, off = counts.cpu().numpy(), offsets.cpu().numpy()
    assert ((counts == 0) == empty).all()
    P = int(off[-1])
    ep, st = counters(envs)
    settings = {"all 0": np.zeros(n), "all 1": np.ones(n), "0.3": np.full(n, 0.3), "reference schedule": S.reference_eps(n)}
    for name, eps in settings.items():
        need, poff, rows, R = S.host_plan(shim, off, eps, ep, st, seed, first_env=FIRST_ENV)
        plan = envs.selectPlan(eps)
        assert plan.R == R == int(need.sum()), (name, plan.R, R)
        assert np.array_equal(plan.plan_offsets.cpu().numpy(), poff), name
        got = plan.rows.cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, rows[:R]), name
        assert (np.diff(got) > 0).all()
        if name == "all 0":
            assert np.array_equal(got, np.arange(P))
        if name == "all 1":
            assert R == int((counts > 0).sum())
    envs.check()
    # a row buffer one too short: the head as before, nothing at or past the capacity, TQ_E_CAPACITY at check()
    eps = settings["reference schedule"]
    need, poff, rows, R = S.host_plan(shim, off, eps, ep, st, seed, first_env=FIRST_ENV)
    if R >= 1:
        L = T.load()
        buf = torch.full((R + 8,), -7, dtype=torch.int32, device="cuda")
        dpoff = torch.zeros(n + 2, dtype=torch.int64, device="cuda")[:n + 1]
        deps = torch.from_numpy(eps).cuda()
        torch.cuda.synchronize()
        assert L.tq_select_plan(envs._h, _ptr(offsets), _ptr(deps), _ptr(dpoff), _ptr(buf), R - 1, None) == 0
        with pytest.raises(T.ToricEnvError, match="capacity"):
            envs.check()
        buf = buf.cpu().numpy()
        assert np.array_equal(buf[:R - 1], rows[:R - 1]) and (buf[R - 1:] == -7).all()
        assert int(dpoff[-1]) == R
        envs.check()                                            # the latch was cleared
    envs.close()


# ------------------------------------------------------------------------------------------------ 2. the gathering forward
def forward_case(d):
    sd = K.integer_state_dict(d) if d == 3 else K.trained_state_dict(d)
    g = K.group(d)
    per = K.stack_of(d, 64)[0][:4 * g + 9]
    assert per.shape[0] == 4 * g + 9
    return sd, g, per


@pytest.mark.parametrize("d", (3, 5, 7))
def test_forward_of_listed_rows_is_the_full_forward_at_those_rows(T, d):
    """A handle of G + 1 rows per pass, so that the list is cut into passes; lists of 1, G, G + 1 and 2 G + 3 rows in
    increasing order, and one shuffled list with repeats.  The integer network at d = 3 tells few perspectives apart
    (two distinct Q-rows), so a seeded random NN_11 follows it there, whose rows differ."""
    sd, g, per = forward_case(d)
    n = per.shape[0]
    f = T.NN11Forward(sd, d, "cuda", max_rows=g + 1)
    torch.manual_seed(3)
    nets = (sd, T.NN_11(d).state_dict()) if d == 3 else (sd,)
    rng = np.random.default_rng(70 + d)
    lists = [np.sort(rng.choice(n, k, replace=False)) for k in (1, g, g + 1, 2 * g + 3)]
    shuffled = rng.choice(n, 2 * g + 3, replace=True)
    shuffled[:4] = shuffled[4:8]                                # repeats for certain
    assert len(set(shuffled.tolist())) < shuffled.size and (np.diff(shuffled) < 0).any()
    lists.append(shuffled)
    for k, dt in enumerate(DTYPES if d == 5 else ((torch.float16, torch.bfloat16) if d == 3 else (torch.uint8,))):
        f.load(nets[k % len(nets)])
        x = torch.from_numpy(per).cuda().to(dt)
        full = f(x)
        assert d == 3 and k == 0 or torch.unique(full, dim=0).shape[0] > n // 2      # rows differ: a mix-up shows
        for rows in lists:
            r = torch.from_numpy(rows.astype(np.int32)).cuda()
            got = f(x, r)
            assert got.dtype == torch.float32 and tuple(got.shape) == (rows.size, 3)
            assert torch.equal(got, full[r.long()]), (d, dt, rows.size)
        assert tuple(f(x, torch.zeros(0, dtype=torch.int32, device="cuda")).shape) == (0, 3)
    f.check()
    with pytest.raises(ValueError, match="int32"):
        f(x, torch.zeros(3, dtype=torch.int64, device="cuda"))
    f.close()


# ------------------------------------------------------------------------------------------------ 3. a bad index
def test_an_index_outside_the_stack_is_latched_and_harms_no_other_row(T):
    d = 5
    sd, g, per = forward_case(d)
    n = per.shape[0]
    f = T.NN11Forward(sd, d, "cuda", max_rows=g + 1)
    x = torch.from_numpy(per).cuda()
    full = f(x)
    rows = np.arange(0, 2 * g + 3, dtype=np.int32) * 2 % n
    bad_at = g + 2                                              # in the second pass
    rows[bad_at] = n                                            # one past the last row
    got = f(x, torch.from_numpy(rows).cuda())
    with pytest.raises(ValueError, match="row index"):
        f.check()
    keep = np.arange(rows.size) != bad_at
    want = full[torch.from_numpy(rows[keep].astype(np.int64)).cuda()]
    assert torch.equal(got[torch.from_numpy(keep).cuda()], want)
    assert torch.equal(got[bad_at:bad_at + 1], f(torch.zeros_like(x[:1])))     # the Q-row of a zero perspective
    f.check()                                                   # read and cleared
    f.close()


# ------------------------------------------------------------------------------------------------ 4. selection, end to end
def oracle_row_count(envs, eps, seed):
    counts = envs.perspectiveCounts()[0].cpu().numpy()
    ep, st = counters(envs)
    greedy = S.oracle_greedy(eps, seed, np.arange(envs.no_envs) + envs.first_env_id, ep, st)
    return int(np.where(counts == 0, 0, np.where(greedy, counts, 1)).sum()), int(counts.sum())


@pytest.mark.parametrize("dtype", (torch.uint8, torch.float32))
def test_sparse_selection_is_the_dense_one_over_twenty_steps(T, dtype):
    d, n, seed = 5, 300, 414
    f = T.NN11Forward(K.trained_state_dict(d), d, "cuda", max_rows=1 << 12)
    dense, sparse = make_envs(T, d, n, seed), make_envs(T, d, n, seed)
    eps = S.reference_eps(n)
    fewer = 0
    for t in range(20):
        act_d, qv_d = T.selectActionEnvSet(dense, f, eps, dtype=dtype)
        act_s, qv_s = T.selectActionEnvSet(sparse, f, eps, dtype=dtype, sparse=True)
        assert torch.equal(act_d, act_s), t
        assert torch.equal(qv_d.view(torch.int32), qv_s.view(torch.int32)), t
        R = sparse.selectPlan(eps).R                            # the plan of this step again: the same draws
        want, P = oracle_row_count(sparse, eps, seed)
        assert R == want <= P, (t, R, want, P)
        fewer += R < P
        dense.actorStep(act_d)
        sparse.actorStep(act_s)
    assert fewer >= 1
    assert torch.equal(dense.getStates(), sparse.getStates())
    f.check()
    for e in (dense, sparse):
        e.check()
        e.close()
    f.close()


# ------------------------------------------------------------------------------------------------ 5. the actor loop
def test_run_actor_sparse_sends_the_same_blocks(T):
    d, n, seed, T_buf, flushes = 5, 300, 515, 4, 2
    f = T.NN11Forward(K.trained_state_dict(d), d, "cuda", max_rows=1 << 12)
    dense, sparse = make_envs(T, d, n, seed), make_envs(T, d, n, seed)
    eps = S.reference_eps(n)
    gd = T.run_actor(dense, f, flushes, T_buf, eps)
    gs = T.run_actor(sparse, f, flushes, T_buf, eps, sparse=True)
    for k in range(flushes):
        bd, bs = next(gd), next(gs)
        assert torch.equal(bd.buf, bs.buf), k                   # every section, the priorities included
        pr = bd.unpack()["priority"]
        assert bool((pr > 0).any()) and bool(torch.isfinite(pr).all())
    for e in (dense, sparse):
        e.check()
        e.close()
    f.check()
    f.close()


# ------------------------------------------------------------------------------------------------ 6. a stale plan
def test_a_plan_of_another_eps_or_of_the_step_before_is_refused(T):
    d, n, seed = 5, 300, 616
    f = T.NN11Forward(K.trained_state_dict(d), d, "cuda", max_rows=1 << 12)
    envs = make_envs(T, d, n, seed)
    eps = S.reference_eps(n)
    persp, pos, _ = envs.generatePerspectiveReused(dtype=torch.uint8)
    plan = envs.selectPlan(eps)
    q = f(persp, plan.rows)
    act, _ = envs.selectAction(q, eps, positions=pos, plan=plan)
    envs.check()                                                # the right eps: clean
    assert bool((act[:, 3] >= 1).all())
    act, qv = envs.selectAction(q, eps[::-1].copy(), positions=pos, plan=plan)
    with pytest.raises(ValueError, match="plan"):
        envs.check()
    refused = act[:, 3] == 0
    assert 0 < int(refused.sum()) < n and not bool(qv[refused].any())
    with pytest.raises(ValueError, match="plan.R"):
        envs.selectAction(q[:-1], eps, positions=pos, plan=plan)
    # a step between the plan and the selection: the lattices' counters moved on
    plan = envs.selectPlan(eps)
    q = f(persp, plan.rows)
    envs.actorStep(None)
    act, qv = envs.selectAction(q, eps, positions=pos, plan=plan)
    with pytest.raises(ValueError, match="plan"):
        envs.check()
    assert 0 < int((act[:, 3] == 0).sum())
    envs.check()
    envs.close()
    f.close()


# ------------------------------------------------------------------------------------------------ 7. a torch model
def test_a_torch_model_selects_the_same_sparse_and_dense(T):
    """NN_11 in torch under K.integer_state_dict: every sum is exact, so whatever kernel the row count selects gives the
    same bits, and the index_select path of _forward_chunked must reproduce the dense selection."""
    d, n, seed = 5, 100, 717
    model = K.model_of(K.integer_state_dict(d), d).cuda()
    dense, sparse = make_envs(T, d, n, seed), make_envs(T, d, n, seed)
    eps = S.reference_eps(n)
    for t in range(3):
        act_d, qv_d = T.selectActionEnvSet(dense, model, eps)
        act_s, qv_s = T.selectActionEnvSet(sparse, model, eps, sparse=True)
        assert torch.equal(act_d, act_s) and torch.equal(qv_d.view(torch.int32), qv_s.view(torch.int32)), t
        assert sparse.selectPlan(eps).R < int(sparse.perspectiveCounts()[1][-1])
        dense.actorStep(act_d)
        sparse.actorStep(act_s)
    for e in (dense, sparse):
        e.check()
        e.close()
