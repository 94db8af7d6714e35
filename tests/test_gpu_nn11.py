"""The hand-written NN_11 forward (tq_nn11_*, policy.NN11Forward) on the GPU against torch: bit for bit where the
arithmetic is exact, within the contract's own rounding error on trained weights, and end to end through the selection
and the evaluation loop."""
import ctypes as C
import os

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")             # no exhaustive solver search per batch shape on a fresh box

import numpy as np
import pytest
import torch

import nn11_cases as K

pytestmark = pytest.mark.gpu
DTYPES = (torch.uint8, torch.float32, torch.float16, torch.bfloat16)
MAX_ROWS = 64


@pytest.fixture(scope="module")
def T():
    import toric_rl_decoder_amd as T
    assert torch.cuda.is_available()
    T.load()
    return T


group = K.group                                # perspectives per workgroup: NN11Geom<D>::G of csrc/nn11.hpp


def row_counts(d):
    g = group(d)
    return sorted({1, 2 * g - 1, 2 * g, 2 * g + 1, 2 * MAX_ROWS + 3})      # the tile edge and the pass edge


_exact = {}


def exact_case(d):
    """(state_dict, first perspectives uint8, torch's f32 CPU Q-table of them), computed once per size."""
    if d not in _exact:
        sd = K.integer_state_dict(d)
        per, _ = K.stack_of(d, 64)
        per = per[:2 * MAX_ROWS + 3]
        assert per.shape[0] == 2 * MAX_ROWS + 3
        with torch.no_grad():
            q = K.model_of(sd, d)(torch.from_numpy(per).float())
        _exact[d] = (sd, per, q.numpy())
    return _exact[d]


@pytest.mark.parametrize("d", K.SIZES)
def test_exact_integer_network_is_bit_equal_to_torch_f32(T, d):
    sd, per, want = exact_case(d)
    f = T.NN11Forward(sd, d, "cuda", max_rows=MAX_ROWS)
    dtypes = DTYPES if d == 7 else (DTYPES[K.SIZES.index(d) % 4],)
    for dt in dtypes:
        x = torch.from_numpy(per).cuda().to(dt)
        for rows in row_counts(d):
            got = f(x[:rows])
            assert got.dtype == torch.float32 and tuple(got.shape) == (rows, 3)
            got = got.cpu().numpy()
            assert np.array_equal(got, want[:rows]), (d, dt, rows, int((got != want[:rows]).any(axis=1).sum()))
    empty = f(x[:0])
    assert tuple(empty.shape) == (0, 3) and empty.dtype == torch.float32
    f.close()


def dense_row_counts(d):
    g = group(d)
    return sorted({1, g, g + 1, 2 * g + 1, 2 * g + 3})      # with a handle of G + 1 rows: the tile, workgroup and pass edges


@pytest.fixture(scope="module")
def dense_handles(T):
    """one handle of G + 1 rows per size, reloaded for every network"""
    handles = {}
    yield handles
    for f in handles.values():
        f.close()


def dense_handle(T, handles, sd, d):
    if d in handles:
        return handles[d].load(sd)
    handles[d] = T.NN11Forward(sd, d, "cuda", max_rows=group(d) + 1)
    return handles[d]


@pytest.mark.parametrize("d,dense_layer", [(d, l) for d in K.SIZES for l in K.DENSE_LAYERS])
def test_dense_exact_network_is_bit_equal_to_the_f64_reference(T, dense_handles, d, dense_layer):
    """K.exact_dense_case: one layer dense, bf16 roundings with ties in weights and activations, every f32 sum exact
    (asserted by the reference), so one right answer in bits -- which tests/test_nn11_host.py shows a wrong rounding
    mode, padding, tap order or k range to miss.  The row counts run down and up again on a handle of G + 1 rows, so
    that a larger pass leaves its activations in the scratch of a smaller one; the handle was loaded with the previous
    network before, so a reload has to replace every weight and bias."""
    rows = K.dense_rows_for(d)
    sd, per, want, _ = K.exact_dense_case(d, dense_layer, rows)
    f = dense_handle(T, dense_handles, sd, d)
    counts = dense_row_counts(d)
    assert counts[-1] == rows == per.shape[0]
    dtypes = DTYPES if d == 7 else (DTYPES[(K.SIZES.index(d) + dense_layer) % 4],)
    for dt in dtypes:
        x = torch.from_numpy(per).cuda().to(dt)
        for n in counts[::-1] + counts:
            got = f(x[:n]).cpu().numpy()
            assert np.array_equal(got, want[:n]), (d, dense_layer, dt, n, int((got != want[:n]).any(axis=1).sum()))


@pytest.mark.parametrize("d,dense_layer", K.WIDE_CASES)
def test_stack_elements_are_converted_as_the_contract_says(T, d, dense_layer):
    """Stacks with elements beside 0 / 1 on the dense case's network fitted to them: {2, 255} for all four element types
    (bf16 holds them), and {2, 3, 257, 259, 261, 263} as f32 and f16, which round (all four ties), and as bf16 after
    torch's rounding.  Expected: the f64 reference on the RNE-rounded stack, under the exactness condition."""
    rows = K.dense_rows_for(d)
    sd, x8, want, _ = K.exact_dense_case(d, dense_layer, rows, K.U8_VALUES)
    f = T.NN11Forward(sd, d, "cuda", max_rows=group(d) + 1)
    x = torch.from_numpy(x8).cuda()
    for dt in DTYPES:
        assert torch.equal(x.to(dt).float(), x.float())
        assert np.array_equal(f(x.to(dt)).cpu().numpy(), want), (d, dense_layer, dt)
    sd, xw, want, _ = K.exact_dense_case(d, dense_layer, rows, K.WIDE_VALUES)
    f.load(sd)
    x = torch.from_numpy(xw).cuda()
    assert torch.equal(x.half().float(), x) and not torch.equal(x.bfloat16().float(), x)
    q32, q16, qbf = f(x), f(x.half()), f(x.bfloat16())
    assert torch.equal(q32, qbf)
    for dt, q in ((torch.float32, q32), (torch.float16, q16), (torch.bfloat16, qbf)):
        got = q.cpu().numpy()
        assert np.array_equal(got, want), (d, dense_layer, dt, int((got != want).any(axis=1).sum()), rows)
    f.close()


@pytest.mark.parametrize("d", (5, 7))
def test_a_rows_q_values_depend_on_nothing_but_the_row(T, d):
    """Trained weights.  Each output's operations are ordered by (tap, k-step, lane half) alone and rows never meet before
    the store, so a perspective's Q-values are the same bits wherever it stands in the batch, whatever stands beside it
    and however the call is cut into passes."""
    g, n = group(d), 300
    sd = K.trained_state_dict(d)
    x = torch.from_numpy(K.stack_of(d, 256)[0][:n]).cuda()
    assert x.shape[0] == n
    f = T.NN11Forward(sd, d, "cuda", max_rows=4096)
    q = f(x)
    assert bool(torch.isfinite(q).all()) and torch.unique(q, dim=0).shape[0] > n // 2      # rows differ: a mix-up shows
    rng = np.random.default_rng(300 + d)
    perm = torch.from_numpy(rng.permutation(n)).cuda()
    assert torch.equal(f(x[perm]), q[perm])
    for k in rng.choice(n, 12, replace=False):
        assert torch.equal(f(x[k:k + 1].clone()), q[k:k + 1]), k
    fill = torch.cat([torch.ones_like(x[:1]), torch.zeros_like(x[:1])]).repeat(n // 2, 1, 1, 1)
    for first in (0, 1):                                        # x at the even rows, then at the odd ones
        y = torch.empty((2 * n,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        y[first::2], y[1 - first::2] = x, fill
        got = f(y)
        assert torch.equal(got[first::2], q), first
        for kind in (0, 1):                                     # the all-ones rows agree among themselves; so do the zeros
            same = got[1 - first::2][kind::2]
            assert torch.equal(same, same[:1].expand_as(same)), (first, kind)
    f.close()
    for max_rows in (g - 1, g, g + 1):
        if max_rows >= 1:
            h = T.NN11Forward(sd, d, "cuda", max_rows=max_rows)
            assert torch.equal(h(x), q), max_rows
            h.close()


def test_a_misaligned_stack_is_refused_before_any_launch(T):
    d = 3
    f = T.NN11Forward(K.integer_state_dict(d), d, "cuda", max_rows=64)
    x = torch.from_numpy(K.dense_rows(d, 9)).cuda()
    y = x[1:]                                                   # contiguous, 18 bytes past an aligned address
    assert y.is_contiguous() and x.data_ptr() % 16 == 0 and y.data_ptr() % 16 != 0
    L = T.load()
    q = torch.full((8, 3), 7.0, device="cuda")
    torch.cuda.synchronize()
    assert L.tq_nn11_forward(f._h, C.c_void_p(y.data_ptr()), 3, 8, C.c_void_p(q.data_ptr()), None) == -1     # TQ_E_INVALID
    assert b"stack must be 16-byte aligned" in L.tq_last_error()
    with pytest.raises(ValueError, match="16-byte aligned"):
        f(y)
    torch.cuda.synchronize()
    assert bool((q == 7.0).all())
    assert tuple(f(x[1:].clone()).shape) == (8, 3)             # the same rows at an aligned address are taken
    f.close()


@pytest.mark.parametrize("d", (5, 7))
def test_trained_weights_are_no_worse_than_the_contract_and_better_than_autocast(T, d):
    """All three reference quantities by torch on the GPU: the f32 forward, the contract restated in torch ops
    (K.contract_forward) and today's bf16 path (autocast on the bf16 stack)."""
    model = K.model_of(K.trained_state_dict(d), d).cuda()
    per, off = K.stack_of(d, 256)
    x = torch.from_numpy(per).cuda()
    with torch.no_grad():
        q32 = model(x.float())
        with torch.autocast("cuda", dtype=torch.bfloat16):
            qac = model(x.bfloat16()).float()
    yard = K.contract_forward(model, x)
    f = T.NN11Forward(model, d, "cuda", max_rows=4096)
    got = f(x)
    e_yard, e_got, e_ac = K.rms(yard, q32), K.rms(got, q32), K.rms(qac, q32)
    m_got, m_ac = float((got - q32).abs().max()), float((qac - q32).abs().max())
    g32 = K.greedy_per_lattice(q32, off)
    flips_got = int((K.greedy_per_lattice(got, off) != g32).sum())
    flips_ac = int((K.greedy_per_lattice(qac, off) != g32).sum())
    print(f"nn11 accuracy d={d}: {x.shape[0]} perspectives of 256 lattices, Q in [{float(q32.min()):.1f}, {float(q32.max()):.1f}]; "
          f"rms error vs torch f32: contract yardstick {e_yard:.4f}, NN11Forward {e_got:.4f}, torch bf16 autocast {e_ac:.4f}; "
          f"max error: NN11Forward {m_got:.4f}, autocast {m_ac:.4f}; "
          f"greedy action differs from f32's on {flips_got} (NN11Forward) / {flips_ac} (autocast) of 256 lattices")
    assert e_yard > 0
    assert e_got <= 2 * e_yard
    assert e_got <= e_ac and m_got <= m_ac
    assert flips_got <= flips_ac
    for dt in DTYPES[1:]:                                       # the stack's element type does not change a bit
        assert torch.equal(f(x.to(dt)), got)
    f.close()


def test_load_refresh_repeat_and_forward_before_load(T):
    d = 5
    a, b = K.integer_state_dict(d), K.trained_state_dict(d)
    per, _ = K.stack_of(d, 64)
    x = torch.from_numpy(per[:333]).cuda()
    f = T.NN11Forward(a, d, "cuda", max_rows=100)
    qa = f(x)
    assert torch.equal(f(x), qa)                                # the same call twice
    f.load(b)
    qb = f(x)
    fresh = T.NN11Forward(T.NN_11(d).eval(), d, "cuda", max_rows=100).load(b)
    assert torch.equal(qb, fresh(x)) and not torch.equal(qa, qb)
    assert f.eval() is f and f.train() is f
    with pytest.raises(ValueError):
        f.load({k: v for k, v in b.items() if k != "conv3.bias"})
    f.close()
    f.close()
    fresh.close()
    # a forward before any load: the error code, not a fault
    L = T.load()
    h = C.c_void_p(None)
    assert L.tq_nn11_create(C.byref(h), d, 64, 0) == 0
    q = torch.zeros((8, 3), device="cuda")
    assert L.tq_nn11_forward(h, C.c_void_p(x.data_ptr()), 3, 8, C.c_void_p(q.data_ptr()), None) == -1
    assert b"before" in L.tq_last_error()
    torch.cuda.synchronize()
    assert not bool(q.any())
    assert L.tq_nn11_destroy(h) == 0


def test_select_action_on_the_u8_stack_end_to_end(T):
    d, n = 5, 512
    model = K.model_of(K.trained_state_dict(d), d).cuda()
    f = T.NN11Forward(model, d, "cuda", max_rows=1 << 12)
    envs = T.EnvSet(T.make("toric-code-v0", {"size": d, "p_error": 0.1}), n, seed=5, numpy_io=False)
    envs.resetAll()
    act, qv = T.selectActionEnvSet(envs, f, 0.0, dtype=torch.uint8)
    envs.check()
    _, pos, cnt = envs.generatePerspective()
    pos, cnt, act = pos.cpu().numpy(), cnt.cpu().numpy(), act.cpu().numpy()
    off = np.concatenate([[0], np.cumsum(cnt)])
    assert (cnt > 0).all()
    for e in range(n):
        assert 1 <= act[e, 3] <= 3
        assert (pos[off[e]:off[e + 1]] == act[e, :3]).all(axis=1).any(), e
    assert qv.dtype == torch.float32 and tuple(qv.shape) == (n, 3) and bool(torch.isfinite(qv).all())
    envs.close()
    f.close()


def test_evaluate_with_the_wrapper_matches_the_torch_model(T):
    d, episodes = 5, 1024
    model = K.model_of(K.trained_state_dict(d), d).cuda()
    f = T.NN11Forward(model, d, "cuda", max_rows=1 << 14)
    args = ("toric-code-v0", {"size": d, "min_qubit_errors": 0}, d // 2, "cuda", [0.1])
    kw = dict(num_of_episodes=episodes, epsilon=0.0, num_of_steps=75, seed=20261, chunk=1 << 14)
    _, ground_t, _, _, _ = T.evaluate(model, *args, **kw)
    _, ground_w, _, _, _ = T.evaluate(f, *args, **kw)
    r = float(ground_t[0])
    sigma = np.sqrt(2 * r * (1 - r) / episodes)
    print(f"evaluate d={d} p=0.1, {episodes} episodes: ground-state rate torch f32 {r:.4f}, NN11Forward {float(ground_w[0]):.4f}, sigma {sigma:.4f}")
    assert 0.5 < r < 1.0
    assert abs(float(ground_w[0]) - r) <= 4 * sigma
    f.close()
