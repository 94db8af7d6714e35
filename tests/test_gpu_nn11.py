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


def group(d):
    return max(1, 256 // (d * d))              # perspectives per workgroup: NN11Geom<D>::G of csrc/nn11.hpp


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
