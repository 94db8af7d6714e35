"""The hand-written eval-mode forward of the BasicBlock ResNets (tq_resnet_*, policy.ResNetForward) on the GPU: bit for
bit where the arithmetic is exact (integer nets against the float64 reference and, where the pool is exact, torch f32; the
dense exact cases of tests/resnet_cases.py against their float64 reference), within the contract's own rounding error on
weights that are not integers, and through the package's callers of a model."""
import ctypes as C
import os

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")             # no exhaustive solver search per batch shape on a fresh box

import numpy as np
import pytest
import torch

import resnet_cases as K

pytestmark = pytest.mark.gpu
DTYPES = (torch.uint8, torch.float32, torch.float16, torch.bfloat16)


@pytest.fixture(scope="module")
def T():
    import toric_rl_decoder_amd as T
    assert torch.cuda.is_available()
    T.load()
    return T


@pytest.mark.parametrize("net,d", K.INTEGER_CASES)
def test_integer_network_is_bit_equal_to_the_f64_reference_and_to_torch_f32(T, net, d):
    """2 G + 3 rows on a handle of G + 1 rows: the tile edge, the workgroup edge and the pass edge are crossed.  ResNet18
    at every supported size, ResNet34 at d = 5 and d = 9.  torch's own f32 forward (on the host) is held to the same bits
    at d = 3, 7, 15, where s^2 is a power of two and its mean over the pixels is exact."""
    g = K.group(d)
    rows = 2 * g + 3
    sd = K.integer_state_dict(net, d)
    per = K.dense_rows(d, rows)
    ref, stats = K.dense_reference(sd, torch.from_numpy(per))
    assert stats["max_act"] <= 256
    want = ref.float().numpy()
    assert len({r.tobytes() for r in want}) > 1
    if d in K.TORCH_EXACT_SIZES:
        with torch.no_grad():
            assert np.array_equal(K.model_of(sd)(torch.from_numpy(per).float()).numpy(), want)
    f = T.ResNetForward(sd, d, "cuda", max_rows=g + 1)
    assert f.net == net
    x = torch.from_numpy(per).cuda().to(DTYPES[(K.SIZES.index(d) + net) % 4])
    for n in (rows, g, 1):
        got = f(x[:n])
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, 3)
        got = got.cpu().numpy()
        assert np.array_equal(got, want[:n]), (net, d, n, int((got != want[:n]).any(axis=1).sum()))
    f.close()


@pytest.mark.parametrize("net,d,dense", K.CASES)
def test_dense_exact_case_is_bit_equal_to_the_f64_reference(T, net, d, dense):
    """K.exact_dense_case: one convolution dense, bf16 roundings with ties in weights and activations, every f32 sum exact
    (asserted by the reference), so one right answer in bits whatever the order of (chunk, tap, k-step) -- which
    tests/test_resnet_host.py shows a wrong rounding, padding, tap, residual, shift, stride or pool to miss.  The row
    counts run down and up again on a handle of G + 1 rows, so that a larger pass leaves its activations in the scratch
    of a smaller."""
    g = K.group(d)
    rows = K.dense_rows_for(d)
    sd, per, want, _ = K.exact_dense_case(net, d, dense, rows)
    f = T.ResNetForward(sd, d, "cuda", max_rows=g + 1)
    x = torch.from_numpy(per).cuda()
    counts = sorted({1, g, g + 1, 2 * g + 1, rows})
    for n in counts[::-1] + counts:
        got = f(x[:n]).cpu().numpy()
        assert np.array_equal(got, want[:n]), (net, d, dense, n, int((got != want[:n]).any(axis=1).sum()))
    f.close()


def test_the_heads_order_of_sums_is_the_contracts(T):
    """An integer net under a linear layer of normal weights: everything up to the channel sums is exact, the head's sums
    round, and the one right answer in bits is the contract's order (a lane's eight channels in order, then the butterfly
    over the 64 lanes), restated in numpy f32 by K.head_in_kernel_order."""
    sd, per, want, plain = K.head_order_case()
    assert (plain != want).any()                                # another order gives other bits: the case can tell
    f = T.ResNetForward(sd, 7, "cuda", max_rows=64)
    got = f(torch.from_numpy(per).cuda()).cpu().numpy()
    assert np.array_equal(got, want), int((got != want).any(axis=1).sum())
    f.close()


def test_all_four_stack_dtypes_give_the_same_bits(T):
    net, d, dense = K.CASES[1]
    sd, per, want, _ = K.exact_dense_case(net, d, dense, K.dense_rows_for(d))
    f = T.ResNetForward(sd, d, "cuda", max_rows=64)
    x = torch.from_numpy(per).cuda()
    for dt in DTYPES:
        assert np.array_equal(f(x.to(dt)).cpu().numpy(), want), dt
    # elements beside 0 / 1: 2 and 255 are held by all four types, so the Q-table is one
    y = x.clone()
    y[::2, 0, 1, 1], y[1::2, 1, 2, 3] = 255, 2
    q = f(y)
    assert not torch.equal(q, f(x))
    for dt in DTYPES[1:]:
        assert torch.equal(y.to(dt).float(), y.float()) and torch.equal(f(y.to(dt)), q), dt
    f.close()


@pytest.fixture(scope="module")
def he18(T):
    """ResNet18 at d = 7 with He-normal weights: (handle, stack of 300 perspectives on the device, its Q-table)"""
    d, n = 7, 300
    f = T.ResNetForward(K.he_state_dict(18), d, "cuda", max_rows=128)
    x = torch.from_numpy(K.dense_rows(d, n)).cuda()
    q = f(x)
    yield f, x, q
    f.close()


def test_a_rows_q_values_depend_on_nothing_but_the_row(T, he18):
    """The order of a sum is (chunk, tap, k-step) for every row and rows never meet before the store: the same bits
    wherever a perspective stands in the batch, whatever the row count and however the call is cut into passes."""
    f, x, q = he18
    n, d = x.shape[0], 7
    assert bool(torch.isfinite(q).all()) and torch.unique(q, dim=0).shape[0] > n // 2      # rows differ: a mix-up shows
    assert torch.equal(f(x), q)                                 # the same call twice
    rng = np.random.default_rng(318)
    perm = torch.from_numpy(rng.permutation(n)).cuda()
    assert torch.equal(f(x[perm]), q[perm])
    for k in rng.choice(n, 6, replace=False):
        assert torch.equal(f(x[k:k + 1].clone()), q[k:k + 1]), k
    assert torch.equal(f(x[3:n - 8].clone()), q[3:n - 8])       # another row count, shifted against the tiles
    g = K.group(d)
    for max_rows in (g - 1, g + 1):
        h = T.ResNetForward(K.he_state_dict(18), d, "cuda", max_rows=max_rows)
        assert torch.equal(h(x[:40]), q[:40]), max_rows
        h.close()


def test_a_module_gives_its_eps_and_load_refreshes_the_weights(T, he18):
    f, x, q = he18
    model = K.model_of(K.he_state_dict(18))
    g = T.ResNetForward(model, 7, "cuda", max_rows=128, eps=0.5)          # the module's own eps, 1e-5, wins
    assert g.eps == 1e-5 and torch.equal(g(x[:50]), q[:50])
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eps = 1e-2
    g.load(model)
    assert g.eps == 1e-2 and not torch.equal(g(x[:50]), q[:50])
    g.load(K.he_state_dict(18, seed=1))                          # a state_dict keeps the handle's eps
    h = T.ResNetForward(K.he_state_dict(18, seed=1), 7, "cuda", max_rows=64, eps=1e-2)
    assert torch.equal(g(x[:50]), h(x[:50])) and not torch.equal(h(x[:50]), q[:50])
    g.close()
    h.close()


def test_forward_chunked_with_a_row_list_equals_the_rows_of_the_full_table(T, he18):
    from toric_rl_decoder_amd.policy import _forward_chunked
    f, x, q = he18
    assert f.gathers is False and f.any_rows is True
    rng = np.random.default_rng(5)
    rows = torch.from_numpy(rng.integers(0, x.shape[0], 77).astype(np.int32)).cuda()       # unsorted, with repeats
    got = _forward_chunked(f, x, 32, rows=rows)
    assert got.dtype == torch.float32 and torch.equal(got, q[rows.long()])
    assert torch.equal(_forward_chunked(f, x, 128), q)


@pytest.fixture(scope="module")
def he18_d5(T):
    f = T.ResNetForward(K.he_state_dict(18), 5, "cuda", max_rows=512)
    yield f
    f.close()


def test_predict_max_with_the_handle_is_segment_max_over_its_own_table(T, he18_d5):
    from oracle import toric_oracle as O
    d, n, f = 5, 48, he18_d5
    _, st = O.reset_lattices(91, np.arange(n), 0, 0.1, d)
    st[::7] = 0                                                 # terminal states
    states = torch.from_numpy(st.astype(np.float32)).cuda()
    got = T.predictMaxOptimized(f, states, d // 2, d, "cuda:0", chunk=100)
    persp, _, counts, offsets = T.generatePerspectiveBatch(d // 2, d, states, device="cuda:0", return_offsets=True)
    largest = torch.clamp(counts.max(), min=1).to(torch.int32).reshape(1)
    want = T.segment_max(f(persp), offsets, largest)
    assert tuple(got.shape) == (n,) and torch.equal(got, want) and bool((got != 0).any())


def test_sparse_selection_reads_the_same_bits_as_the_dense_one(T, he18_d5):
    d, n, f = 5, 96, he18_d5
    out = []
    for sparse in (False, True):
        envs = T.EnvSet(T.make("toric-code-v0", {"size": d, "p_error": 0.1}), n, seed=5, numpy_io=False)
        envs.resetAll()
        out.append(T.selectActionEnvSet(envs, f, 0.3, dtype=torch.uint8, sparse=sparse))
        envs.check()
        envs.close()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_evaluate_takes_the_handle_and_decides_as_its_own_table_does(T, he18_d5):
    """One evaluate call at d = 5 with the handle as the model, against the same call with a model that answers from the
    handle's own Q-table: every figure evaluate returns is the same."""
    d, f = 5, he18_d5

    class Table(torch.nn.Module):                               # a torch module that answers from the handle's own table
        def forward(self, persp):
            return f(persp.contiguous())

    args = ("toric-code-v0", {"size": d, "min_qubit_errors": 0}, d // 2, "cuda", [0.1])
    kw = dict(num_of_episodes=64, epsilon=0.0, num_of_steps=12, seed=31, round_like_reference=False)
    got = T.evaluate(f, *args, **kw)
    want = T.evaluate(Table(), *args, **kw)
    assert len(got) == len(want) == 5 and 0.0 <= got[0][0] <= 1.0 and got[2][0] > 0
    for a, b in zip(got[:4], want[:4]):
        assert np.array_equal(a, b)
    assert len(got[4]) == len(want[4]) and all(np.array_equal(a, b) for a, b in zip(got[4], want[4]))


def test_argument_errors_are_codes_not_aborts_and_no_rows_is_a_no_op(T):
    d = 5
    sd = K.integer_state_dict(18, d)
    with pytest.raises(ValueError, match="neither"):
        T.ResNetForward({k: v for k, v in sd.items() if k != "layer3.0.bn2.bias"}, d, "cuda")       # wrong keys
    with pytest.raises(ValueError):
        T.ResNetForward(sd, 6, "cuda")
    with pytest.raises(ValueError):
        T.ResNetForward(sd, d, "cuda", eps=0.0)
    f = T.ResNetForward(sd, d, "cuda", max_rows=16)
    x = torch.from_numpy(K.dense_rows(d, 9)).cuda()
    with pytest.raises(ValueError):
        f.load(K.integer_state_dict(34, d))                     # the other net on this handle
    with pytest.raises(ValueError):
        f(x[:, :, :3])                                          # not (rows, 2, d, d)
    with pytest.raises(ValueError):
        f(x.to(torch.int32))
    empty = f(x[:0])
    assert tuple(empty.shape) == (0, 3) and empty.dtype == torch.float32
    L = T.load()
    q = torch.full((8, 3), 7.0, device="cuda")
    torch.cuda.synchronize()
    assert L.tq_resnet_forward(f._h, C.c_void_p(x.data_ptr()), 3, 0, None, None) == 0           # rows = 0: nothing is read
    assert L.tq_resnet_forward(f._h, C.c_void_p(x.data_ptr()), 7, 8, C.c_void_p(q.data_ptr()), None) == -1      # TQ_E_INVALID
    assert L.tq_resnet_forward(f._h, C.c_void_p(x.data_ptr()), 3, -1, C.c_void_p(q.data_ptr()), None) == -1
    assert L.tq_resnet_forward(f._h, C.c_void_p(x.data_ptr() + 18), 3, 8, C.c_void_p(q.data_ptr()), None) == -1
    assert b"16-byte aligned" in L.tq_last_error()
    assert L.tq_resnet_load(f._h, None, None, None, None, 1e-5, None) == -1
    f.close()
    f.close()
    # a forward before any load: the error code, not a fault
    h = C.c_void_p(None)
    assert L.tq_resnet_create(C.byref(h), 34, d, 64, 0) == 0
    assert L.tq_resnet_forward(h, C.c_void_p(x.data_ptr()), 3, 8, C.c_void_p(q.data_ptr()), None) == -1
    assert b"before" in L.tq_last_error()
    torch.cuda.synchronize()
    assert bool((q == 7.0).all())
    assert L.tq_resnet_destroy(h) == 0


def test_he_normal_weights_stay_within_the_contracts_own_rounding_error(T):
    """No trained ResNet checkpoint exists: seeded He-normal conv weights and sane random BatchNorm statistics
    (K.he_state_dict) on the perspectives of 256 lattices at d = 7, p = 0.1.  All reference quantities by torch on the GPU:
    the f32 eval forward and the contract restated in torch ops (K.contract_forward), from which the kernels differ in f32
    summation order alone.  Gate: the kernels' rms error against f32 <= 1.1 x the contract's own (the learner-step gate's
    margin).  Measured on an MI355X (profiles/resnet_forward_accuracy.txt): see that file."""
    net, d = 18, 7
    model = K.model_of(K.he_state_dict(net)).cuda()
    per, off = K.stack_of(d, 256)
    x = torch.from_numpy(per).cuda()
    with torch.no_grad():
        q32 = model(x.float())
    yard = K.contract_forward(model, x)
    f = T.ResNetForward(model, d, "cuda", max_rows=4096)
    got = f(x)
    e_yard, e_got = K.rms(yard, q32), K.rms(got, q32)
    m_yard, m_got = float((yard - q32).abs().max()), float((got - q32).abs().max())
    g32 = K.greedy_per_lattice(q32, off)
    flips_yard = int((K.greedy_per_lattice(yard, off) != g32).sum())
    flips_got = int((K.greedy_per_lattice(got, off) != g32).sum())
    print(f"resnet accuracy ResNet{net} d={d}: {x.shape[0]} perspectives of 256 lattices, Q in [{float(q32.min()):.3f}, "
          f"{float(q32.max()):.3f}], rms of Q {float(q32.double().pow(2).mean().sqrt()):.4f}; rms error vs torch f32: contract "
          f"yardstick {e_yard:.6f}, ResNetForward {e_got:.6f} (ratio {e_got / e_yard:.4f}); max error: yardstick {m_yard:.6f}, "
          f"ResNetForward {m_got:.6f}; greedy action differs from f32's on {flips_yard} (yardstick) / {flips_got} (ResNetForward) "
          f"of 256 lattices")
    assert e_yard > 0 and bool(torch.isfinite(got).all())
    assert e_got <= 1.1 * e_yard
    f.close()
