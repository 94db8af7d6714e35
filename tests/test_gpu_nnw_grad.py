"""The wide nets' learner step (tq_nnw_grad_*, policy.NNWideGrad, policy.learnerStep) on the GPU: bit for bit on the two
cases of tests/nnw_grad_cases.py for NN_8 at every size and NN_17 at three, every stack element type, the handle's
scratch, its argument checks, the forward and the head, dense weights against torch's f32 autograd, and three learner
steps on a replay memory.  G: a conv workgroup's perspectives (nnw_cases.group(d)); p: a wgrad chunk's records
(nnw_wgrad_persp(d))."""
import ctypes as C

import numpy as np
import pytest
import torch

import nnw_cases as K
import nnw_grad_cases as GC

pytestmark = pytest.mark.gpu
DTYPES = (torch.uint8, torch.float32, torch.float16, torch.bfloat16)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def T():
    import toric_rl_decoder_amd as T
    assert torch.cuda.is_available()
    T.load()
    return T


def grads_of(model):
    return {k: p.grad.cpu().numpy() for k, p in model.named_parameters()}


def poison(model):
    for p in model.parameters():
        if p.grad is not None:
            p.grad.fill_(float("nan"))                          # gradients are written, not accumulated


def step(grad, model, c, x, n, w):
    poison(model)
    loss, q = grad.backward(x[:n], c["actions"][:n].to(DEV), c["y"][:n].to(DEV), w.to(DEV))
    return loss, q, grads_of(model)


def handle_of(T, c, max_batch=None):
    """(model holding the case's network, NNWideGrad over it); the handle held the negated network before"""
    net, d = c["net"], c["d"]
    model = K.MODULES[net](d).to(DEV)
    model.load_state_dict({k: -v for k, v in c["sd"].items()})
    grad = T.NNWideGrad(model, d, DEV, max_batch=max_batch or c["x"].shape[0])
    model.load_state_dict(c["sd"])
    grad.load()
    return model, grad


def assert_step(c, n, loss, q, got, what):
    w, want_loss, want = GC.at_rows(c, n)
    assert q.dtype == loss.dtype == torch.float32 and tuple(q.shape) == (n, 3) and tuple(loss.shape) == (n,)
    assert np.array_equal(q.cpu().numpy(), c["q"][:n]), what
    assert np.array_equal(loss.cpu().numpy(), want_loss), what
    assert len(got) == 2 * (GC.layers(c["net"]) + 1)
    for k in GC.params(c["net"]):
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()), want[k].size)


def run_case(T, c, dtype=torch.uint8):
    net, d = c["net"], c["d"]
    model, grad = handle_of(T, c)
    assert grad.net == net and grad.max_batch == GC.row_counts(d)[-1]
    x = torch.from_numpy(c["x"]).to(DEV).to(dtype)
    return model, grad, x


@pytest.mark.parametrize("d", K.SIZES)
def test_nn8_integer_case_is_bit_equal_to_torch_autograd(T, d):
    """GC.integer_case (torch's own f32 autograd is the reference): all 18 gradient tensors, q and loss, for n = 1,
    G + 1 and p + 1 records."""
    c = GC.integer_case(8, d)
    model, grad, x = run_case(T, c, DTYPES[K.SIZES.index(d) % 4])
    assert GC.row_counts(d) == sorted({1, K.group(d) + 1, GC.wgrad_persp(d) + 1})
    for n in GC.row_counts(d):
        loss, q, got = step(grad, model, c, x, n, GC.at_rows(c, n)[0])
        assert len(got) == 18
        assert_step(c, n, loss, q, got, (8, d, n))
    grad.check()
    grad.close()


@pytest.mark.parametrize("d", (3, 5, 9))
def test_nn17_integer_case_is_bit_equal_to_torch_autograd(T, d):
    """All 42 tensors at n = p + 1: d = 3's single output pixel, a chunk boundary and a two-chunk sum."""
    c = GC.integer_case(17, d)
    model, grad, x = run_case(T, c)
    n = GC.wgrad_persp(d) + 1
    loss, q, got = step(grad, model, c, x, n, GC.at_rows(c, n)[0])
    assert len(got) == 42
    assert_step(c, n, loss, q, got, (17, d, n))
    grad.check()
    grad.close()


@pytest.mark.parametrize("net,d", ((8, 3), (8, 5), (8, 7), (17, 5)))
def test_rounding_case_is_bit_equal_to_the_float64_reference(T, net, d):
    """GC.rounding_case: float64 autograd with G rounded to bf16, ties included, every sum exact, at least two layers' G
    changed by RNE (asserted by the case)."""
    c = GC.rounding_case(net, d)
    model, grad, x = run_case(T, c)
    for n in GC.row_counts(d):
        loss, q, got = step(grad, model, c, x, n, GC.at_rows(c, n)[0])
        assert_step(c, n, loss, q, got, (net, d, n))
    grad.check()
    grad.close()


def test_the_four_stack_element_types_give_the_same_bits(T):
    d = 5
    c = GC.rounding_case(8, d)
    n = GC.wgrad_persp(d) + 1
    model, grad, _ = run_case(T, c)
    for dt in DTYPES:
        x = torch.from_numpy(c["x"]).to(DEV).to(dt)
        loss, q, got = step(grad, model, c, x, n, GC.at_rows(c, n)[0])
        assert_step(c, n, loss, q, got, (dt, n))
    grad.close()


def test_a_step_after_a_larger_one_gives_the_bits_of_a_fresh_handle(T):
    """One handle, n descending then ascending (p + 1, 1, G + 1): a larger step leaves its activations, gradients and
    partial images in the scratch of a smaller one."""
    d = 5
    c = GC.rounding_case(8, d)
    p, g = GC.wgrad_persp(d), K.group(d)
    model, used, x = run_case(T, c)
    for n in (p + 1, 1, g + 1):
        w = GC.at_rows(c, n)[0]
        loss_u, q_u, got_u = step(used, model, c, x, n, w)
        fresh = T.NNWideGrad(model, d, DEV, max_batch=p + 1)
        loss_f, q_f, got_f = step(fresh, model, c, x, n, w)
        fresh.close()
        assert torch.equal(loss_u, loss_f) and torch.equal(q_u, q_f), n
        for k in GC.params(8):
            assert np.array_equal(got_u[k], got_f[k]), (n, k)
        assert_step(c, n, loss_u, q_u, got_u, ("used", n))
    used.close()


@pytest.mark.parametrize("net", K.NETS)
def test_q_is_the_forward_handles_and_loss_is_the_head_contracts(T, net):
    """Dense weights (he_state_dict) and arbitrary f32 targets and weights: q is bit-equal to NNWideForward on the same
    state_dict, loss to GC.head_contract in f32 torch ops; with weights and without."""
    d, n = 5, K.group(5) + 3
    sd = K.he_state_dict(net, d)
    model = K.MODULES[net](d).to(DEV)
    model.load_state_dict(sd)
    grad = T.NNWideGrad(model, d, DEV, max_batch=n)
    fwd = T.NNWideForward(sd, d, DEV, max_rows=n)
    rng = np.random.default_rng(net)
    x = torch.from_numpy(K.dense_rows(d, n)).to(DEV)
    a = torch.from_numpy(rng.integers(0, 3, n)).to(DEV)
    y = torch.from_numpy((rng.normal(size=n) * 3).astype(np.float32)).to(DEV)
    for w in (torch.from_numpy(rng.uniform(0.01, 3, n).astype(np.float32)).to(DEV), None):
        loss, q = grad.backward(x, a, y, w)
        assert torch.equal(q, fwd(x)) and bool(q.abs().sum() > 0)
        want, _ = GC.head_contract(q.cpu(), a.cpu(), y.cpu(), None if w is None else w.cpu())
        assert torch.equal(loss.cpu(), want)
    grad.check()
    grad.close()
    fwd.close()


def test_an_action_outside_the_range_gives_no_loss_and_no_gradient_and_is_latched(T):
    """The record with a bad action has loss 0 and contributes nothing: the gradients are those of the same step with
    that record's weight 0 (dq = 0 either way; the other records' head divides by the same n)."""
    d, n = 3, 8
    c = GC.integer_case(8, d)
    model, grad = handle_of(T, c, max_batch=n)
    x = torch.from_numpy(c["x"][:n]).to(DEV)
    a, y = c["actions"][:n].to(DEV), c["y"][:n].to(DEV)
    w = torch.full((n,), n / 2, device=DEV)
    for bad_value in (3, -1):
        bad = a.clone()
        bad[2] = bad_value
        poison(model)
        loss_b, q_b = grad.backward(x, bad, y, w)
        got_b = grads_of(model)
        with pytest.raises(ValueError, match="actions_idx"):
            grad.check()
        grad.check()                                            # the latch was cleared
        w0 = w.clone()
        w0[2] = 0
        poison(model)
        loss_0, q_0 = grad.backward(x, a, y, w0)
        got_0 = grads_of(model)
        assert float(loss_b[2]) == 0.0 and torch.equal(loss_b, loss_0) and torch.equal(q_b, q_0)
        keep = [i for i in range(n) if i != 2]
        assert np.array_equal(loss_b.cpu().numpy()[keep], GC.at_rows(c, n)[1][keep])
        for k in GC.params(8):
            assert np.array_equal(got_b[k], got_0[k]), k
    grad.check()
    grad.close()


def test_arguments_are_checked_before_any_launch(T):
    d, n = 3, 8
    c = GC.integer_case(8, d)
    L = T.load()
    model = T.NN_8(d).to(DEV)
    model.load_state_dict(c["sd"])
    x = torch.from_numpy(c["x"][:n + 1]).to(DEV)
    a, y = c["actions"][:n].to(DEV), c["y"][:n].to(DEV)
    loss = torch.full((n,), 7.0, device=DEV)
    gw = [torch.full_like(p, 7.0) for k, p in model.named_parameters() if k.endswith("weight")]
    gb = [torch.full_like(p, 7.0) for k, p in model.named_parameters() if k.endswith("bias")]
    pw, pb = (C.c_void_p * 9)(*[t.data_ptr() for t in gw]), (C.c_void_p * 9)(*[t.data_ptr() for t in gb])
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(h, state=x, n_=n, a_=a, y_=y, loss_=loss, pw_=pw, pb_=pb):
        return L.tq_nnw_grad_step(h, p(state) if state is not None else None, 3, n_, p(a_) if a_ is not None else None,
                                  p(y_) if y_ is not None else None, None, None, p(loss_) if loss_ is not None else None, pw_, pb_, None)

    raw = C.c_void_p(None)
    for net, batch in ((11, n), (0, n), (8, 0), (8, 4097), (17, 4097)):
        assert L.tq_nnw_grad_create(C.byref(raw), net, d, batch, 0) == -1 and not raw.value, (net, batch)
    with pytest.raises(ValueError, match="neither"):
        T.NNWideGrad(T.NN_11(d).to(DEV), d, DEV)                # a wrong net
    with pytest.raises(ValueError, match="max_batch"):
        T.NNWideGrad(model, d, DEV, max_batch=0)
    with pytest.raises(ValueError, match="max_batch"):
        T.NNWideGrad(model, d, DEV, max_batch=4097)
    assert L.tq_nnw_grad_create(C.byref(raw), 8, d, n, 0) == 0
    assert call(raw) == -1 and b"before" in L.tq_last_error()                  # a step before any load
    assert L.tq_nnw_grad_destroy(raw) == 0
    g = T.NNWideGrad(model, d, DEV, max_batch=n)
    torch.cuda.synchronize()
    assert call(g._h, n_=n + 1) == -1 and call(g._h, n_=0) == -1 and call(g._h, n_=-3) == -1
    with pytest.raises(ValueError, match="max_batch"):
        g.backward(x, torch.zeros(n + 1, dtype=torch.int64), torch.zeros(n + 1))       # n > max_batch
    for kw in (dict(state=None), dict(a_=None), dict(y_=None), dict(loss_=None), dict(pw_=None), dict(pb_=None)):
        assert call(g._h, **kw) == -1, kw
    hole = (C.c_void_p * 9)(*[t.data_ptr() for t in gw[:5]] + [None] + [t.data_ptr() for t in gw[6:]])
    assert call(g._h, pw_=hole) == -1
    odd = x[1:]                                                 # contiguous, 18 bytes past an aligned address
    assert odd.is_contiguous() and odd.data_ptr() % 16 != 0
    assert call(g._h, state=odd) == -1 and b"16-byte aligned" in L.tq_last_error()
    with pytest.raises(ValueError, match="net"):
        g.load(T.NN_17(d).to(DEV))                              # a model of the other net
    torch.cuda.synchronize()
    assert bool((loss == 7.0).all()) and all(bool((t == 7.0).all()) for t in gw + gb)
    assert call(g._h) == 0                                      # the same call with nothing wrong is taken
    torch.cuda.synchronize()
    assert not bool((loss == 7.0).any()) and not any(bool((t == 7.0).all()) for t in gw + gb)
    g.check()
    g.close()
    g.close()


def test_three_learner_steps_with_adam_reload_the_masters_and_write_the_priorities(T):
    d, B, beta, alpha, lr = 5, 64, 0.4, 0.6, 1e-4
    mem = GC.play_memory(T, d, 78)
    sd = K.he_state_dict(8, d)
    target = T.NNWideForward(sd, d, DEV, max_rows=4096)
    model = T.NN_8(d).to(DEV)
    model.load_state_dict(sd)
    grad = T.NNWideGrad(model, d, DEV, max_batch=B)
    fwd = T.NNWideForward(sd, d, DEV, max_rows=B)
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    fixed = mem.sample_batch(B, beta, next_state=False)
    f_state, f_actions, f_reward, _, f_terminal, f_weights, f_indices = fixed
    f_y = T.learnerTargets(target, mem, f_indices, f_reward, f_terminal)
    seen = []
    for s in range(3):
        before = mem.leaves().cpu().numpy()
        masters = {k: v.detach().clone() for k, v in model.state_dict().items()}
        loss, idx = T.learnerStep(grad, target, mem, opt, B, beta)
        assert bool(torch.isfinite(loss).all()) and tuple(loss.shape) == (B,)
        assert any(not torch.equal(masters[k], v) for k, v in model.state_dict().items())       # Adam stepped the masters
        want = before.copy()                                    # the tree holds |loss| of this step (last occurrence wins)
        for i, v in zip(idx.cpu().numpy(), loss.abs().cpu().numpy()):
            want[i] = np.float64(v) ** alpha
        got = mem.leaves().cpu().numpy()
        assert np.all(np.abs(got - want) <= np.spacing(np.abs(want)))
        fwd.load(model.state_dict())                            # the handle's network is the updated masters': load() happened
        q_want = fwd(f_state)
        seen.append(q_want.clone())
        masters = {k: v.detach().clone() for k, v in model.state_dict().items()}
        _, q = grad.backward(f_state, f_actions, f_y, f_weights)
        assert torch.equal(q, q_want), s
        assert all(torch.equal(masters[k], v) for k, v in model.state_dict().items())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    grad.check()
    mem.check()
    for h in (grad, fwd, target, mem):
        h.close()


def rel_l2(a, b):
    return float(torch.linalg.norm((a.double() - b.double()).flatten()) / torch.linalg.norm(b.double().flatten()))


def cosine(a, b):
    return float(torch.dot(a.double().flatten(), b.double().flatten()) / (torch.linalg.norm(a.double()) * torch.linalg.norm(b.double())))


@pytest.mark.parametrize("d", (5, 7))
def test_dense_weights_stay_within_the_contracts_own_error(T, d):
    """NN_8 on he_state_dict, 64 records from play, five batches.  Per parameter tensor, the relative L2 error against
    torch's f32 autograd of the kernels and of the contract restated in f32 torch ops (GC.reference_backward): the
    contract's own error is measured on the CPU on all five; the kernels' error on the first batch may exceed the
    largest of the five by a tenth (DESIGN.md 3.7's criterion: the two differ only in the order of their f32 sums).
    The table it prints is kept in profiles/nnw_grad_accuracy.txt."""
    B, net = 64, 8
    sd = K.he_state_dict(net, d)
    model = K.model_of(sd, d).to(DEV)
    target = T.NNWideForward(sd, d, DEV, max_rows=4096)
    mem = GC.play_memory(T, d, 40 + d)
    batches = []
    for _ in range(5):
        state, actions, reward, _, terminal, weights, indices = mem.sample_batch(B, 0.4, next_state=False)
        y = T.learnerTargets(target, mem, indices, reward, terminal)
        batches.append((state, actions, y, weights))
    mem.check()
    cpu = K.model_of(sd, d).train()
    e_contract, f32_grads = [], []
    for state, actions, y, weights in batches:
        s, a, yy, w = state.cpu(), actions.cpu(), y.cpu(), weights.cpu()
        cpu.zero_grad()
        qa = cpu(s.float()).gather(1, a.view(-1, 1)).squeeze(1)
        (w * (yy - qa) ** 2).mean().backward()
        g32 = {k: p.grad.clone() for k, p in cpu.named_parameters()}
        _, gc = GC.reference_backward(sd, s, lambda q: GC.head_contract(q, a, yy, w)[1], dtype=torch.float32)
        e_contract.append({k: rel_l2(gc[k], g32[k]) for k in GC.params(net)})
        f32_grads.append(g32)
    grad = T.NNWideGrad(model, d, DEV, max_batch=B)
    state, actions, y, weights = batches[0]
    loss, q = grad.backward(state, actions, y, weights)
    got = {k: p.grad.cpu() for k, p in model.named_parameters()}
    assert bool(torch.isfinite(loss).all())
    worst = []
    print(f"nnw grad accuracy NN_8 d={d}: {B} records, relative L2 error against torch f32 autograd per tensor: kernels (batch 0) | "
          f"contract in f32 torch ops (batches 0..4) | cosine of the kernels' gradient to f32's")
    for k in GC.params(net):
        e_k, yard = rel_l2(got[k], f32_grads[0][k]), [e[k] for e in e_contract]
        print(f"  {k:15s} {e_k:.5f} | {' '.join(f'{v:.5f}' for v in yard)} | {cosine(got[k], f32_grads[0][k]):.6f}")
        worst.append((e_k / max(yard), k))
    print(f"  largest ratio of the kernels' error to the contract's largest: {max(worst)[0]:.3f} ({max(worst)[1]})")
    for ratio, k in worst:
        assert ratio <= 1.1, (k, ratio)
    for h in (grad, target, mem):
        h.close()
