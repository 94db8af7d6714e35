"""NN_11's learner step (tq_nn11_grad_*, policy.NN11Grad, policy.learnerStep) on the GPU: bit for bit on the two cases
of tests/nn11_grad_cases.py at every size, element type and row count that takes another path; the handle's scratch,
its argument checks, trained weights against torch's f32 autograd, and twenty learner steps on a replay memory."""
import ctypes as C
import os

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

import numpy as np
import pytest
import torch

import nn11_cases as K
import nn11_grad_cases as GC

pytestmark = pytest.mark.gpu
DTYPES = (torch.uint8, torch.float32, torch.float16, torch.bfloat16)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def T():
    import toric_rl_decoder_amd as T
    assert torch.cuda.is_available()
    T.load()
    return T


@pytest.fixture(scope="module")
def handles(T):
    """one (model, NN11Grad of the largest row count) per size, reloaded for every network"""
    made = {}
    yield made
    for _, g in made.values():
        g.close()


def handle(T, made, d):
    if d not in made:
        model = T.NN_11(d).to(DEV)
        made[d] = (model, T.NN11Grad(model, d, DEV, max_batch=GC.row_counts(d)[-1]))
    return made[d]


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


@pytest.mark.parametrize("kind", ("integer", "rounding"))
@pytest.mark.parametrize("d", K.SIZES)
def test_both_cases_are_bit_equal_to_their_references(T, handles, d, kind):
    """GC.integer_case (torch's own f32 autograd is the reference) and GC.rounding_case (float64 autograd with G rounded
    to bf16, ties included, every sum exact).  Row counts at the conv kernels' tile and workgroup edges and around the
    wgrad workgroup's record count, descending then ascending on one handle, so that a larger step leaves its
    activations, gradients and partial images in the scratch of a smaller one; the handle held another network before."""
    c = GC.integer_case(d) if kind == "integer" else GC.rounding_case(d)
    model, grad = handle(T, handles, d)
    model.load_state_dict({k: -v for k, v in c["sd"].items()})
    grad.load()
    model.load_state_dict(c["sd"])
    grad.load()
    fwd = T.NN11Forward(c["sd"], d, DEV, max_rows=GC.row_counts(d)[-1])
    counts = GC.row_counts(d)
    assert counts[-1] == c["x"].shape[0] == grad.max_batch
    i = K.SIZES.index(d) + (kind == "rounding")
    for dt in DTYPES if d == 7 else (DTYPES[i % 4],):
        x = torch.from_numpy(c["x"]).to(DEV).to(dt)
        for n in counts[::-1] + counts:
            w, want_loss, want = GC.at_rows(c, n)
            loss, q, got = step(grad, model, c, x, n, w)
            assert q.dtype == loss.dtype == torch.float32 and tuple(q.shape) == (n, 3) and tuple(loss.shape) == (n,)
            assert torch.equal(q, fwd(x[:n])) and np.array_equal(q.cpu().numpy(), c["q"][:n]), (d, kind, dt, n)
            assert np.array_equal(loss.cpu().numpy(), want_loss), (d, kind, dt, n)
            for k in GC.PARAMS:
                assert np.array_equal(got[k], want[k]), (d, kind, dt, n, k, int((got[k] != want[k]).sum()), want[k].size)
    grad.check()
    fwd.close()


@pytest.mark.parametrize("d", (3, 5))
def test_a_forward_and_a_grad_handle_hold_the_same_network_after_every_load(T, d):
    """Both handles keep their packed network in one struct with one load and one forward.  Given the same integer
    network, and then reloaded with a second one (the conv stack of another size's integer network under the negated
    linear layer), an NN11Forward and an NN11Grad give the same Q bits on one workgroup's perspectives and one more:
    torch's own f32 bits, since every activation is a small integer (asserted)."""
    n = K.group(d) + 1
    c = GC.integer_case(d)
    second = dict(K.integer_state_dict(d + 2))
    second["linear1.weight"], second["linear1.bias"] = -c["sd"]["linear1.weight"], -c["sd"]["linear1.bias"]
    x = torch.from_numpy(c["x"][:n]).to(DEV)
    a, y = c["actions"][:n].to(DEV), c["y"][:n].to(DEV)
    model = T.NN_11(d).to(DEV)
    model.load_state_dict(c["sd"])
    grad = T.NN11Grad(model, d, DEV, max_batch=n)
    fwd = T.NN11Forward(c["sd"], d, DEV, max_rows=n)
    seen = []
    for sd in (c["sd"], second):
        outs, want = K.layer_outputs(K.model_of(sd, d), torch.from_numpy(c["x"][:n]).float())
        assert all(bool((o == o.round()).all()) and float(o.max()) < 256 for o in outs) and bool(outs[-1].any())
        if sd is second:
            model.load_state_dict(sd)
            grad.load()
            fwd.load(sd)
        _, q = grad.backward(x, a, y)
        assert torch.equal(q, fwd(x)) and np.array_equal(q.cpu().numpy(), want.numpy()), d
        seen.append(want)
    assert np.array_equal(seen[0].numpy(), c["q"][:n]) and not torch.equal(seen[0], seen[1])
    grad.check()
    grad.close()
    fwd.close()


@pytest.mark.parametrize("d", (7, 17))
def test_a_step_after_a_larger_one_gives_the_bits_of_a_fresh_handle(T, d):
    c = GC.rounding_case(d)
    counts = GC.row_counts(d)
    big, small = counts[-1], counts[2]
    x = torch.from_numpy(c["x"]).to(DEV)
    model = T.NN_11(d).to(DEV)
    model.load_state_dict(c["sd"])
    used = T.NN11Grad(model, d, DEV, max_batch=big)
    step(used, model, c, x, big, GC.at_rows(c, big)[0])
    w = GC.at_rows(c, small)[0]
    loss_u, q_u, got_u = step(used, model, c, x, small, w)
    fresh = T.NN11Grad(model, d, DEV, max_batch=big)
    loss_f, q_f, got_f = step(fresh, model, c, x, small, w)
    assert torch.equal(loss_u, loss_f) and torch.equal(q_u, q_f)
    for k in GC.PARAMS:
        assert np.array_equal(got_u[k], got_f[k]), k
        assert np.array_equal(got_u[k], GC.at_rows(c, small)[2][k]), k
    used.close()
    fresh.close()


def test_arguments_are_checked_before_any_launch(T):
    d, n = 3, 8
    c = GC.integer_case(d)
    L = T.load()
    model = T.NN_11(d).to(DEV)
    model.load_state_dict(c["sd"])
    x = torch.from_numpy(c["x"][:n + 1]).to(DEV)
    a, y = c["actions"][:n].to(DEV), c["y"][:n].to(DEV)
    loss = torch.full((n,), 7.0, device=DEV)
    gw = [torch.full_like(p, 7.0) for k, p in model.named_parameters() if k.endswith("weight")]
    gb = [torch.full_like(p, 7.0) for k, p in model.named_parameters() if k.endswith("bias")]
    pw, pb = (C.c_void_p * 12)(*[t.data_ptr() for t in gw]), (C.c_void_p * 12)(*[t.data_ptr() for t in gb])
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(h, state=x, n_=n, a_=a, y_=y, loss_=loss, pw_=pw, pb_=pb):
        return L.tq_nn11_grad_step(h, p(state) if state is not None else None, 3, n_, p(a_) if a_ is not None else None,
                                   p(y_) if y_ is not None else None, None, None, p(loss_) if loss_ is not None else None, pw_, pb_, None)

    raw = C.c_void_p(None)
    assert L.tq_nn11_grad_create(C.byref(raw), d, n, 0) == 0
    assert call(raw) == -1 and b"before" in L.tq_last_error()                  # a step before any load
    assert L.tq_nn11_grad_destroy(raw) == 0
    g = T.NN11Grad(model, d, DEV, max_batch=n)
    torch.cuda.synchronize()
    assert call(g._h, n_=n + 1) == -1 and call(g._h, n_=0) == -1 and call(g._h, n_=-3) == -1
    for kw in (dict(state=None), dict(a_=None), dict(y_=None), dict(loss_=None), dict(pw_=None), dict(pb_=None)):
        assert call(g._h, **kw) == -1, kw
    hole = (C.c_void_p * 12)(*[t.data_ptr() for t in gw[:5]] + [None] + [t.data_ptr() for t in gw[6:]])
    assert call(g._h, pw_=hole) == -1
    odd = x[1:]                                                 # contiguous, 18 bytes past an aligned address
    assert odd.is_contiguous() and odd.data_ptr() % 16 != 0
    assert call(g._h, state=odd) == -1 and b"16-byte aligned" in L.tq_last_error()
    with pytest.raises(ValueError, match="16-byte aligned"):
        g.backward(odd, a, y)
    torch.cuda.synchronize()
    assert bool((loss == 7.0).all()) and all(bool((t == 7.0).all()) for t in gw + gb)
    assert call(g._h) == 0                                      # the same call with nothing wrong is taken
    torch.cuda.synchronize()
    assert not bool((loss == 7.0).any())
    g.check()
    bad = a.clone()
    bad[2] = 3
    l2, _ = g.backward(x[:n], bad, y)                           # an action outside 0..2: no loss, the latch
    assert float(l2[2]) == 0.0
    with pytest.raises(ValueError, match="actions_idx"):
        g.check()
    g.check()
    g.close()
    g.close()


def rel_l2(a, b):
    return float(torch.linalg.norm((a.double() - b.double()).flatten()) / torch.linalg.norm(b.double().flatten()))


def cosine(a, b):
    return float(torch.dot(a.double().flatten(), b.double().flatten()) / (torch.linalg.norm(a.double()) * torch.linalg.norm(b.double())))


@pytest.mark.parametrize("d", (5, 7))
def test_trained_weights_stay_within_the_contracts_own_error(T, d):
    """Per parameter tensor, the relative L2 error against torch's f32 autograd of the kernels and of the contract
    restated in f32 torch ops (GC.reference_backward): over five batches of 64 records the contract's own error is
    measured on the CPU; the kernels' error on the first batch may exceed the largest of the five by a tenth.  The two
    differ only in the order of their f32 sums."""
    B = 64
    sd = K.trained_state_dict(d)
    model = K.model_of(sd, d).to(DEV)
    mem = GC.play_memory(T, d, 40 + d)
    batches = []
    for _ in range(5):
        state, actions, reward, _, terminal, weights, indices = mem.sample_batch(B, 0.4, next_state=False)
        y = T.learnerTargets(model, mem, indices, reward, terminal)
        batches.append((state, actions, y, weights))
    mem.check()
    cpu = K.model_of(sd, d).train()
    e_contract, f32_grads = [], []
    for state, actions, y, weights in batches:
        s, a, yy, w = state.cpu(), actions.cpu(), y.cpu(), weights.cpu()
        cpu.zero_grad()
        qa = cpu(s).gather(1, a.view(-1, 1)).squeeze(1)
        (w * (yy - qa) ** 2).mean().backward()
        g32 = {k: p.grad.clone() for k, p in cpu.named_parameters()}
        _, gc = GC.reference_backward(sd, s, lambda q: GC.head_contract(q, a, yy, w)[1], dtype=torch.float32)
        e_contract.append({k: rel_l2(gc[k], g32[k]) for k in GC.PARAMS})
        f32_grads.append(g32)
    grad = T.NN11Grad(model, d, DEV, max_batch=B)
    state, actions, y, weights = batches[0]
    loss, q = grad.backward(state, actions, y, weights)
    got = {k: p.grad.cpu() for k, p in model.named_parameters()}
    assert bool(torch.isfinite(loss).all())
    worst = []
    print(f"nn11 grad accuracy d={d}: {B} records, relative L2 error against torch f32 autograd per tensor: kernels (batch 0) | "
          f"contract in f32 torch ops (batches 0..4) | cosine of the kernels' gradient to f32's")
    for k in GC.PARAMS:
        e_k, yard = rel_l2(got[k], f32_grads[0][k]), [e[k] for e in e_contract]
        print(f"  {k:15s} {e_k:.5f} | {' '.join(f'{v:.5f}' for v in yard)} | {cosine(got[k], f32_grads[0][k]):.6f}")
        worst.append((e_k / max(yard), k))
    print(f"  largest ratio of the kernels' error to the contract's largest: {max(worst)[0]:.3f} ({max(worst)[1]})")
    for ratio, k in worst:
        assert ratio <= 1.1, (k, ratio)
    grad.close()
    mem.close()


def test_twenty_learner_steps_on_one_sample_lower_the_loss_and_write_the_priorities(T):
    d, B, beta, alpha, steps, lr = 5, 64, 0.4, 0.6, 20, 1e-4      # 1e-3 diverges in f32 torch as well: y is near 100
    mem = GC.play_memory(T, d, 77)
    target = T.NN11Forward(K.trained_state_dict(d), d, DEV, max_rows=4096)
    torch.manual_seed(5)
    model = T.NN_11(d).to(DEV)
    twin = T.NN_11(d).to(DEV)
    twin.load_state_dict(model.state_dict())
    grad = T.NN11Grad(model, d, DEV, max_batch=B)
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    batch = mem.sample_batch(B, beta, next_state=False)
    state, actions, reward, _, terminal, weights, indices = batch
    mean = []
    for s in range(steps):
        before = mem.leaves().cpu().numpy()
        loss, idx = T.learnerStep(grad, target, mem, opt, B, beta, batch=batch)
        assert torch.equal(idx, indices) and bool(torch.isfinite(loss).all())
        mean.append(float(loss.mean()))
        if s in (0, steps - 1):                                 # the tree holds |loss| of this step (last occurrence wins)
            want = before.copy()
            for i, v in zip(idx.cpu().numpy(), loss.abs().cpu().numpy()):
                want[i] = np.float64(v) ** alpha
            got = mem.leaves().cpu().numpy()
            assert np.all(np.abs(got - want) <= np.spacing(np.abs(want)))
    grad.check()
    mem.check()
    y = T.learnerTargets(target, mem, indices, reward, terminal)
    opt32, mean32 = torch.optim.SGD(twin.parameters(), lr=lr), []
    for s in range(steps):
        opt32.zero_grad()
        l32 = weights * (y - twin(state).gather(1, actions.view(-1, 1)).squeeze(1)) ** 2
        l32.mean().backward()
        opt32.step()
        mean32.append(float(l32.mean()))
    print(f"learnerStep d={d}, batch {B}, SGD lr {lr}, {steps} steps on one sample: mean loss per step\n"
          f"  NN11Grad  {' '.join(f'{v:.4f}' for v in mean)}\n  torch f32 {' '.join(f'{v:.4f}' for v in mean32)}")
    assert all(np.isfinite(mean)) and mean[-1] < mean[0], mean
    grad.close()
    target.close()
    mem.close()
