"""NN_11's optimizer step (tq_nn11_grad_opt_step, policy.NN11Optimizer) on the GPU: bit for bit on the cases of
tests/nn11_opt_cases.py; the re-pack against tq_nn11_grad_load; chained steps on real gradients; the argument checks;
torch.optim interop; and twenty learner steps without a load()."""
import copy
import ctypes as C
import os

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

import numpy as np
import pytest
import torch

import nn11_cases as K
import nn11_grad_cases as GC
import nn11_opt_cases as OC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = OC.HYPER


@pytest.fixture(scope="module")
def T():
    import toric_rl_decoder_amd as T
    assert torch.cuda.is_available()
    T.load()
    return T


def state_of(opt, i):
    """(m, v) of parameter i as numpy; m None for RMSprop"""
    return (None if opt._m is None else opt._m[i].cpu().numpy()), opt._v[i].cpu().numpy()


def fixed_batch(d, n=8):
    c = GC.integer_case(d)
    return (torch.from_numpy(c["x"][:n]).to(DEV), c["actions"][:n].to(DEV), c["y"][:n].to(DEV),
            torch.linspace(0.5, 1.5, n, device=DEV))


@pytest.mark.parametrize("d", (3, 5))
@pytest.mark.parametrize("kind", OC.KINDS)
def test_a_step_gives_the_contracts_bits_for_all_24_tensors(T, kind, d):
    """d = 3: the smallest linear layer (192 weights) and the 3-element bias on the scalar tail; d = 5: another linear
    size; conv7's and conv10's weights and five conv biases are no multiple of 4 either.  t = 1, 2 and 1000."""
    model = T.NN_11(d).to(DEV)
    grad = T.NN11Grad(model, d, DEV, max_batch=8)
    opt = T.NN11Optimizer(grad, kind)
    params = dict(model.named_parameters())
    assert list(params) == OC.PARAMS
    for t in OC.STEPS:
        case = OC.model_case(d, kind, t)
        with torch.no_grad():
            for i, (name, tc) in enumerate(case.items()):
                params[name].copy_(torch.from_numpy(tc["p"]))
                params[name].grad = torch.from_numpy(tc["g"]).to(DEV)
                opt._v[i].copy_(torch.from_numpy(tc["v"]))
                if kind == "Adam":
                    opt._m[i].copy_(torch.from_numpy(tc["m"]))
        grad.load()
        opt.step_count = t - 1
        opt.step()
        assert opt.step_count == t
        for i, (name, tc) in enumerate(case.items()):
            m, v = state_of(opt, i)
            for got, want, what in zip((params[name].detach().cpu().numpy(), m, v), tc["want"], ("p", "m", "v")):
                assert (got is None and want is None) or OC.same_bits(got, want), \
                    (kind, d, t, name, what, int((OC.bits(got) != OC.bits(want)).sum()), got.size)
            assert OC.same_bits(params[name].grad.cpu().numpy(), tc["g"])       # the gradients are only read
    grad.check()
    grad.close()


@pytest.mark.parametrize("kind,steps", (("Adam", 2), ("RMSprop", 1)))
def test_the_repack_is_loads(T, kind, steps):
    """after a step and no load(), a backward gives the bits of a second handle that packed the updated masters through
    tq_nn11_grad_load: q, loss and all 24 gradients"""
    d = 5
    model = K.model_of(K.trained_state_dict(d), d).to(DEV)
    grad = T.NN11Grad(model, d, DEV, max_batch=8)
    opt = T.NN11Optimizer(grad, kind)
    x, a, y, w = fixed_batch(d)
    _, q_before = grad.backward(x, a, y, w)
    for s in range(steps):
        opt.step()
        loss, q = grad.backward(x, a, y, w)
        got = {k: p.grad.clone() for k, p in model.named_parameters()}
        twin = copy.deepcopy(model)
        for p in twin.parameters():
            p.grad = None
        fresh = T.NN11Grad(twin, d, DEV, max_batch=8)
        loss_f, q_f = fresh.backward(x, a, y, w)
        assert torch.equal(q, q_f) and torch.equal(loss, loss_f), (kind, s)
        for k, p in twin.named_parameters():
            assert torch.equal(got[k], p.grad), (kind, s, k)
        assert not torch.equal(q, q_before)                     # the step did change what the forward reads
        q_before = q
        fresh.close()
    grad.check()
    grad.close()


@pytest.mark.parametrize("kind", OC.KINDS)
def test_five_chained_steps_on_real_gradients(T, kind):
    d = 5
    model = K.model_of(K.trained_state_dict(d), d).to(DEV)
    grad = T.NN11Grad(model, d, DEV, max_batch=8)
    opt = T.NN11Optimizer(grad, kind)
    x, a, y, w = fixed_batch(d)
    params = list(model.parameters())
    for t in range(1, 6):
        grad.backward(x, a, y, w)
        c = OC.consts(kind, t)
        want = []
        for i, p in enumerate(params):
            m, v = state_of(opt, i)
            want.append(OC.update(kind, c, p.detach().cpu().numpy(), p.grad.cpu().numpy(), m, v))
        opt.step()
        for i, p in enumerate(params):                          # then on from the device's values
            m, v = state_of(opt, i)
            for got, ref, what in zip((p.detach().cpu().numpy(), m, v), want[i], ("p", "m", "v")):
                assert (got is None and ref is None) or OC.same_bits(got, ref), (kind, t, OC.PARAMS[i], what)
        assert any(float(p.grad.abs().max()) > 0 for p in params)
    grad.check()
    grad.close()


def test_arguments_are_checked_before_any_launch(T):
    d = 3
    L = T.load()
    torch.manual_seed(3)
    model = T.NN_11(d).to(DEV)
    g = T.NN11Grad(model, d, DEV, max_batch=8)
    flat = [p for pair in g._params for p in pair]
    before = [p.detach().clone() for p in flat]
    mk = lambda fill: [torch.full_like(p, fill) for p in flat]
    grads, m, v = mk(0.5), mk(0.0), mk(0.0)
    arr = lambda ts, which: (C.c_void_p * 12)(*[t.data_ptr() for t in ts[which::2]])
    ok = dict(kind=0, lr=H["lr"], b1=0.9, b2=0.999, eps=1e-8, alpha=0.99, step=1,
              w=arr(flat, 0), b=arr(flat, 1), gw=arr(grads, 0), gb=arr(grads, 1), mw=arr(m, 0), mb=arr(m, 1), vw=arr(v, 0), vb=arr(v, 1))

    def call(h, **kw):
        a = {**ok, **kw}
        return L.tq_nn11_grad_opt_step(h, a["kind"], a["lr"], a["b1"], a["b2"], a["eps"], a["alpha"], a["step"], a["w"], a["b"],
                                       a["gw"], a["gb"], a["mw"], a["mb"], a["vw"], a["vb"], None)

    assert call(None) == -1
    raw = C.c_void_p(None)
    assert L.tq_nn11_grad_create(C.byref(raw), d, 8, 0) == 0
    assert call(raw) == -1 and b"before" in L.tq_last_error()                  # a handle that was never loaded
    assert L.tq_nn11_grad_destroy(raw) == 0
    for kw in (dict(kind=2), dict(kind=-1), dict(lr=-1e-3), dict(lr=float("nan")), dict(eps=-1e-8), dict(b1=1.0), dict(b1=-0.5),
               dict(b2=1.0), dict(b2=2.0), dict(kind=1, alpha=1.0), dict(kind=1, alpha=-0.1), dict(step=0), dict(step=-1),
               dict(w=None), dict(b=None), dict(gw=None), dict(gb=None), dict(vw=None), dict(vb=None), dict(mw=None), dict(mb=None),
               dict(kind=1, vw=None)):
        assert call(g._h, **kw) == -1, kw
    for key, ts, which in (("w", flat, 0), ("b", flat, 1), ("gw", grads, 0), ("gb", grads, 1), ("mw", m, 0), ("mb", m, 1), ("vw", v, 0),
                           ("vb", v, 1)):
        ptrs = [t.data_ptr() for t in ts[which::2]]
        ptrs[5] = None
        assert call(g._h, **{key: (C.c_void_p * 12)(*ptrs)}) == -1, key
    with pytest.raises(ValueError):
        T.NN11Optimizer(g, "Adam", lr=-1.0)
    opt = T.NN11Optimizer(g, "Adam")
    with pytest.raises(ValueError, match="grad"):               # no backward yet
        opt.step()
    assert opt.step_count == 0
    torch.cuda.synchronize()
    for p, was, mm, vv in zip(flat, before, m, v):
        assert torch.equal(p, was) and not bool(mm.any()) and not bool(vv.any())
    assert call(g._h, kind=1, mw=None, mb=None) == 0            # RMSprop does not read exp_avg; nothing wrong: taken
    torch.cuda.synchronize()
    assert all(not torch.equal(p, was) for p, was in zip(flat, before)) and all(bool(vv.any()) for vv in v)
    assert not any(bool(mm.any()) for mm in m)
    g.check()
    g.close()


def torch_optimizer(kind, params, **kw):
    if kind == "Adam":
        return torch.optim.Adam(params, lr=H["lr"], betas=H["betas"], eps=H["eps"], **kw)
    return torch.optim.RMSprop(params, lr=H["lr"], alpha=H["alpha"], eps=H["eps"], **kw)


@pytest.mark.parametrize("kind", OC.KINDS)
def test_state_dicts_go_both_ways_between_torch_and_the_device(T, kind):
    """torch's state after 3 steps loads into NN11Optimizer; one more step on the same gradients in both, and in float64
    from the same state: the device's change is held to the criterion of the host accuracy test, MARGIN times the error
    of torch's own f32 step."""
    d = 3
    torch.manual_seed(11)
    model = T.NN_11(d).to(DEV)
    topt = torch_optimizer(kind, model.parameters())
    gen = torch.Generator(device=DEV).manual_seed(5)
    draw = lambda: [torch.randn(p.shape, generator=gen, device=DEV) * 10.0 ** float(torch.randint(-4, 1, (1,))) for p in model.parameters()]
    for _ in range(3):
        for p, gr in zip(model.parameters(), draw()):
            p.grad = gr
        topt.step()
    last = draw()
    start = [p.detach().clone() for p in model.parameters()]
    sd = copy.deepcopy(topt.state_dict())
    twin = copy.deepcopy(model)
    grad = T.NN11Grad(twin, d, DEV, max_batch=8)
    opt = T.NN11Optimizer(grad, kind)
    opt.load_state_dict(sd)
    assert opt.step_count == 3
    m64 = copy.deepcopy(model).double()
    o64 = torch_optimizer(kind, m64.parameters(), foreach=False)
    o64.load_state_dict(copy.deepcopy(sd))                      # torch casts the state to the parameters' float64
    for ps, grads in ((model.parameters(), last), (twin.parameters(), last), (m64.parameters(), [x.double() for x in last])):
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
    topt.step()
    opt.step()
    o64.step()
    flat = lambda ps: torch.cat([p.detach().double().flatten() for p in ps]).cpu().numpy()
    p0, ref = flat(start), flat(m64.parameters())
    e_dev, e_torch = OC.change_error(flat(twin.parameters()), p0, ref), OC.change_error(flat(model.parameters()), p0, ref)
    print(f"nn11 opt interop {kind}: error of the 4th step's change against float64: device {e_dev:.3e}, torch f32 {e_torch:.3e}")
    assert e_dev <= OC.MARGIN * e_torch, (e_dev, e_torch)
    # and back: the device's state_dict loads into torch on the same model, with the state and the step count
    back = opt.state_dict()
    t2 = torch_optimizer(kind, twin.parameters())
    t2.load_state_dict(back)
    got = t2.state_dict()
    assert got["param_groups"] == topt.state_dict()["param_groups"]
    for i in range(24):
        assert float(got["state"][i]["step"]) == 4.0
        key = "exp_avg_sq" if kind == "Adam" else "square_avg"
        assert torch.equal(got["state"][i][key], opt._v[i]) and got["state"][i][key].data_ptr() != opt._v[i].data_ptr()
    for change in (dict(weight_decay=0.1), dict(amsgrad=True) if kind == "Adam" else dict(centered=True)):
        bad = copy.deepcopy(sd)
        bad["param_groups"][0].update(change)
        with pytest.raises(ValueError):
            opt.load_state_dict(bad)
    assert opt.step_count == 4
    grad.check()
    grad.close()


def test_twenty_learner_steps_without_a_load(T):
    """learnerStep with NN11Optimizer (Adam, lr 0.00025) next to torch.optim.Adam(foreach=False) + load() on a twin model
    and twin handle, on one fixed sample: finite losses, a clean latch, and if torch's loss fell the device's did too.
    The trajectories are printed (profiles/nn11_opt_accuracy.txt holds them); no number is put on their distance."""
    d, B, beta, steps = 5, 64, 0.4, 20
    mem = GC.play_memory(T, d, 78)
    target = T.NN11Forward(K.trained_state_dict(d), d, DEV, max_rows=4096)
    torch.manual_seed(6)
    model = T.NN_11(d).to(DEV)
    twin = copy.deepcopy(model)
    batch = mem.sample_batch(B, beta, next_state=False)
    runs = {}
    for name, net in (("NN11Optimizer", model), ("torch Adam + load()", twin)):
        grad = T.NN11Grad(net, d, DEV, max_batch=B)
        if name == "NN11Optimizer":
            opt = T.NN11Optimizer(grad, "Adam", lr=H["lr"])
        else:
            opt = torch.optim.Adam(net.parameters(), lr=H["lr"], foreach=False)
        loads, real_load = [], grad.load
        grad.load = lambda: (loads.append(1), real_load())[1]
        mean = []
        for _ in range(steps):
            loss, idx = T.learnerStep(grad, target, mem, opt, B, beta, batch=batch)
            assert torch.equal(idx, batch[6]) and bool(torch.isfinite(loss).all()), name
            mean.append(float(loss.mean()))
        grad.check()
        assert len(loads) == (0 if name == "NN11Optimizer" else steps), (name, len(loads))
        runs[name] = mean
        grad.close()
    mem.check()
    print(f"learnerStep d={d}, batch {B}, Adam lr {H['lr']}, {steps} steps on one sample: mean loss per step")
    for name, mean in runs.items():
        print(f"  {name:20s} {' '.join(f'{v:.4f}' for v in mean)}")
    ours, torchs = runs["NN11Optimizer"], runs["torch Adam + load()"]
    assert all(np.isfinite(ours)) and all(np.isfinite(torchs))
    if torchs[-1] < torchs[0]:
        assert ours[-1] < ours[0], (ours, torchs)
    target.close()
    mem.close()
