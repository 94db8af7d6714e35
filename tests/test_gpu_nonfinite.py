"""NaN and inf through the network, target and selection kernels on the GPU: the contract of include/toricenv.h
("Non-finite values").  A NaN is compared by position (np.isnan equality), an inf by position and sign, everything else
bit for bit against the same call without the poison or against a fresh handle.  Non-finite values enter only as literal
NaN / inf elements or as one f32 weight beyond bf16's range, so where they end up does not depend on the order of a sum
(plain_cases.order_free_pattern asserts it for every case on the CPU)."""
import copy
import os

os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")

import numpy as np
import pytest
import torch

import nn11_cases as K
import nn11_grad_cases as GC
import nn11_opt_cases as OC
import nnw_cases as KW
import nnw_grad_cases as GW
import plain_cases as P
import resnet_cases as RK
import select_plan_cases as S
from oracle import toric_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
NAN, INF = float("nan"), float("inf")
FLOAT_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
NAN_WORDS = (0x7fffffff, 0xffffffff, 0x7f800001)       # NaNs that a carry out of the rounding turned into -0, +0 and +inf


@pytest.fixture(scope="module")
def T():
    import toric_rl_decoder_amd as T
    assert torch.cuda.is_available()
    T.load()
    return T


# ---- the forward families ----------------------------------------------------------------------------------------------
class Family:
    """One forward family at one size: its He network, its torch model, its contract and its handle."""

    def __init__(self, name, d):
        self.name, self.d = name, d
        if name == "nn11":
            self.sd = P.he_state_dict(K.NET, d)
            last = len(K.CH) - 1
            self.layers = {"early": ("conv2.weight", "conv2.bias", K.CH[1], 9), "last": (f"conv{last}.weight", f"conv{last}.bias", K.CH[last - 1], 9)}
        elif name in ("nn8", "nn17"):
            net = int(name[2:])
            self.sd = KW.he_state_dict(net, d)
            last, ch = KW.layers(net), KW.CH[net]
            self.layers = {"early": ("conv2.weight", "conv2.bias", ch[1], 9), "last": (f"conv{last}.weight", f"conv{last}.bias", ch[last - 1], 9)}
        else:
            net = int(name[6:])
            self.sd = RK.he_state_dict(net)
            bn = {c: (b, s) for c, b, s in RK.convs(net)}
            self.layers = {k: (c + ".weight", bn[c][0] + ".bias", bn[c][1][1], bn[c][1][2] * bn[c][1][3])
                           for k, c in (("early", "layer2.0.conv1"), ("shortcut", "layer2.0.shortcut.0"), ("last", "layer4.1.conv2"))}
            self.bn_weight = {k: bn[c][0] + ".weight" for k, c in (("early", "layer2.0.conv1"), ("last", "layer4.1.conv2"))}

    def model(self, sd):
        if self.name == "nn11":
            return K.model_of(sd, self.d)
        return KW.model_of(sd, self.d) if self.name in ("nn8", "nn17") else RK.model_of(sd)

    def contract(self, sd, x):
        """the f32 contract on the CPU, after the check that an f64 evaluation has the same NaN / inf pattern"""
        fwd = K.contract_forward if not self.name.startswith("resnet") else RK.contract_forward
        return P.order_free_pattern(fwd, self.model(sd), x.cpu()).numpy()

    def handle(self, T, max_rows, sd=None):
        sd = self.sd if sd is None else sd
        if self.name == "nn11":
            return T.NN11Forward(sd, self.d, DEV, max_rows=max_rows)
        cls = T.NNWideForward if self.name in ("nn8", "nn17") else T.ResNetForward
        return cls(sd, self.d, DEV, max_rows=max_rows)

    def poisoned(self, where, kind):
        weight, bias, cin, taps = self.layers[where]
        if kind == "nan batchnorm weight":
            return P.poisoned_state_dict(self.sd, weight, self.bn_weight[where], "nan bias", bias_at=5)
        return P.poisoned_state_dict(self.sd, weight, bias, kind, at=(5 * cin + 3) * taps + taps // 2, bias_at=5)

    def weight_poisons(self):
        out = [(w, k) for w in self.layers for k in P.WEIGHT_POISONS]
        return out + ([(w, "nan batchnorm weight") for w in self.bn_weight] if self.name.startswith("resnet") else [])


FORWARD_CONFIGS = (("nn11", 3), ("nn11", 5), ("nn8", 3), ("nn17", 3), ("resnet18", 3), ("resnet18", 5))
SCRATCH_CONFIGS = tuple((n, d) for n in ("nn11", "nn8", "nn17", "resnet18") for d in (3, 5)) + (("resnet34", 3),)


def float_stack(d, rows):
    return torch.from_numpy(K.dense_rows(d, rows).astype(F32))


@pytest.mark.parametrize("name,d", FORWARD_CONFIGS)
def test_a_poisoned_stack_element_stays_in_its_row_and_goes_where_torch_sends_it(T, name, d):
    """He weights, 2 G + 3 rows on a handle of G + 1: three passes.  A NaN, then a +inf, in one stack element of the
    first row, of the last row of a workgroup and of the first row of the second pass, as f32, f16 and bf16 stacks: every
    other row keeps the bits of the call without poison, and the three rows carry contract_forward's pattern."""
    fam = Family(name, d)
    rows = K.dense_rows_for(d)
    at = P.poison_rows(d, rows)
    f = fam.handle(T, K.group(d) + 1)
    x = float_stack(d, rows)
    clean = {dt: f(x.to(DEV).to(dt)).cpu().numpy() for dt in FLOAT_DTYPES}
    assert all(np.isfinite(q).all() for q in clean.values())
    other = np.setdiff1d(np.arange(rows), at)
    for value in (NAN, INF):
        bad = x.clone()
        for k, r in enumerate(at):
            bad[r, k % 2, (d // 2 + k) % d, k % d] = value
        want = fam.contract(fam.sd, bad[at])                    # torch's rows do not meet either: the three rows are enough
        assert P.pattern(want).any(axis=1).all()
        for dt in FLOAT_DTYPES:
            got = f(bad.to(DEV).to(dt)).cpu().numpy()
            assert np.array_equal(got[other].view(np.uint32), clean[dt][other].view(np.uint32)), (name, d, value, dt)
            assert P.same_pattern(got[at], want), (name, d, value, dt, P.pattern(got)[at].tolist(), P.pattern(want).tolist())
    # NaNs whose rounding carried out of the exponent: as the same stack converted to bf16 by torch
    words = x.clone()
    for k, r in enumerate(at):
        words[r].view(-1).view(torch.int32)[k + 1] = int(np.array(NAN_WORDS[k], np.uint32).view(np.int32))
    assert int(torch.isnan(words).sum()) == 3 and int(torch.isnan(words.bfloat16()).sum()) == 3
    got, want = f(words.to(DEV)).cpu().numpy(), f(words.bfloat16().to(DEV)).cpu().numpy()
    assert P.same_bits_nan_equal(got, want) and np.isnan(got[at]).any(axis=1).all() and np.isfinite(got[other]).all(), (name, d)
    f.close()


@pytest.mark.parametrize("name,d", FORWARD_CONFIGS)
def test_a_poisoned_weight_goes_where_torch_sends_it_and_a_reload_removes_it(T, name, d):
    """One NaN conv weight, one f32 weight of 3.4e38 (bf16's inf) and one NaN bias (a ResNet: BatchNorm's beta, and a NaN
    gamma), in an early layer -- the poison then passes ReLUs, roundings and the zero padding, where 0 x inf is a NaN --
    and in the last one, where under the inf weight the rows differ: +inf where the activation it meets is positive, NaN
    where it is 0.  One handle of G + 1 rows, reloaded, on G + 3 rows of which the contract is evaluated on every fifth;
    the clean network afterwards gives the bits it gave before."""
    fam = Family(name, d)
    rows = K.group(d) + 3
    x8 = torch.from_numpy(K.dense_rows(d, rows))
    f = fam.handle(T, K.group(d) + 1)
    clean = f(x8.to(DEV)).cpu().numpy()
    for where, kind in fam.weight_poisons():
        sd = fam.poisoned(where, kind)
        want = fam.contract(sd, x8[::5])
        got = f.load(sd)(x8.to(DEV)).cpu().numpy()
        assert P.pattern(got).any(axis=1).all(), (name, d, where, kind)
        assert P.same_pattern(got[::5], want), (name, d, where, kind, P.pattern(got[::5]).tolist(), P.pattern(want).tolist())
    assert np.array_equal(f.load(fam.sd)(x8.to(DEV)).cpu().numpy().view(np.uint32), clean.view(np.uint32))
    f.close()


@pytest.mark.parametrize("name,d", SCRATCH_CONFIGS)
def test_a_forward_after_a_call_full_of_nan_gives_the_bits_of_a_fresh_handle(T, name, d):
    """0 x NaN is not 0: after a call at the handle's full rows with a NaN in every stack element, every activation image
    of the scratch is NaN, and a read beyond a later call's own rows shows, which finite leftovers under zero weights,
    masks and padded channels do not."""
    fam = Family(name, d)
    g = K.group(d)
    x = torch.from_numpy(K.dense_rows(d, g + 1)).to(DEV)
    fresh, used = fam.handle(T, g + 1), fam.handle(T, g + 1)
    full = used(torch.full((g + 1, 2, d, d), NAN, device=DEV))
    assert bool(torch.isnan(full).all())
    for n in sorted({1, g, g + 1}):
        want, got = fresh(x[:n]), used(x[:n])
        assert bool(torch.isfinite(want).all()) and torch.equal(got.view(torch.int32), want.view(torch.int32)), (name, d, n)
    fresh.close()
    used.close()


# ---- the learner step --------------------------------------------------------------------------------------------------
class Learner:
    """One net's learner step at one size.  integer: the integer network, whose activations are small integers, so that the
    ReLU masks -- signs of finite sums, which decide where a NaN gradient passes -- are torch's own whatever the order of
    the sums; else He weights."""

    def __init__(self, name, d, integer=False):
        self.name, self.d = name, d
        self.net = 11 if name == "nn11" else int(name[2:])
        bound = K.NET if name == "nn11" else KW.BOUND[self.net]
        self.sd = P.integer_state_dict(bound, d) if integer else P.he_state_dict(bound, d)
        self.params = GC.PARAMS if name == "nn11" else GW.params(self.net)
        self.wgrad_persp = (GC if name == "nn11" else GW).wgrad_persp(d)
        self.reference_backward = (GC if name == "nn11" else GW).reference_backward

    def model(self, T):
        m = (T.NN_11 if self.name == "nn11" else KW.MODULES[self.net])(self.d).to(DEV)
        m.load_state_dict(self.sd)
        return m

    def grad(self, T, model, max_batch):
        return (T.NN11Grad if self.name == "nn11" else T.NNWideGrad)(model, self.d, DEV, max_batch=max_batch)

    def batch(self, n, seed=0):
        """-> (x f32 (n,2,d,d), actions i64, y f32, w f32) on the CPU"""
        g = torch.Generator().manual_seed(4100 + 10 * self.d + seed)
        x = float_stack(self.d, n)
        return x, torch.randint(0, 3, (n,), generator=g), torch.randn(n, generator=g), 0.5 + torch.rand(n, generator=g)


def learner_step(grad, model, x, a, y, w):
    for p in model.parameters():
        if p.grad is not None:
            p.grad.fill_(7.0)                                   # gradients are written, not accumulated
    loss, q = grad.backward(x.to(DEV), a.to(DEV), y.to(DEV), w.to(DEV))
    return loss.cpu(), q.cpu(), {k: p.grad.cpu().numpy() for k, p in model.named_parameters()}


LEARNER_CONFIGS = (("nn11", 3), ("nn11", 5), ("nn8", 3), ("nn17", 3))


@pytest.mark.parametrize("name,d", LEARNER_CONFIGS)
def test_a_poisoned_record_of_a_learner_step(T, name, d):
    """n = G + 1 records, one of them (the last of the first workgroup) poisoned in turn by y = NaN, weight = inf and a
    NaN stack element.  loss and q of the other records keep the clean step's bits; the record's own follow the head's
    contract; every gradient tensor's NaN mask is that of the f32 autograd of the contract on the CPU (on the integer
    network: the masks of the backward are signs of finite sums, and only there are they torch's for certain), with the zero
    padding's zeros as terms of the sums (reference_backward's pad_explicitly: the kernels multiply them, and torch's own
    padded conv2d leaves them out in f32 and multiplies them in f64); the f64 autograd must give the same masks."""
    net = Learner(name, d, integer=True)
    n = K.group(d) + 1
    r = n - 2
    x, a, y, w = net.batch(n)
    model = net.model(T)
    grad = net.grad(T, model, n)
    loss0, q0, g0 = learner_step(grad, model, x, a, y, w)
    assert bool(torch.isfinite(loss0).all()) and all(np.isfinite(v).all() for v in g0.values())
    others = torch.arange(n) != r
    for kind in GC.LEARNER_POISONS:
        xb, yb, wb = GC.poisoned_batch(kind, r, x, y, w)
        loss, q, got = learner_step(grad, model, xb, a, yb, wb)
        assert torch.equal(loss[others].view(torch.int32), loss0[others].view(torch.int32)), (name, d, kind)
        assert torch.equal(q[others].view(torch.int32), q0[others].view(torch.int32)), (name, d, kind)
        if kind == "stack nan":
            assert P.same_pattern(q, P.order_free_pattern(K.contract_forward, K.model_of(net.sd, d) if name == "nn11" else KW.model_of(net.sd, d), xb))
        else:
            assert torch.equal(q.view(torch.int32), q0.view(torch.int32))
        want_loss, _ = GC.head_contract(q, a, yb, wb)
        assert P.same_bits_nan_equal(loss.numpy(), want_loss.numpy()) and P.pattern(loss)[r] != P.FINITE, (name, d, kind, loss[r])
        dq = lambda qq: GC.head_contract(qq.float(), a, yb, wb)[1]
        _, ref = net.reference_backward(net.sd, xb, dq, dtype=torch.float32, pad_explicitly=True)
        _, r64 = net.reference_backward(net.sd, xb, dq, dtype=torch.float64, exact=False, pad_explicitly=True)
        assert all(torch.equal(torch.isnan(ref[k]), torch.isnan(r64[k])) for k in net.params), "not a case"
        masks = {k: (int(np.isnan(got[k]).sum()), int(torch.isnan(ref[k]).sum()), got[k].size) for k in net.params}
        wrong = {k: v for k, v in masks.items() if not np.array_equal(np.isnan(got[k]), torch.isnan(ref[k]).numpy())}
        assert not wrong, (name, d, kind, wrong)
        assert any(v[0] for v in masks.values()), (name, d, kind)
    grad.check()
    grad.close()


@pytest.mark.parametrize("name,d", tuple((n, d) for n in ("nn11", "nn8", "nn17") for d in (3, 5)))
def test_a_learner_step_after_one_full_of_nan_gives_the_bits_of_a_fresh_handle(T, name, d):
    """A step at the handle's full p + 1 records with a NaN in every stack element and every y leaves NaN in the kept
    activations, the G images and the partial weight-gradient images; finite steps of 1, G + 1 and p + 1 records then
    give loss, q and every gradient tensor of a fresh handle, bit for bit."""
    net = Learner(name, d)
    big = net.wgrad_persp + 1
    x, a, y, w = net.batch(big, seed=1)
    m_used, m_fresh = net.model(T), net.model(T)
    used, fresh = net.grad(T, m_used, big), net.grad(T, m_fresh, big)
    loss, q, got = learner_step(used, m_used, torch.full_like(x, NAN), a, torch.full_like(y, NAN), w)
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(q).all()) and all(np.isnan(v).all() for v in got.values())
    for n in sorted({1, K.group(d) + 1, big}):
        lu, qu, gu = learner_step(used, m_used, x[:n], a[:n], y[:n], w[:n])
        lf, qf, gf = learner_step(fresh, m_fresh, x[:n], a[:n], y[:n], w[:n])
        assert bool(torch.isfinite(lf).all()) and torch.equal(lu.view(torch.int32), lf.view(torch.int32)), (name, d, n)
        assert torch.equal(qu.view(torch.int32), qf.view(torch.int32)), (name, d, n)
        for k in net.params:
            assert np.isfinite(gf[k]).all() and np.array_equal(gu[k].view(np.uint32), gf[k].view(np.uint32)), (name, d, n, k)
    for h in (used, fresh):
        h.check()
        h.close()


def test_a_nan_weight_in_the_target_network_reaches_the_loss(T):
    """d = 3, B = 8, end to end: a target handle with one NaN weight -> learnerTargets gives a NaN y for every record
    whose next state has a perspective (0 x NaN under the terminal flag is a NaN too, as in the torch expression) and the
    reward for the others -> the learner step's loss is a NaN exactly there.  No optimizer step, no priority update."""
    d, B = 3, 8
    mem = GC.play_memory(T, d, 33)
    net = Learner("nn11", d)
    target = T.NN11Forward(P.poisoned_state_dict(net.sd, "conv2.weight", "conv2.bias", "nan weight", at=77), d, DEV, max_rows=1 << 10)
    state, actions, reward, _, terminal, weights, indices = mem.sample_batch(B, 0.4, next_state=False)
    _, _, counts, _ = mem.next_perspectives(indices)
    y = T.learnerTargets(target, mem, indices, reward, terminal)
    has = counts.cpu().numpy() > 0
    assert np.array_equal(np.isnan(y.cpu().numpy()), has) and has.any()
    assert torch.equal(y[~torch.from_numpy(has).to(DEV)], reward[~torch.from_numpy(has).to(DEV)].clamp(-100, 100))
    model = net.model(T)
    grad = net.grad(T, model, B)
    loss, q = grad.backward(state, actions, y, weights)
    assert bool(torch.isfinite(q).all()) and np.array_equal(np.isnan(loss.cpu().numpy()), has)
    for h in (grad, target, mem):
        h.check()
        h.close()


# ---- the optimizer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", OC.KINDS)
def test_an_optimizer_step_propagates_nan_and_inf_gradients(T, kind):
    """One NN11Optimizer step at d = 3 with NaN, +inf and -inf gradient elements in every tensor: masters and state as
    the numpy contract has them (NaN by position).  With every tensor poisoned, the learner step after it is NaN in every
    output, on this handle and on one that loads the updated masters: that only shows that nothing got stuck finite.
    Where a NaN lands in the conv images is compared by tests/test_nonfinite_host.py (any NaN conv weight makes every
    Q-value a NaN, so no forward can tell); the linear image and bias are told apart by the test below."""
    d, t = 3, 2
    model = T.NN_11(d).to(DEV)
    grad = T.NN11Grad(model, d, DEV, max_batch=8)
    opt = T.NN11Optimizer(grad, kind)
    params = dict(model.named_parameters())
    case = OC.model_case(d, kind, t)
    c = OC.consts(kind, t)
    want = {}
    with torch.no_grad():
        for i, (name, tc) in enumerate(case.items()):
            k = min(3, tc["g"].size // 3)
            g = tc["g"].copy()
            g.reshape(-1)[np.random.default_rng(i).choice(g.size, 3 * k, replace=False)] = np.repeat(np.array([NAN, INF, -INF], F32), k)
            want[name] = OC.update(kind, c, tc["p"], g, tc["m"], tc["v"])
            params[name].copy_(torch.from_numpy(tc["p"]))
            params[name].grad = torch.from_numpy(g).to(DEV)
            opt._v[i].copy_(torch.from_numpy(tc["v"]))
            if kind == "Adam":
                opt._m[i].copy_(torch.from_numpy(tc["m"]))
    grad.load()
    opt.step_count = t - 1
    opt.step()
    for i, name in enumerate(case):
        m = None if opt._m is None else opt._m[i].cpu().numpy()
        for got, ref, what in zip((params[name].detach().cpu().numpy(), m, opt._v[i].cpu().numpy()), want[name], "pmv"):
            assert (got is None and ref is None) or P.same_bits_nan_equal(got, ref), (kind, name, what)
        assert int(np.isnan(want[name][0]).sum()) in (3, 9)
    c8 = GC.integer_case(d)
    x, a, y = torch.from_numpy(c8["x"][:8]).to(DEV), c8["actions"][:8].to(DEV), c8["y"][:8].to(DEV)
    loss, q = grad.backward(x, a, y)
    got = {k: p.grad.clone() for k, p in model.named_parameters()}
    twin = copy.deepcopy(model)
    for p in twin.parameters():
        p.grad = None
    fresh = T.NN11Grad(twin, d, DEV, max_batch=8)
    loss_f, q_f = fresh.backward(x, a, y)
    assert P.same_bits_nan_equal(q.cpu().numpy(), q_f.cpu().numpy()) and P.same_bits_nan_equal(loss.cpu().numpy(), loss_f.cpu().numpy())
    for k, p in twin.named_parameters():
        assert P.same_bits_nan_equal(got[k].cpu().numpy(), p.grad.cpu().numpy()), (kind, k)
    for h in (grad, fresh):
        h.check()
        h.close()


@pytest.mark.parametrize("kind", OC.KINDS)
def test_a_nan_gradient_of_the_linear_layer_lands_in_its_own_place_of_the_image(T, kind):
    """He weights and the real gradients of a step at d = 3; then one NaN in linear1.weight's gradient (row 1) and a +inf
    in linear1.bias's (element 2), and one optimizer step.  Masters and state as the numpy contract gives them from the
    device's own gradients; the re-packed linear image and bias then make the Q-values of actions 1 and 2 NaN in every row
    and leave action 0's finite and bit-equal to a handle that loads the updated masters -- a NaN scattered to another
    row of the image, or dropped, shows."""
    d, n, t = 3, 8, 1
    net = Learner("nn11", d)
    model = net.model(T)
    grad = net.grad(T, model, n)
    opt = T.NN11Optimizer(grad, kind)
    x, a, y, w = net.batch(n, seed=2)
    learner_step(grad, model, x, a, y, w)
    params = dict(model.named_parameters())
    with torch.no_grad():
        params["linear1.weight"].grad[1, 17] = NAN
        params["linear1.bias"].grad[2] = INF
    c = OC.consts(kind, t)
    want = {}
    for i, (name, p) in enumerate(params.items()):
        m = None if opt._m is None else opt._m[i].cpu().numpy()
        want[name] = OC.update(kind, c, p.detach().cpu().numpy(), p.grad.cpu().numpy(), m, opt._v[i].cpu().numpy())
    opt.step()
    for i, (name, p) in enumerate(params.items()):
        m = None if opt._m is None else opt._m[i].cpu().numpy()
        for got, ref, what in zip((p.detach().cpu().numpy(), m, opt._v[i].cpu().numpy()), want[name], "pmv"):
            assert (got is None and ref is None) or P.same_bits_nan_equal(got, ref), (kind, name, what)
    nan_at = {k: np.argwhere(np.isnan(v.detach().cpu().numpy())).tolist() for k, v in params.items()}
    assert {k: v for k, v in nan_at.items() if v} == {"linear1.weight": [[1, 17]], "linear1.bias": [[2]]}, nan_at
    _, q, _ = learner_step(grad, model, x, a, y, w)
    assert bool(torch.isfinite(q[:, 0]).all()) and bool(torch.isnan(q[:, 1:]).all())
    twin = copy.deepcopy(model)
    fresh = net.grad(T, twin, n)
    _, q_f, _ = learner_step(fresh, twin, x, a, y, w)
    assert P.same_bits_nan_equal(q.numpy(), q_f.numpy())
    for h in (grad, fresh):
        h.check()
        h.close()


# ---- maxima and selection against the oracle ---------------------------------------------------------------------------
def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def padded_amax(q, off, largest):
    """predict_max's reduction: np.amax over the slice padded with zero rows up to ``largest`` (None: no padding)"""
    out = np.zeros(off.size - 1, F32)
    for i in range(off.size - 1):
        s = q[off[i]:off[i + 1]].reshape(-1)
        if s.size:
            pad = 0 if largest is None else 3 * (largest - s.size // 3)
            out[i] = np.amax(np.concatenate([s, np.zeros(pad, F32)]))
    return out


def test_segment_max_and_td_target_keep_a_nan_like_np_amax(T):
    q, off = S.nonfinite_slices()
    n = off.size - 1
    longest = int(np.diff(off).max())
    dq, doff = dev(q), dev(off)
    got = T.segment_max(dq, doff).cpu().numpy()
    assert P.same_bits_nan_equal(got, padded_amax(q, off, None))
    got = T.segment_max(dq, doff, torch.tensor([longest], dtype=torch.int32, device=DEV)).cpu().numpy()
    want_m = padded_amax(q, off, longest)
    assert P.same_bits_nan_equal(got, want_m) and np.isnan(want_m).sum() > 20 and np.isneginf(want_m).any() and (want_m == 0).any()
    rng = np.random.default_rng(8)
    r, t = rng.normal(size=n).astype(F32), rng.integers(0, 2, n).astype(bool)
    t[np.isneginf(want_m)] = False                                      # -inf reaches the clamp; under the flag it is 0 x -inf
    want = (torch.from_numpy(r) + (~torch.from_numpy(t)).float() * 0.95 * torch.from_numpy(want_m)).clamp(-100, 100).numpy()
    got = T.td_target(dq, doff, dev(r), dev(t), 0.95).cpu().numpy()
    assert P.same_bits_nan_equal(got, want), np.flatnonzero(np.isnan(got) != np.isnan(want))
    assert np.isnan(want[t]).any() and (want == -100).any()             # 0 x NaN under the flag; -inf clamped


def test_block_priorities_keep_a_nan_like_the_oracle(T):
    d, n, steps = 5, 64, 4
    env = T.make("toric-code-v0", {"size": d, "min_qubit_errors": 0, "p_error": 0.1})
    gpu = T.EnvSet(env, n, device=DEV, seed=91, numpy_io=False)
    gpu.resetAll()
    blk = gpu.newTransitionBlock(steps=steps)
    for s in range(steps):
        gpu.actorStep(None, block=blk, slot=s)
    rng = np.random.default_rng(91)
    q = (rng.normal(size=(steps + 1, n, 3)) * 3).astype(F32)
    flat = q.reshape(-1, 3)
    for i, row in enumerate(rng.choice(flat.shape[0], 60, replace=False)):
        if i < 30:
            flat[row, i % 3] = np.nan                                # each of the three places
        elif i < 40:
            flat[row] = np.nan
        elif i < 50:
            flat[row] = -np.inf
        else:
            flat[row, i % 3], flat[row, (i + 1) % 3] = np.nan, np.inf
    blk.computePriorities(n, steps, dev(q), 0.95)
    u = blk.unpack()
    A = u["action"].cpu().numpy().reshape(steps, n, 4).transpose(1, 0, 2)
    R = u["reward"].cpu().numpy().reshape(steps, n).T
    got = u["priority"].cpu().numpy().reshape(steps, n).T
    Q = q.transpose(1, 0, 2)
    live = A[:, :, 3] > 0
    assert live.all()
    with np.errstate(invalid="ignore"):
        want = O.compute_priorities(A, R, Q[:, :-1], Q[:, 1:], 0.95).astype(F32)
    assert P.same_bits_nan_equal(got, want), int((np.isnan(got) != np.isnan(want)).sum())
    assert np.isnan(want).sum() >= 40 and np.isposinf(want).any()
    gpu.check()
    gpu.close()


def slice_envs(T, n, d=5):
    envs = T.EnvSet(T.make("toric-code-v0", {"size": d, "p_error": 0.1}), n, seed=606, first_env_id=40, numpy_io=False)
    envs.REUSED_PROBE_CANDIDATES = 0
    envs.resetAll()
    return envs


def test_greedy_selection_takes_the_first_nan_like_np_argmax(T):
    """The slices of S.nonfinite_slices (1, 21, 22 and 43 perspectives: 3 cnt straddles one and two rounds of 64 lanes)
    through the handle-bound selection, dense and planned, and the stateless one, at eps = 0."""
    q, off = S.nonfinite_slices()
    n = off.size - 1
    row = (np.arange(q.shape[0]) - np.repeat(off[:-1], np.diff(off))).astype(np.int32)
    pos = np.ascontiguousarray(np.stack([row % 2, row // 2 % 5, row // 10], axis=1))      # a position of its own for every row of a slice
    flat = [int(np.argmax(q[off[i]:off[i + 1]].reshape(-1))) for i in range(n)]
    envs = slice_envs(T, n)
    ep, st = (c.cpu().numpy().astype(np.uint32) for c in envs.getCounters())
    want_act, want_qv, chosen = O.select_action_batch(q, off, pos, 0.0, envs.seed, np.arange(n) + 40, ep, st)
    assert [int(c - off[i]) * 3 + int(a[3]) - 1 for i, (c, a) in enumerate(zip(chosen, want_act))] == flat
    dq, doff, dpos = dev(q), dev(off), dev(pos)
    act, qv = (t.clone() for t in envs.selectAction(dq, 0.0, positions=dpos, offsets=doff))     # the handle's own buffers
    assert np.array_equal(act.cpu().numpy(), want_act), np.flatnonzero((act.cpu().numpy() != want_act).any(axis=1))
    assert P.same_bits_nan_equal(qv.cpu().numpy(), want_qv)
    plan = envs.selectPlan(0.0, offsets=doff)
    assert plan.R == q.shape[0]
    act_p, qv_p = envs.selectAction(dq[plan.rows.long()], 0.0, positions=dpos, offsets=doff, plan=plan)
    assert torch.equal(act_p, act) and torch.equal(qv_p.view(torch.int32), qv.view(torch.int32))     # bit-identical to the dense one
    envs.check()
    envs.close()
    from toric_rl_decoder_amd import policy
    act_s, qv_s = policy._selectActionBatch_prime(q, off[1:], pos, np.ones(n, bool), device=DEV)
    assert np.array_equal(act_s.astype(np.int32), want_act) and P.same_bits_nan_equal(qv_s.astype(F32), want_qv)


class PoisonedQ(torch.nn.Module):
    """A Q-function of the perspective alone with integer weights (any kernel, any batch: the same bits), NaN in one
    column of the rows whose key is 0 mod 4 and +inf in another of those with key 1 mod 8."""

    def __init__(self, d):
        super().__init__()
        rng = np.random.default_rng(d)
        self.w = torch.nn.Parameter(torch.from_numpy(rng.integers(-3, 4, (2 * d * d, 3)).astype(F32)), requires_grad=False)
        self.key = torch.nn.Parameter(torch.from_numpy(rng.integers(1, 50, 2 * d * d).astype(F32)), requires_grad=False)

    def forward(self, x):
        f = x.flatten(1).float()
        q = f @ self.w
        key = (f @ self.key).long()
        rows = torch.arange(q.shape[0], device=q.device)
        q[rows, key % 3] = torch.where(key % 4 == 0, torch.full_like(q[:, 0], NAN), q[rows, key % 3])
        q[rows, (key + 1) % 3] = torch.where(key % 8 == 1, torch.full_like(q[:, 0], INF), q[rows, (key + 1) % 3])
        return q


def test_select_action_entry_points_with_a_model_that_returns_nan(T):
    """selectActionEnvSet dense and sparse and the stateless selectActionBatch at eps = 0 over a model whose Q-table holds
    NaN and +inf: the oracle's selection on the same table."""
    d, n, seed = 5, 200, 707
    model = PoisonedQ(d).to(DEV)
    dense = T.EnvSet(T.make("toric-code-v0", {"size": d, "p_error": 0.12}), n, seed=seed, numpy_io=False)
    sparse = T.EnvSet(T.make("toric-code-v0", {"size": d, "p_error": 0.12}), n, seed=seed, numpy_io=False)
    for e in (dense, sparse):
        e.REUSED_PROBE_CANDIDATES = 0
        e.resetAll()
    states = dense.getStates().cpu().numpy()
    per, pos, cnt, off = O.generate_perspective_batch(states)
    with torch.no_grad():
        q = model.cpu()(torch.from_numpy(per.astype(F32))).numpy()
    model.to(DEV)
    nan_slices = sum(bool(np.isnan(q[off[i]:off[i + 1]]).any()) for i in range(n))
    assert nan_slices > n // 4 and nan_slices < n and np.isposinf(q).any() and cnt.max() >= 22 and cnt.min() <= 21
    ep, st = (c.cpu().numpy().astype(np.uint32) for c in dense.getCounters())
    want_act, want_qv, _ = O.select_action_batch(q, off, pos, 0.0, seed, np.arange(n), ep, st)
    act_d, qv_d = T.selectActionEnvSet(dense, model, 0.0)
    act_s, qv_s = T.selectActionEnvSet(sparse, model, 0.0, sparse=True)
    assert np.array_equal(act_d.cpu().numpy(), want_act) and P.same_bits_nan_equal(qv_d.cpu().numpy(), want_qv)
    assert torch.equal(act_s, act_d) and torch.equal(qv_s.view(torch.int32), qv_d.view(torch.int32))
    act_b, qv_b = T.selectActionBatch(3, 0.0, d // 2, d, states, model, DEV)
    assert np.array_equal(act_b, want_act.astype(np.int64)) and P.same_bits_nan_equal(qv_b.astype(F32), want_qv)
    for e in (dense, sparse):
        e.check()
        e.close()
