"""NN_11's optimizer step without a GPU: the host side of toric-rl-decoder_amd/csrc/nn11_opt.hpp -- the update functions,
nn11_opt_consts, the argument check and the destination functions -- built with g++ through tests/host_nn11_opt_shim.cpp,
against the contract restated in numpy (tests/nn11_opt_cases.py); the contract's accuracy against float64 torch.optim; and
the torch.optim side of policy.NN11Optimizer (state_dict both ways) on CPU tensors.  Test-only build: the product has no
CPU path."""
import copy
import ctypes as C
import types

import numpy as np
import pytest
import torch

import toric_rl_decoder_amd as T

import nn11_opt_cases as OC
from host_build import build_shim
KIND_ID = {"Adam": 0, "RMSprop": 1}
H = OC.HYPER
HYPER_ARGS = (H["lr"], H["betas"][0], H["betas"][1], H["eps"], H["alpha"])


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "host_nn11_opt_shim.cpp", fast=True)
    vp, d = C.c_void_p, C.c_double
    hyper = [C.c_int, d, d, d, d, d, C.c_int64]
    lib.shim_nn11_opt_consts.restype = None
    lib.shim_nn11_opt_consts.argtypes = hyper + [vp]
    lib.shim_nn11_opt_bad_args.restype = C.c_int
    lib.shim_nn11_opt_bad_args.argtypes = hyper
    lib.shim_nn11_opt_update.restype = None
    lib.shim_nn11_opt_update.argtypes = hyper + [C.c_int64, vp, vp, vp, vp]
    lib.shim_nn11_opt_sizes.restype = None
    lib.shim_nn11_opt_sizes.argtypes = [C.c_int, C.c_int, vp]
    lib.shim_nn11_opt_images.restype = None
    lib.shim_nn11_opt_images.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    return lib


def shim_update(shim, kind, t, p, g, m, v, hyper=HYPER_ARGS):
    p, v = p.copy(), v.copy()
    m = None if m is None else m.copy()
    shim.shim_nn11_opt_update(KIND_ID[kind], *hyper, t, p.size, p.ctypes.data, np.ascontiguousarray(g).ctypes.data,
                              None if m is None else m.ctypes.data, v.ctypes.data)
    return p, m, v


@pytest.mark.parametrize("t", OC.STEPS)
@pytest.mark.parametrize("kind", OC.KINDS)
def test_the_headers_update_gives_the_contracts_bits_and_every_mutant_differs(shim, kind, t):
    got_c = np.zeros(7, np.float32)
    shim.shim_nn11_opt_consts(KIND_ID[kind], *HYPER_ARGS, t, got_c.ctypes.data)
    c = OC.consts(kind, t)
    names = ("c1", "c2", "c3", "cb", "ce", "cs", "ca")
    for k, val in zip(names, got_c):
        assert OC.same_bits(np.float32(c.get(k, 0)), val), (k, c.get(k), val)
    case = OC.model_case(3, kind, t)                       # asserts its own coverage and that each mutant differs
    seen = {mu: 0 for mu, kinds in OC.MUTANTS.items() if kind in kinds}
    for name, tc in case.items():
        got = shim_update(shim, kind, t, tc["p"], tc["g"], tc["m"], tc["v"])
        for a, want, what in zip(got, tc["want"], ("p", "m", "v")):
            assert (a is None and want is None) or OC.same_bits(a, want), (name, what, int((OC.bits(a) != OC.bits(want)).sum()))
        for mu in seen:
            mut = OC.update(kind, c, tc["p"], tc["g"], tc["m"], tc["v"], mutant=mu)
            seen[mu] += sum(int((OC.bits(a) != OC.bits(b)).sum()) for a, b in zip(got, mut) if a is not None)
    print(f"nn11 opt {kind} t={t}: elements (of p', m', v' together) that each mutant changes: {seen}")
    assert all(seen.values()), seen


def test_arguments_outside_the_contract_are_refused(shim):
    ok = dict(lr=2.5e-4, b1=0.9, b2=0.999, eps=1e-8, alpha=0.99, step=1)
    call = lambda kind, **kw: shim.shim_nn11_opt_bad_args(kind, *[{**ok, **kw}[k] for k in ("lr", "b1", "b2", "eps", "alpha", "step")])
    assert call(0) == 0 and call(1) == 0 and call(0, lr=0.0, eps=0.0, b1=0.0, b2=0.0) == 0 and call(1, alpha=0.0) == 0
    assert call(2) and call(-1)
    for kind in (0, 1):
        for kw in (dict(lr=-1e-9), dict(lr=float("nan")), dict(eps=-1e-9), dict(eps=float("nan")), dict(step=0), dict(step=-4)):
            assert call(kind, **kw), (kind, kw)
    for kw in (dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=-0.1), dict(b1=float("nan")), dict(b2=1.5)):
        assert call(0, **kw), kw
        assert call(1, **kw) == 0                          # what the kind does not use is not looked at
    for kw in (dict(alpha=1.0), dict(alpha=-0.1), dict(alpha=float("nan"))):
        assert call(1, **kw), kw
        assert call(0, **kw) == 0
    L = T.load()
    assert L.tq_nn11_grad_opt_step(None, 0, 2.5e-4, 0.9, 0.999, 1e-8, 0.99, 1, *([None] * 9)) == -1      # TQ_E_INVALID
    assert "NN11Optimizer" in T.__all__


@pytest.mark.parametrize("d", (3, 5))
def test_the_destinations_are_the_exact_inverses_of_the_packs(shim, d):
    """every element of every layer's weight, distinct per element, scattered into zeroed images: byte for byte the
    header's host packs (forward image, dgrad image, padded bias, linear image), padding included"""
    rng = np.random.default_rng(d)
    for l, name in enumerate(OC.NAMES, start=1):
        sh = OC.shapes(d)
        n = int(np.prod(sh[name + ".weight"]))
        w = (rng.permutation(n) + 1).astype(np.float32) / np.float32(64) * rng.choice((-1, 1), n).astype(np.float32)
        assert len(np.unique(np.abs(w))) == n                  # distinct per element, none zero
        b = rng.normal(size=sh[name + ".bias"]).astype(np.float32)
        sizes = np.zeros(4, np.int64)
        shim.shim_nn11_opt_sizes(l, d, sizes.ctypes.data)
        made = []
        for which in (0, 1):
            wimg, dimg = np.zeros(max(1, sizes[0]), np.uint16), np.zeros(max(1, sizes[1]), np.uint16)
            bias, limg = np.zeros(sizes[2], np.float32), np.zeros(max(1, sizes[3]), np.float32)
            shim.shim_nn11_opt_images(which, l, d, w.ctypes.data, b.ctypes.data, wimg.ctypes.data, dimg.ctypes.data, bias.ctypes.data,
                                      limg.ctypes.data)
            made.append((wimg, dimg, bias, limg))
        for a, bb, what in zip(made[0], made[1], ("forward image", "dgrad image", "bias", "linear image")):
            assert a.tobytes() == bb.tobytes(), (d, name, what)
        img = made[0][0] if l <= 11 else made[0][3]
        assert int((img != 0).sum()) == n, (d, name)                       # every element arrived, none on another's place


def _torch_run(kind, dtype, p0, grads, foreach=None):
    p = torch.tensor(p0, dtype=dtype, requires_grad=True)
    kw = dict(lr=H["lr"], eps=H["eps"], foreach=foreach)
    opt = torch.optim.Adam([p], betas=H["betas"], **kw) if kind == "Adam" else torch.optim.RMSprop([p], alpha=H["alpha"], **kw)
    for g in grads:
        p.grad = torch.tensor(g, dtype=dtype)
        opt.step()
    return p.detach().numpy()


@pytest.mark.parametrize("seed", (0, 1, 2))
@pytest.mark.parametrize("kind", OC.KINDS)
def test_the_contract_is_as_accurate_as_torchs_own_f32_optimizer(kind, seed):
    """50 steps on 4096 elements, lr 0.00025: the relative L2 error of the accumulated change against a float64 run of
    torch.optim may be at most MARGIN times that of torch's own f32 optimizer (foreach=False) against the same run."""
    rng = np.random.default_rng([77, seed])
    n, steps = 4096, 50
    p0 = (rng.normal(size=n) * 0.05).astype(np.float32)
    scale = 10.0 ** rng.uniform(-4, 0, n)
    grads = [(rng.normal(size=n) * scale).astype(np.float32) for _ in range(steps)]
    ref64 = _torch_run(kind, torch.float64, p0, grads, foreach=False)
    t32 = _torch_run(kind, torch.float32, p0, grads, foreach=False)
    p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t, g in enumerate(grads, start=1):
        p, m1, v = OC.update(kind, OC.consts(kind, t), p, g, m, v)
        m = m if m1 is None else m1
    e_contract, e_torch = OC.change_error(p, p0, ref64), OC.change_error(t32, p0, ref64)
    print(f"nn11 opt accuracy {kind} seed {seed}: contract {e_contract:.3e}, torch f32 {e_torch:.3e}, ratio {e_contract / e_torch:.3f}")
    assert e_contract <= OC.MARGIN * e_torch, (e_contract, e_torch)


def cpu_optimizer(kind, d=3, **kw):
    """policy.NN11Optimizer on a CPU model: everything but step() works without a device"""
    torch.manual_seed(d)
    model = T.NN_11(d)
    grad = types.SimpleNamespace(_params=[(getattr(model, n).weight, getattr(model, n).bias) for n in OC.NAMES])
    return model, T.NN11Optimizer(grad, kind, **kw)


def torch_optimizer(kind, model, **kw):
    return torch.optim.Adam(model.parameters(), **kw) if kind == "Adam" else torch.optim.RMSprop(model.parameters(), **kw)


def assert_same_state_dict(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert sorted(a["state"].keys()) == sorted(b["state"].keys())
    for i in a["state"]:
        assert sorted(a["state"][i].keys()) == sorted(b["state"][i].keys()), i
        for k, x in a["state"][i].items():
            y = b["state"][i][k]
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (i, k)


@pytest.mark.parametrize("kind", OC.KINDS)
def test_state_dict_round_trips_with_torch_optim(kind):
    model, opt = cpu_optimizer(kind)
    assert opt.repacks is True and opt.step_count == 0
    opt.zero_grad()
    opt.zero_grad(set_to_none=True)
    fresh = torch_optimizer(kind, model, lr=H["lr"])
    assert_same_state_dict(opt.state_dict(), fresh.state_dict())           # torch's keys and defaults, no state yet
    assert [k for k, _ in model.named_parameters()] == OC.PARAMS
    hyper = dict(lr=1e-3, eps=1e-6, **(dict(betas=(0.8, 0.99)) if kind == "Adam" else dict(alpha=0.9)))
    topt = torch_optimizer(kind, model, **hyper)
    g = torch.Generator().manual_seed(3)
    for _ in range(3):
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        topt.step()
    sd = copy.deepcopy(topt.state_dict())
    opt.load_state_dict(sd)
    assert opt.step_count == 3 and opt.lr == 1e-3 and opt.eps == 1e-6
    assert (opt.betas == (0.8, 0.99)) if kind == "Adam" else (opt.alpha == 0.9)
    back = opt.state_dict()
    assert_same_state_dict(back, sd)
    assert back["state"][0]["step"].dtype == torch.float32 and back["state"][0]["step"].dim() == 0
    for p, v in zip(model.parameters(), opt._v):
        assert v.is_contiguous() and v.dtype == torch.float32 and v.shape == p.shape
    again = torch_optimizer(kind, model)
    again.load_state_dict(back)                                            # and torch takes it
    assert_same_state_dict(again.state_dict(), sd)
    back["state"][5]["step"].fill_(9.0)                                    # copies: the optimizer's own state is untouched
    assert_same_state_dict(opt.state_dict(), sd)

    def refused(change):
        bad = copy.deepcopy(sd)
        change(bad)
        before = opt.state_dict()
        with pytest.raises(ValueError):
            opt.load_state_dict(bad)
        assert_same_state_dict(opt.state_dict(), before)

    refused(lambda s: s["param_groups"][0].update(weight_decay=0.1))
    refused(lambda s: s["param_groups"][0].update(maximize=True))
    refused(lambda s: s["param_groups"][0].update(lr=-1.0))
    if kind == "Adam":
        refused(lambda s: s["param_groups"][0].update(amsgrad=True))
    else:
        refused(lambda s: s["param_groups"][0].update(momentum=0.9))
        refused(lambda s: s["param_groups"][0].update(centered=True))
    refused(lambda s: s["state"][7]["step"].fill_(4.0))
    refused(lambda s: s["state"][2].update({("exp_avg_sq" if kind == "Adam" else "square_avg"): torch.zeros(5)}))
    refused(lambda s: s["state"].pop(3))
    other = torch_optimizer("RMSprop" if kind == "Adam" else "Adam", model)
    with pytest.raises(ValueError):
        opt.load_state_dict(other.state_dict())
    for kw in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)) if kind == "Adam" else dict(alpha=1.0)):
        with pytest.raises(ValueError):
            cpu_optimizer(kind, **kw)
    with pytest.raises(ValueError):
        cpu_optimizer("SGD")
    model.conv3.bias.grad = None
    with pytest.raises(ValueError, match="grad"):
        opt.step()
