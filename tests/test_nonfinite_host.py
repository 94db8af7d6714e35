"""NaN and inf without a GPU: the contract of include/toricenv.h ("Non-finite values") on the host side of the headers the
HIP kernels share -- nn11_bf16 and the ReLU mask against torch, the scalar forwards of NN_11 and ResNet18 under a
poisoned weight against contract_forward, the TD target against the oracle's predict_max and the torch expression, the
greedy choice against np.argmax, and the optimizer's update and re-pack against the numpy contract.  NaNs are compared by
position, infs by sign, everything else bit for bit.  Test-only builds: the product itself has no CPU path."""
import ctypes as C

import numpy as np
import pytest
import torch

import nn11_cases as K
import nn11_opt_cases as OC
import plain_cases as P
import resnet_cases as RK
import select_plan_cases as S
from host_build import build_shim
from oracle import toric_oracle as O
from toric_rl_decoder_amd import resnet as R

F32 = np.float32
NAN, INF = F32(np.nan), F32(np.inf)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- bf16 and the mask ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nn11(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "host_nn11_shim.cpp", fast=True, openmp=True)
    lib.shim_nn11_forward.restype = C.c_int
    lib.shim_nn11_forward.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_int64, C.c_void_p]
    lib.shim_nn11_bf16.restype = lib.shim_nn11_mask.restype = None
    lib.shim_nn11_bf16.argtypes = lib.shim_nn11_mask.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    return lib


LOW_HALVES = (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff)


def test_bf16_is_torchs_on_every_high_half_and_a_nan_stays_a_nan(nn11):
    """All 65 536 high halves x LOW_HALVES: the halves around the tie, which decide the rounding, and around 0, which
    decide whether an inf's neighbour is a NaN.  Bits equal where torch's result is a number; a NaN where it is one."""
    hi = np.arange(1 << 16, dtype=np.uint32) << 16
    u = np.ascontiguousarray((hi[:, None] | np.array(LOW_HALVES, np.uint32)[None, :]).reshape(-1))
    x = u.view(F32)
    got = np.zeros(x.size, np.uint16)
    nn11.shim_nn11_bf16(ptr(x), x.size, ptr(got))
    want_t = torch.from_numpy(x.copy()).bfloat16()
    want = want_t.view(torch.int16).numpy().view(np.uint16)
    nan = torch.isnan(want_t).numpy()
    assert np.array_equal(nan, np.isnan(x)) and nan.sum() == 6 * 2 * 127 + 2 * 5
    got_nan = (got & 0x7fff) > 0x7f80
    assert np.array_equal(got_nan, nan), [hex(v) for v in u[got_nan != nan][:8]]
    assert np.array_equal(got[~nan], want[~nan]), [hex(v) for v in u[~nan][got[~nan] != want[~nan]][:8]]
    for word in (0x7fffffff, 0xffffffff, 0x7f800001):              # the carries that gave -0, +0 and +inf
        assert got_nan[np.flatnonzero(u == word)].all(), hex(word)
    assert got[u == 0x7f7f8000] == 0x7f80 and got[u == 0x7f7f7fff] == 0x7f7f      # the rounding boundary to inf, as before


def test_the_relu_mask_is_torchs_threshold_backward_on_every_bf16(nn11):
    a = np.arange(1 << 16, dtype=np.uint16)
    got = np.zeros(a.size, np.uint8)
    nn11.shim_nn11_mask(ptr(a), a.size, ptr(got))
    x = torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16).float().requires_grad_()
    torch.relu(x).backward(torch.ones_like(x))
    want = x.grad.numpy()
    assert int(np.isnan(x.detach().numpy()).sum()) == 2 * 127 and want[np.isnan(x.detach().numpy())].all()
    assert np.array_equal(got, want.astype(np.uint8))


# ---- the scalar forwards under a poisoned weight --------------------------------------------------------------------
def nn11_forward(lib, sd, d, per):
    w = [np.ascontiguousarray(sd[n + ".weight"].numpy(), F32) for n in K.NAMES]
    b = [np.ascontiguousarray(sd[n + ".bias"].numpy(), F32) for n in K.NAMES]
    wp = (C.c_void_p * 12)(*[a.ctypes.data for a in w])
    bp = (C.c_void_p * 12)(*[a.ctypes.data for a in b])
    per = np.ascontiguousarray(per, np.uint8)
    q = np.full((per.shape[0], 3), 7.0, F32)
    assert lib.shim_nn11_forward(d, wp, bp, ptr(per), per.shape[0], ptr(q)) == 0
    return q


@pytest.mark.parametrize("layer", (2, 11))
@pytest.mark.parametrize("kind", P.WEIGHT_POISONS)
def test_nn11_host_forward_sends_a_poisoned_weight_where_torch_does(nn11, kind, layer):
    """d = 3, He weights.  Layer 2: the poison passes nine ReLUs, bf16 roundings and the zero padding (0 x inf there is a
    NaN in torch).  Layer 11, the unpadded last one: under the inf weight the feature is +inf where the activation it
    meets is positive and a NaN where it is 0, so that rows differ and Q holds infs of both signs."""
    d = 3
    per = K.dense_rows(d, K.dense_rows_for(d))
    sd = P.poisoned_state_dict(P.he_state_dict(K.NET, d), f"conv{layer}.weight", f"conv{layer}.bias", kind, at=(5 * K.CH[layer - 1] + 3) * 9 + 4, bias_at=5)
    want = P.order_free_pattern(K.contract_forward, K.model_of(sd, d), torch.from_numpy(per)).numpy()
    got = nn11_forward(nn11, sd, d, per)
    assert P.same_pattern(got, want), (kind, layer, P.pattern(got).tolist(), P.pattern(want).tolist())
    if layer == 11 and kind == "inf weight":
        assert {P.NAN, P.PLUS_INF, P.MINUS_INF} <= set(P.pattern(want).reshape(-1).tolist())


@pytest.fixture(scope="module")
def resnet(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "host_resnet_shim.cpp", fast=True, openmp=True)
    i, i64, vp = C.c_int, C.c_int64, C.c_void_p
    lib.shim_resnet_forward.restype = i
    lib.shim_resnet_forward.argtypes = [i, i, C.POINTER(vp), C.POINTER(vp), vp, vp, C.c_float, vp, i64, vp]
    return lib


def resnet_forward(lib, sd, d, per, eps=RK.EPS):
    net = RK.net_of(sd)
    arr = lambda k: np.ascontiguousarray(sd[k].numpy(), F32)
    w = [arr(c + ".weight") for c, _, _ in RK.convs(net)]
    bn = [arr(f"{b}.{k}") for _, b, _ in RK.convs(net) for k in R.BN_KEYS]
    lw, lb = arr("linear.weight"), arr("linear.bias")
    wp = (C.c_void_p * len(w))(*[a.ctypes.data for a in w])
    bp = (C.c_void_p * len(bn))(*[a.ctypes.data for a in bn])
    per = np.ascontiguousarray(per, np.uint8)
    q = np.full((per.shape[0], 3), 7.0, F32)
    assert lib.shim_resnet_forward(net, d, wp, bp, ptr(lw), ptr(lb), eps, ptr(per), per.shape[0], ptr(q)) == 0
    return q


RESNET_POISONS = P.WEIGHT_POISONS + ("nan batchnorm weight",)


def resnet_poisoned(sd, conv, kind):
    """``conv`` of RK.convs(net) by name: its weight, or its BatchNorm's beta (the "bias") or gamma"""
    bn = {c: b for c, b, _ in RK.convs(RK.net_of(sd))}[conv]
    if kind == "nan batchnorm weight":
        return P.poisoned_state_dict(sd, conv + ".weight", bn + ".weight", "nan bias", bias_at=5)
    cin = sd[conv + ".weight"].shape[1]
    taps = sd[conv + ".weight"].shape[2] * sd[conv + ".weight"].shape[3]
    return P.poisoned_state_dict(sd, conv + ".weight", bn + ".bias", kind, at=(5 * cin + 3) * taps + taps // 2, bias_at=5)


@pytest.mark.parametrize("conv", ("layer2.0.conv1", "layer2.0.shortcut.0", "layer4.1.conv2"))
@pytest.mark.parametrize("kind", RESNET_POISONS)
def test_resnet_host_forward_sends_a_poisoned_weight_where_torch_does(resnet, kind, conv):
    """ResNet18 at d = 3: a convolution in the middle, a 1x1 shortcut (its image is rounded, added and only then meets a
    ReLU) and the last convolution, whose output goes through the residual sum and the pool alone."""
    d = 3
    per = K.dense_rows(d, K.dense_rows_for(d))
    sd = resnet_poisoned(RK.he_state_dict(18), conv, kind)
    want = P.order_free_pattern(RK.contract_forward, RK.model_of(sd), torch.from_numpy(per)).numpy()
    got = resnet_forward(resnet, sd, d, per)
    assert P.same_pattern(got, want), (kind, conv, P.pattern(got).tolist(), P.pattern(want).tolist())


# ---- the TD target --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def td(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "host_td_target_shim.cpp")
    lib.shim_td_target.restype = None
    lib.shim_td_target.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_void_p]
    return lib


def td_slices(d=5):
    """States whose slices cover the issue's list -> (states, q (P,3), off, what: slice -> description).  Slice 0 is the
    longest (every qubit a hit) and slice 1 as long; the others are shorter and so zero-padded by the reference."""
    rng = np.random.default_rng(77)
    n = 14
    _, st = O.reset_lattices(9, np.arange(n), 0, 0.12, d)
    st[0] = st[1] = st[12] = 1
    st[13] = 0                                                      # no perspective at all
    _, _, cnt, off = O.generate_perspective_batch(st)
    assert cnt[0] == cnt[1] == cnt[12] == cnt.max() and cnt[13] == 0 and (cnt[2:12] > 1).all() and (cnt[2:12] < cnt.max()).all()
    q = (-np.abs(rng.normal(size=(int(off[-1]), 3))) * 20 - 1).astype(F32)         # negative: the zero padding decides
    q[off[11]:off[12]] *= -1                                                     # ... and one positive slice
    sl = lambda i: q[off[i]:off[i + 1]].reshape(-1)                              # a view
    what = {}
    sl(0)[sl(0).size // 2], what[0] = NAN, "longest, NaN in the middle"
    sl(1)[:], what[1] = -INF, "longest, all -inf"
    sl(2)[0], what[2] = NAN, "NaN first"
    sl(3)[sl(3).size // 2], what[3] = NAN, "NaN in the middle"
    sl(4)[-1], what[4] = NAN, "NaN last"
    sl(5)[:], what[5] = NAN, "all NaN"
    sl(6)[:], what[6] = -INF, "shorter, all -inf: the padding's 0"
    sl(7)[1], what[7] = INF, "+inf"
    sl(8)[2], sl(8)[0], what[8] = NAN, INF, "+inf before a NaN"
    sl(9)[1], what[9] = NAN, "terminal flag, cnt > 0, a NaN"
    sl(10)[1], what[10] = INF, "terminal flag, cnt > 0, +inf"
    what[11], what[12], what[13] = "finite", "longest, finite, terminal flag", "no perspectives"
    return st, q, off, cnt, what


def td_case():
    st, q, off, cnt, what = td_slices()
    r = np.linspace(-2, 2, len(cnt)).astype(F32)
    t = np.zeros(len(cnt), np.uint8)
    t[[9, 10, 12, 13]] = 1

    def q_fn(per):                                                  # predict_max gives a state without perspectives one dummy row
        rows = np.insert(q, np.repeat(off[1:][cnt == 0], 1), F32(5), axis=0)
        assert rows.shape[0] == per.shape[0]
        return rows

    with np.errstate(invalid="ignore"):
        m = O.predict_max(q_fn, st)
    y = (torch.from_numpy(r) + (~torch.from_numpy(t.astype(bool))).float() * 0.95 * torch.from_numpy(m)).clamp(-100, 100).numpy()
    return q, off, r, t, m, y, what


def test_td_case_is_what_the_issue_lists():
    q, off, r, t, m, y, what = td_case()
    want = {0: P.NAN, 1: P.FINITE, 2: P.NAN, 3: P.NAN, 4: P.NAN, 5: P.NAN, 6: P.FINITE, 7: P.FINITE, 8: P.NAN, 9: P.NAN, 10: P.NAN,
            11: P.FINITE, 12: P.FINITE, 13: P.FINITE}
    assert P.pattern(y).tolist() == [want[i] for i in range(len(want))], (P.pattern(y).tolist(), what)
    assert np.isneginf(m[1]) and y[1] == -100 and m[6] == 0 and y[6] == r[6] and np.isposinf(m[7]) and y[7] == 100
    assert m[13] == 0 and y[13] == r[13] and y[12] == r[12]


def test_compiled_td_function_keeps_nan_like_predict_max_and_the_torch_expression(td):
    q, off, r, t, m, want, what = td_case()
    got = np.full(len(r), F32(7))
    td.shim_td_target(ptr(q), ptr(off), len(r), ptr(r), ptr(t), 0.95, -100.0, 100.0, ptr(got))
    assert P.same_bits_nan_equal(got, want), [(what[i], got[i], want[i]) for i in range(len(r)) if not P.same_bits_nan_equal(got[i:i + 1], want[i:i + 1])]


# ---- the greedy choice ----------------------------------------------------------------------------------------------
def test_host_greedy_choice_is_np_argmax_with_nan(tmp_path_factory):
    lib = S.load_shim(tmp_path_factory)
    q, off = S.nonfinite_slices()
    n = off.size - 1
    pos = np.arange(3 * q.shape[0], dtype=np.int32).reshape(-1, 3) % 17
    pos[:, 0] = np.arange(q.shape[0]) - np.repeat(off[:-1], np.diff(off))       # the row within the slice: the choice shows
    ep, st = np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32)
    want_act, want_qv, chosen = O.select_action_batch(q, off, pos, 0.0, 5, np.arange(n), ep, st)
    flat = [int(np.argmax(q[off[i]:off[i + 1]].reshape(-1))) for i in range(n)]
    assert [(int(c - off[i]), int(a[3]) - 1) for i, (c, a) in enumerate(zip(chosen, want_act))] == [divmod(f, 3) for f in flat]
    nan_first = [int(np.flatnonzero(np.isnan(q[off[i]:off[i + 1]].reshape(-1)))[0]) for i in range(n) if np.isnan(q[off[i]:off[i + 1]]).any()]
    assert nan_first == [f for i, f in enumerate(flat) if np.isnan(q[off[i]:off[i + 1]]).any()] and len(nan_first) > 20
    act, qv, bad = S.host_select_planned(lib, q, off, off, pos, 0.0, ep, st, 5)
    assert bad == 0
    assert np.array_equal(act, want_act), np.flatnonzero((act != want_act).any(axis=1))
    assert P.same_bits_nan_equal(qv, want_qv)


def test_the_oracles_c_restatement_takes_the_first_nan_like_the_numpy_one():
    from oracle.c_oracle import CEnvBatch
    q, off = S.nonfinite_slices()
    n = off.size - 1
    row = (np.arange(q.shape[0]) - np.repeat(off[:-1], np.diff(off))).astype(np.int32)
    pos = np.ascontiguousarray(np.stack([row % 2, row // 2 % 5, row // 10], axis=1))
    ce = CEnvBatch(5, n, seed=5)
    want_act, want_qv, _ = O.select_action_batch(q, off, pos, 0.0, 5, np.arange(n), ce.episodes, ce.steps)
    act, qv = ce.select(q, off, pos, 0.0)
    assert np.array_equal(act, want_act) and P.same_bits_nan_equal(qv, want_qv)


# ---- the optimizer --------------------------------------------------------------------------------------------------
KIND_ID = {"Adam": 0, "RMSprop": 1}
H = OC.HYPER
HYPER_ARGS = (H["lr"], H["betas"][0], H["betas"][1], H["eps"], H["alpha"])


@pytest.fixture(scope="module")
def opt(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "host_nn11_opt_shim.cpp", fast=True)
    vp, dbl = C.c_void_p, C.c_double
    hyper = [C.c_int, dbl, dbl, dbl, dbl, dbl, C.c_int64]
    lib.shim_nn11_opt_update.restype = None
    lib.shim_nn11_opt_update.argtypes = hyper + [C.c_int64, vp, vp, vp, vp]
    lib.shim_nn11_opt_sizes.restype = None
    lib.shim_nn11_opt_sizes.argtypes = [C.c_int, C.c_int, vp]
    lib.shim_nn11_opt_images.restype = None
    lib.shim_nn11_opt_images.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]
    return lib


def poisoned_gradient(g, seed):
    """NaN, +inf and -inf at three random places each (one each in the linear layer's bias of three elements)"""
    k = min(3, g.size // 3)
    at = np.random.default_rng(seed).choice(g.size, 3 * k, replace=False)
    g = g.copy()
    g.reshape(-1)[at] = np.repeat([NAN, INF, -INF], k)
    return g


def bf16_nan_equal(a, b):
    a, b = np.asarray(a, np.uint16), np.asarray(b, np.uint16)
    na, nb = (a & 0x7fff) > 0x7f80, (b & 0x7fff) > 0x7f80
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])


@pytest.mark.parametrize("kind", OC.KINDS)
def test_optimizer_update_and_repack_propagate_nan_and_inf(opt, kind):
    """One step at d = 3 on every tensor of the model case with NaN, +inf and -inf gradient elements: p', m', v' as the
    numpy contract gives them (an inf gradient makes v' inf and the quotient a NaN, as IEEE has it), and the four images
    scattered from the updated masters equal the host pack of the same masters."""
    d, t = 3, 2
    c = OC.consts(kind, t)
    case = OC.model_case(d, kind, t)
    new = {}
    for i, (name, tc) in enumerate(case.items()):
        g = poisoned_gradient(tc["g"], i)
        want = OC.update(kind, c, tc["p"], g, tc["m"], tc["v"])
        p, v = tc["p"].copy(), tc["v"].copy()
        m = None if tc["m"] is None else tc["m"].copy()
        opt.shim_nn11_opt_update(KIND_ID[kind], *HYPER_ARGS, t, p.size, ptr(p), ptr(np.ascontiguousarray(g)), None if m is None else ptr(m), ptr(v))
        for a, w, what in zip((p, m, v), want, "pmv"):
            assert (a is None and w is None) or P.same_bits_nan_equal(a, w), (name, what)
        k = int(np.isnan(g).sum())
        assert k in (1, 3) and np.isnan(p).sum() == 3 * k and np.isposinf(v).sum() == 2 * k, name     # nothing is clamped or skipped
        new[name] = p
    assert set(new) == set(OC.shapes(d))
    for l, name in enumerate(OC.NAMES, start=1):
        w, b = new[name + ".weight"], new[name + ".bias"]
        sizes = np.zeros(4, np.int64)
        opt.shim_nn11_opt_sizes(l, d, ptr(sizes))
        made = []
        for which in (0, 1):
            wimg, dimg = np.zeros(max(1, sizes[0]), np.uint16), np.zeros(max(1, sizes[1]), np.uint16)
            bias, limg = np.zeros(sizes[2], F32), np.zeros(max(1, sizes[3]), F32)
            opt.shim_nn11_opt_images(which, l, d, ptr(w), ptr(b), ptr(wimg), ptr(dimg), ptr(bias), ptr(limg))
            made.append((wimg, dimg, bias, limg))
        assert bf16_nan_equal(made[0][0], made[1][0]) and bf16_nan_equal(made[0][1], made[1][1]), name
        assert P.same_bits_nan_equal(made[0][2], made[1][2]) and P.same_bits_nan_equal(made[0][3], made[1][3]), name
        img = made[0][0] if l <= 11 else made[0][3].view(np.uint32) >> 16
        assert int(((np.asarray(img) & 0x7fff) > 0x7f80).sum()) == 9 == int(np.isnan(w).sum()), name      # each NaN master is a NaN in the image
