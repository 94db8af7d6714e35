"""The wide nets' forward (NN_8, NN_17) without a GPU: the host side of toric-rl-decoder_amd/csrc/nnw.hpp -- the network
table, the index functions of the weight / linear images and the pack routines that the HIP kernels use -- built with
g++ through tests/host_nnw_shim.cpp; the yardsticks of tests/nnw_cases.py against torch and against each other; and the
Python surface as far as it goes without a device.  Test-only build: the product itself has no CPU path."""
import ctypes as C

import numpy as np
import pytest
import torch

import toric_rl_decoder_amd as T

import nnw_cases as K
from host_build import build_shim

MODES = {0: "circular", 1: "zero", 2: "valid"}
FIVE_SHAPES = {(2, 8, "circular"), (16, 8, "zero"), (16, 7, "zero"), (14, 7, "zero"), (14, 7, "valid")}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "host_nnw_shim.cpp", fast=True, openmp=True)
    i, i64, vp = C.c_int, C.c_int64, C.c_void_p
    for name, res, args in (("shim_nnw_slot", i, [i]), ("shim_nnw_layers", i, [i]), ("shim_nnw_layer", None, [i, i, vp]),
                            ("shim_nnw_wimg_offset", i64, [i, i]), ("shim_nnw_bias_offset", i, [i, i]),
                            ("shim_nnw_wimg_elems", i64, [i, i]), ("shim_nnw_wimg_of", i64, [i, i, i, i, i]),
                            ("shim_nnw_wimg_coord", None, [i64, i, i, vp]), ("shim_nnw_lin_elems", i64, [i]),
                            ("shim_nnw_lin_index", i64, [i, i, i, i]), ("shim_nnw_pack_layer", None, [i, i, vp, vp, vp, vp]),
                            ("shim_nnw_pack_linear", None, [i, vp, vp]),
                            ("shim_nnw_forward", i, [i, i, C.POINTER(vp), C.POINTER(vp), vp, i64, vp])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def layer_of(shim, net, l):
    out = np.zeros(8, np.int32)
    shim.shim_nnw_layer(net, l, out.ctypes.data)
    return dict(zip(("cin", "cout", "mode", "taps", "ksteps", "ntiles", "bias_offset", "chunks"), map(int, out)))


def bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def shim_forward(shim, sd, d, per):
    net = K.net_of(sd)
    w = [np.ascontiguousarray(sd[n + ".weight"].numpy(), np.float32) for n in K.names(net)]
    b = [np.ascontiguousarray(sd[n + ".bias"].numpy(), np.float32) for n in K.names(net)]
    wp = (C.c_void_p * len(w))(*[a.ctypes.data for a in w])
    bp = (C.c_void_p * len(b))(*[a.ctypes.data for a in b])
    per = np.ascontiguousarray(per, np.uint8)
    q = np.full((per.shape[0], 3), np.nan, np.float32)
    assert shim.shim_nnw_forward(net, d, wp, bp, per.ctypes.data, per.shape[0], q.ctypes.data) == 0
    return q


def test_the_table_is_the_references_and_five_shapes_are_all_it_needs(shim):
    assert shim.shim_nnw_slot(8) == 0 and shim.shim_nnw_slot(17) == 1 and shim.shim_nnw_slot(11) == -1
    assert K.CH[8] == (2, 256, 256, 240, 224, 220, 215, 205, 200)
    assert K.CH[17] == (2, 256, 256, 251, 250, 240, 240, 235, 233, 233, 229, 225, 223, 220, 220, 220, 215, 214, 205, 204, 200)
    seen = set()
    for net in K.NETS:
        L = shim.shim_nnw_layers(net)
        assert L == K.layers(net) == (8 if net == 8 else 20)
        woff = boff = 0
        for l in range(1, L + 1):
            y = layer_of(shim, net, l)
            assert (y["cin"], y["cout"]) == (K.CH[net][l - 1], K.CH[net][l])
            assert y["mode"] == (0 if l == 1 else (2 if l == L else 1))
            assert y["taps"] == (1 if l == 1 else 9)
            assert y["ksteps"] == (2 if l == 1 else -(-y["cin"] // 32) * 2) and y["ntiles"] == -(-y["cout"] // 32)
            if l > 1:                                           # a layer reads the image its predecessor wrote
                assert y["ksteps"] * 16 == layer_of(shim, net, l - 1)["ntiles"] * 32
            assert y["chunks"] == (1 if l == 1 else 2) and y["ksteps"] % y["chunks"] == 0 and y["ksteps"] // y["chunks"] <= 8
            assert shim.shim_nnw_wimg_offset(net, l) == woff and y["bias_offset"] == boff == shim.shim_nnw_bias_offset(net, l)
            elems = shim.shim_nnw_wimg_elems(y["cin"], y["cout"])
            assert elems == y["taps"] * y["ksteps"] * y["ntiles"] * 512
            woff, boff = woff + elems, boff + y["ntiles"] * 32
            seen.add((y["ksteps"], y["ntiles"], MODES[y["mode"]]))
        assert shim.shim_nnw_wimg_offset(net, L + 1) == woff and shim.shim_nnw_bias_offset(net, L + 1) == boff
        assert layer_of(shim, net, L)["ntiles"] * 32 == 224    # the linear image's channel count
    assert seen == FIVE_SHAPES


@pytest.mark.parametrize("ksteps,ntiles,taps", [(2, 8, 1), (16, 8, 9), (16, 7, 9), (14, 7, 9)])
def test_image_index_and_coordinate_round_trip(shim, ksteps, ntiles, taps):
    n = taps * ksteps * ntiles * 512
    rng = np.random.default_rng(ksteps * 100 + ntiles)
    out = np.zeros(3, np.int32)
    for idx in np.concatenate([[0, 1, 7, 8, 511, 512, n - 1], rng.integers(0, n, 2000)]):
        shim.shim_nnw_wimg_coord(int(idx), ksteps, ntiles, out.ctypes.data)
        cout, k, tap = map(int, out)
        assert 0 <= cout < ntiles * 32 and 0 <= k < ksteps * 16 and 0 <= tap < taps
        assert shim.shim_nnw_wimg_of(cout, k, tap, ksteps, ntiles) == idx
        # the fragment order of nn11_wimg_index: lane l element j = W[32 ntile + (l & 31)][16 kstep + 8 (l >> 5) + j][tap]
        j, lane, f = idx & 7, (idx >> 3) & 63, idx >> 9
        assert (cout, k, tap) == (32 * (f % ntiles) + (lane & 31), 16 * (f // ntiles % ksteps) + 8 * (lane >> 5) + j, f // ntiles // ksteps)


@pytest.mark.parametrize("net,l", [(8, 1), (8, 3), (8, 4), (8, 8), (17, 4), (17, 12), (17, 19)])
def test_host_pack_of_a_layer_against_a_numpy_restatement(shim, net, l):
    y = layer_of(shim, net, l)
    cin, cout, ks, nt, taps = y["cin"], y["cout"], y["ksteps"], y["ntiles"], y["taps"]
    rng = np.random.default_rng([net, l])
    w = rng.normal(size=(cout, cin, 3, 3)).astype(np.float32)
    w[w == 0] = 1.0                                             # every real element is non-zero: the padding alone is zero
    b = (rng.normal(size=cout).astype(np.float32) + 3.0)
    img = np.full(taps * ks * nt * 512, 0xFFFF, np.uint16)
    bias = np.full(nt * 32, np.nan, np.float32)
    shim.shim_nnw_pack_layer(cin, cout, w.ctypes.data, b.ctypes.data, img.ctypes.data, bias.ctypes.data)
    assert np.array_equal(bias[:cout], b) and not bias[cout:].any()
    # [tap][k][cout] padded, then gathered through the index function
    if l == 1:
        full = np.zeros((1, ks * 16, nt * 32), np.float32)
        full[0, :18, :cout] = w.reshape(cout, 18).T            # k = cin * 9 + tap
    else:
        full = np.zeros((9, ks * 16, nt * 32), np.float32)
        full[:, :cin, :cout] = w.reshape(cout, cin, 9).transpose(2, 1, 0)
    want = bf16(full)
    got = (img.astype(np.uint32) << 16).view(np.float32)
    tap, k, c = np.meshgrid(np.arange(full.shape[0]), np.arange(ks * 16), np.arange(nt * 32), indexing="ij")
    idx = ((((tap * ks + (k >> 4)) * nt + (c >> 5)) * 64 + ((c & 31) | (((k >> 3) & 1) << 5))) * 8 + (k & 7))
    assert sorted(idx.ravel().tolist()) == list(range(img.size))        # a bijection onto the image
    assert np.array_equal(got[idx], want)
    assert int((got != 0).sum()) == cout * (18 if l == 1 else cin * 9)  # padding zero, nothing else
    for c_, k_, t_ in ((0, 0, 0), (cout - 1, (18 if l == 1 else cin) - 1, taps - 1)):
        assert got[shim.shim_nnw_wimg_of(c_, k_, t_, ks, nt)] == want[t_, k_, c_]


@pytest.mark.parametrize("d", (3, 5, 9))
def test_linear_image_feature_order(shim, d):
    npix = (d - 2) ** 2
    rng = np.random.default_rng(d)
    w = rng.normal(size=(3, 200 * npix)).astype(np.float32)
    assert shim.shim_nnw_lin_elems(d) == 3 * npix * 224
    limg = np.full(3 * npix * 224, np.nan, np.float32)
    shim.shim_nnw_pack_linear(d, w.ctypes.data, limg.ctypes.data)
    limg = limg.reshape(3, npix, 224)
    want = np.zeros((3, npix, 224), np.float32)
    want[:, :, :200] = bf16(w).reshape(3, 200, npix).transpose(0, 2, 1)     # torch flattens (channel, y, x)
    assert np.array_equal(limg, want)
    for a, p, c in ((0, 0, 0), (2, npix - 1, 199), (1, npix // 2, 223)):
        assert shim.shim_nnw_lin_index(a, p, c, npix) == (a * npix + p) * 224 + c


@pytest.mark.parametrize("net,d", [(8, 3), (8, 7), (17, 5), (17, 9)])
def test_integer_nets_dense_reference_shim_and_torch_f32_agree_in_bits(shim, net, d):
    """Every activation is a small integer (asserted on torch's own f32 result), so bf16 storage and any summation order
    are exact: the float64 reference, the shim (the product's pack and index functions) and torch's f32 forward give
    one Q-table."""
    sd = K.integer_state_dict(net, d)
    model = K.model_of(sd, d)
    per = K.dense_rows(d, 40)
    outs, q = K.layer_outputs(model, torch.from_numpy(per).float())
    for i, a in enumerate(outs):
        assert bool((a == a.round()).all()) and float(a.max()) <= i + 2
    assert bool(outs[-1].flatten(1).any(dim=1).float().mean() > 0.5)
    assert len({r.tobytes() for r in q.numpy()}) >= 0.9 * per.shape[0]
    ref, _ = K.dense_reference(sd, torch.from_numpy(per), 0)
    assert np.array_equal(ref.numpy(), q.numpy().astype(np.float64))
    got = shim_forward(shim, sd, d, per)
    assert np.array_equal(got, q.numpy()), (net, d, int((got != q.numpy()).any(axis=1).sum()))


@pytest.mark.parametrize("net,d,dense_layer", K.CASES)
def test_dense_exact_cases_fit_agree_with_the_f32_contract_and_see_every_mutant(shim, net, d, dense_layer):
    """The cases tests/test_gpu_nnw.py holds the kernels to, at the same rows.  exact_dense_case asserts the exactness
    condition with its factor 2 of margin; under it the f32 contract in torch ops (and, at the small sizes, the shim over
    the product's packed images) must give the float64 reference's bits.  The case must round, tell rows apart, keep
    part of the last layer alive, and give another Q-table in bits under each of K.MUTANTS that is not void."""
    rows = K.dense_rows_for(d)
    sd, per, want, stats = K.exact_dense_case(net, d, dense_layer, rows)
    assert per.shape[0] == rows and per.dtype == np.uint8
    assert max(stats["conv_sum"], stats["linear_sum"]) < K.CASE_LIMIT
    changed = float(np.mean(stats["changed"][dense_layer - 1:]))
    assert changed > 0.002 and sum(stats["changed"]) > 0.01, stats["changed"]
    assert stats["distinct_features"] == 1.0 and 0.05 < stats["alive"][-1] < 0.2
    x = torch.from_numpy(per)
    f32 = K.contract_forward(K.model_of(sd, d), x).numpy()
    assert np.array_equal(f32, want), (net, d, dense_layer, int((f32 != want).any(axis=1).sum()), rows)
    if d <= 7:
        got = shim_forward(shim, sd, d, per)
        assert np.array_equal(got, want), (net, d, dense_layer, int((got != want).any(axis=1).sum()), rows)
    shares, void = {}, []
    for name, switches in K.MUTANTS.items():
        if K.mutant_is_void(name, net, d, dense_layer):
            void.append(name + ": the dense layer has no zero padding to replace (the unpadded last conv, or d = 3)")
            continue
        q, _ = K.dense_reference(sd, x, dense_layer, **switches)
        shares[name] = float((q.numpy() != want.astype(np.float64)).any(axis=1).mean())
    print(f"dense net {net} d={d} layer {dense_layer}: {rows} rows, largest sum of magnitudes conv {stats['conv_sum']:.3g} linear "
          f"{stats['linear_sum']:.3g} of {K.EXACT_LIMIT:.3g}, narrowed {stats['narrowed']}, RNE changed {changed:.4f} of the "
          f"activations from the dense layer on, alive in the last layer {stats['alive'][-1]:.3f}, mutant shares {shares}, void {void}")
    assert len(shares) + len(void) == len(K.MUTANTS) and len(void) <= 1
    assert min(shares.values()) > 0, shares


def test_the_torch_modules_carry_the_references_parameter_names():
    for net, cls in ((8, T.NN_8), (17, T.NN_17)):
        m = cls(5)
        sd = m.state_dict()
        want = [f"conv{i + 1}.{k}" for i in range(K.layers(net)) for k in ("weight", "bias")] + ["linear1.weight", "linear1.bias"]
        assert list(sd.keys()) == want
        for i in range(K.layers(net)):
            c = getattr(m, f"conv{i + 1}")
            assert tuple(c.weight.shape) == (K.CH[net][i + 1], K.CH[net][i], 3, 3)
            assert c.padding == ((0, 0) if i in (0, K.layers(net) - 1) else (1, 1))
        assert tuple(m.linear1.weight.shape) == (3, 200 * 9)
        cls(5).load_state_dict(K.integer_state_dict(net, 5))    # strict: the names and shapes are the module's
        assert tuple(m(torch.zeros(2, 2, 5, 5)).shape) == (2, 3)


def test_which_net_is_read_from_keys_and_shapes():
    from toric_rl_decoder_amd import nnw
    assert nnw.which_net(K.integer_state_dict(8, 5), 5) == 8 and nnw.which_net(T.NN_17(7).state_dict(), 7) == 17
    sd = K.integer_state_dict(8, 5)
    for bad in ({k: v for k, v in sd.items() if k != "conv3.bias"}, {**sd, "conv9.weight": sd["conv8.weight"]},
                {**sd, "conv4.weight": sd["conv4.weight"][:, :-1]}, T.NN_11(5).state_dict()):
        with pytest.raises(ValueError, match="neither"):
            nnw.which_net(bad, 5)
    with pytest.raises(ValueError, match="linear1.weight"):
        nnw.which_net(sd, 7)                                    # another size's linear layer


def test_the_wrapper_is_public_and_fails_loudly_without_a_gpu():
    assert T.NNWideForward.any_rows is True and T.NNWideForward.gathers is False
    assert {"NN_8", "NN_17", "NNWideForward"} <= set(T.__all__)
    with pytest.raises(ValueError):
        T.NNWideForward(T.NN_11(5), 5, "cuda")                  # not a wide net: refused before the device is asked for
    if not torch.cuda.is_available():
        with pytest.raises(T.ToricEnvError):
            T.NNWideForward(T.NN_8(5), 5, "cuda")
    with pytest.raises((ValueError, T.ToricEnvError)):
        T.NNWideForward(T.NN_8(5), 5, "cpu")


def test_create_rejects_bad_arguments_before_the_device_is_touched():
    L = T.load()
    h = C.c_void_p(None)
    for net, d, max_rows in ((11, 7, 64), (0, 7, 64), (8, 4, 64), (17, 23, 64), (17, 7, 0), (8, 7, -5), (8, 7, (1 << 24) + 1)):
        assert L.tq_nnw_create(C.byref(h), net, d, max_rows, 0) == -1, (net, d, max_rows)       # TQ_E_INVALID
        assert not h.value
    assert L.tq_nnw_create(None, 8, 7, 64, 0) == -1
    assert L.tq_nnw_forward(None, None, 0, 0, None, None) == -1
    assert L.tq_nnw_load(None, None, None, None) == -1
    assert L.tq_nnw_destroy(None) == 0
