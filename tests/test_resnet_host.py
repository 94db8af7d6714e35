"""The BasicBlock ResNets' forward (ResNet18, ResNet34) without a GPU: the host side of
toric-rl-decoder_amd/csrc/resnet.hpp -- the network table, the index functions of the weight images, the BatchNorm fold
and the pack routines that the HIP kernels use -- built with g++ through tests/host_resnet_shim.cpp; the yardsticks of
tests/resnet_cases.py against torch and against each other; and the Python surface as far as it goes without a device.
Test-only build: the product itself has no CPU path."""
import ctypes as C

import numpy as np
import pytest
import torch

import toric_rl_decoder_amd as T
from toric_rl_decoder_amd import resnet as R

import resnet_cases as K
from host_build import build_shim

FIELDS = ("cin", "cout", "taps", "stride", "role", "stage", "block", "half_in", "half_out", "img_taps", "ksteps", "ntiles", "chunks",
          "st_offset", "stack", "block_has_shortcut")
# (k-steps, n-tiles, taps, stride, reads the stack) of every kernel shape at the full grid, and the one at the half grid
FULL_SHAPES = {(2, 2, 9, 1, 1), (4, 2, 9, 1, 0), (4, 4, 9, 1, 0), (4, 4, 1, 1, 0), (8, 4, 9, 1, 0), (8, 8, 9, 1, 0), (8, 8, 1, 1, 0),
               (16, 8, 9, 1, 0), (16, 16, 9, 2, 0), (16, 16, 1, 2, 0)}
HALF_SHAPES = {(32, 16, 9, 1, 0)}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "host_resnet_shim.cpp", fast=True, openmp=True)
    i, i64, vp, f = C.c_int, C.c_int64, C.c_void_p, C.c_float
    for name, res, args in (("shim_resnet_slot", i, [i]), ("shim_resnet_convs", i, [i]), ("shim_resnet_conv", None, [i, i, vp]),
                            ("shim_resnet_wimg_offset", i64, [i, i]), ("shim_resnet_st_offset", i, [i, i]),
                            ("shim_resnet_wimg_elems", i64, [i, i, i]), ("shim_resnet_wimg_of", i64, [i, i, i, i, i]),
                            ("shim_resnet_wimg_coord", None, [i64, i, i, vp]), ("shim_resnet_src_pixel", i, [i, i, i, i, i, i]),
                            ("shim_resnet_half", i, [i]), ("shim_resnet_pack_conv", None, [i, i, i, vp, C.POINTER(vp), f, vp, vp, vp]),
                            ("shim_resnet_pack_linear", None, [vp, vp]),
                            ("shim_resnet_forward", i, [i, i, C.POINTER(vp), C.POINTER(vp), vp, vp, f, vp, i64, vp])):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def conv_of(shim, net, i):
    out = np.zeros(16, np.int32)
    shim.shim_resnet_conv(net, i, out.ctypes.data)
    return dict(zip(FIELDS, map(int, out)))


def bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def shim_forward(shim, sd, d, per, eps=K.EPS):
    net = K.net_of(sd)
    arr = lambda k: np.ascontiguousarray(sd[k].numpy(), np.float32)
    w = [arr(c + ".weight") for c, _, _ in K.convs(net)]
    bn = [arr(f"{b}.{k}") for _, b, _ in K.convs(net) for k in R.BN_KEYS]
    lw, lb = arr("linear.weight"), arr("linear.bias")
    wp = (C.c_void_p * len(w))(*[a.ctypes.data for a in w])
    bp = (C.c_void_p * len(bn))(*[a.ctypes.data for a in bn])
    per = np.ascontiguousarray(per, np.uint8)
    q = np.full((per.shape[0], 3), np.nan, np.float32)
    assert shim.shim_resnet_forward(net, d, wp, bp, lw.ctypes.data, lb.ctypes.data, eps, per.ctypes.data, per.shape[0], q.ctypes.data) == 0
    return q


def test_the_table_is_the_references_block_graph(shim):
    """Channel counts, block counts, which blocks have a shortcut convolution and the order of the convolutions: those of
    a module built from the reference's description (its state_dict key order), and the eleven kernel shapes are all the
    two nets need."""
    assert shim.shim_resnet_slot(18) == 0 and shim.shim_resnet_slot(34) == 1 and shim.shim_resnet_slot(50) == -1
    full, halfs = set(), set()
    for net, blocks in ((18, (2, 2, 2, 2)), (34, (3, 4, 6, 3))):
        model = K.MODULES[net]()
        keys = [k for k in model.state_dict().keys() if k.endswith(".weight") and model.state_dict()[k].dim() == 4]
        n = shim.shim_resnet_convs(net)
        assert n == len(keys) == len(K.convs(net)) == 1 + 2 * sum(blocks) + 3 == (20 if net == 18 else 36)
        assert [c + ".weight" for c, _, _ in K.convs(net)] == keys
        woff = soff = 0
        cuts = []
        for i, (name, bn, shape) in enumerate(K.convs(net)):
            y = conv_of(shim, net, i)
            assert (y["cout"], y["cin"], y["taps"]) == (shape[0], shape[1], shape[2] * shape[3]), name
            mod = model.get_submodule(name)
            assert mod.stride == (y["stride"],) * 2 and mod.padding == ((1, 1) if y["taps"] == 9 else (0, 0)) and mod.bias is None
            assert tuple(model.get_submodule(bn).weight.shape) == (y["cout"],)
            role = 0 if name == "conv1" else (3 if ".shortcut." in name else int(name[-1]))
            assert y["role"] == role
            if i:
                st, b = int(name[5]), int(name.split(".")[1])
                assert (y["stage"], y["block"]) == (st, b) and b < blocks[st - 1]
                assert y["cout"] == (64, 128, 256, 512)[st - 1]
                assert y["block_has_shortcut"] == (1 if len(model.get_submodule(f"layer{st}.{b}.shortcut")) else 0)
                assert y["stride"] == (2 if (st, b) == (4, 0) and role in (1, 3) else 1)
                assert y["half_in"] == (1 if st == 4 and not (b == 0 and role in (1, 3)) else 0) and y["half_out"] == (1 if st == 4 else 0)
                if role == 3:
                    cuts.append((st, b))
            assert y["stack"] == (1 if i == 0 else 0) and y["img_taps"] == (1 if i == 0 else y["taps"])
            assert y["ksteps"] == (2 if i == 0 else y["cin"] // 16) and y["ntiles"] == y["cout"] // 32
            assert y["chunks"] == -(-y["ksteps"] // 8) and y["ksteps"] % y["chunks"] == 0 and y["ksteps"] // y["chunks"] <= 8
            assert shim.shim_resnet_wimg_offset(net, i) == woff and y["st_offset"] == soff == shim.shim_resnet_st_offset(net, i)
            elems = shim.shim_resnet_wimg_elems(y["cin"], y["cout"], y["taps"])
            assert elems == y["img_taps"] * y["ksteps"] * y["ntiles"] * 512
            woff, soff = woff + elems, soff + y["ntiles"] * 32
            (halfs if y["half_in"] else full).add((y["ksteps"], y["ntiles"], y["taps"], y["stride"], y["stack"]))
        assert cuts == [(2, 0), (3, 0), (4, 0)]
        assert shim.shim_resnet_wimg_offset(net, n) == woff and shim.shim_resnet_st_offset(net, n) == soff
    assert full == FULL_SHAPES and halfs == HALF_SHAPES
    for d in K.SIZES:                                               # an image of the half grid fits the scratch of the full one
        assert shim.shim_resnet_half(d) == K.half(d) and 512 * K.half(d) ** 2 <= 256 * d * d


@pytest.mark.parametrize("ksteps,ntiles,taps", [(2, 2, 1), (4, 4, 1), (8, 8, 9), (16, 16, 9), (32, 16, 9)])
def test_image_index_and_coordinate_round_trip(shim, ksteps, ntiles, taps):
    n = taps * ksteps * ntiles * 512
    rng = np.random.default_rng(ksteps * 100 + ntiles)
    out = np.zeros(3, np.int32)
    for idx in np.concatenate([[0, 1, 7, 8, 511, 512, n - 1], rng.integers(0, n, 2000)]):
        shim.shim_resnet_wimg_coord(int(idx), ksteps, ntiles, out.ctypes.data)
        cout, k, tap = map(int, out)
        assert 0 <= cout < ntiles * 32 and 0 <= k < ksteps * 16 and 0 <= tap < taps
        assert shim.shim_resnet_wimg_of(cout, k, tap, ksteps, ntiles) == idx
        j, lane, f = idx & 7, (idx >> 3) & 63, idx >> 9
        assert (cout, k, tap) == (32 * (f % ntiles) + (lane & 31), 16 * (f // ntiles % ksteps) + 8 * (lane >> 5) + j, f // ntiles // ksteps)


@pytest.mark.parametrize("side", (2, 3, 4, 5, 6, 7, 10, 11, 21))
def test_source_pixels_of_both_strides_and_both_kernel_sizes(shim, side):
    s = (side + 1) // 2
    for y in range(side):
        for x in range(side):
            for tap in range(9):
                sy, sx = y + tap // 3 - 1, x + tap % 3 - 1
                want = sy * side + sx if 0 <= sy < side and 0 <= sx < side else -1
                assert shim.shim_resnet_src_pixel(side, 1, 9, y, x, tap) == want
            assert shim.shim_resnet_src_pixel(side, 1, 1, y, x, 0) == y * side + x          # the 1x1 reads the centre
    if side % 2:                                                    # stride 2 is taken from an odd grid only
        for y in range(s):
            for x in range(s):
                for tap in range(9):
                    sy, sx = 2 * y + tap // 3 - 1, 2 * x + tap % 3 - 1
                    want = sy * side + sx if 0 <= sy < side and 0 <= sx < side else -1
                    assert shim.shim_resnet_src_pixel(side, 2, 9, y, x, tap) == want
                assert shim.shim_resnet_src_pixel(side, 2, 1, y, x, 0) == 2 * y * side + 2 * x


@pytest.mark.parametrize("net,i", [(18, 0), (18, 1), (18, 7), (18, 12), (18, 15), (18, 17), (34, 35)])
def test_host_pack_and_fold_against_a_numpy_restatement(shim, net, i):
    y = conv_of(shim, net, i)
    cin, cout, ks, nt, taps, itaps = y["cin"], y["cout"], y["ksteps"], y["ntiles"], y["taps"], y["img_taps"]
    k = 3 if taps == 9 else 1
    rng = np.random.default_rng([net, i])
    w = rng.normal(size=(cout, cin, k, k)).astype(np.float32)
    w[w == 0] = 1.0                                             # every real element is non-zero: the padding alone is zero
    gamma, beta, mean = (rng.normal(size=cout).astype(np.float32) + o for o in (2.0, 0.0, 0.5))
    var = rng.uniform(0.5, 2.0, cout).astype(np.float32)
    eps = np.float32(1e-3)
    img = np.full(itaps * ks * nt * 512, 0xFFFF, np.uint16)
    scale, shift = np.full(nt * 32, np.nan, np.float32), np.full(nt * 32, np.nan, np.float32)
    bn = (C.c_void_p * 4)(*[a.ctypes.data for a in (gamma, beta, mean, var)])
    shim.shim_resnet_pack_conv(cin, cout, taps, w.ctypes.data, bn, eps, img.ctypes.data, scale.ctypes.data, shift.ctypes.data)
    # the fold, every f32 operation rounded once; zero in the padding
    s = gamma / np.sqrt(var + eps)
    assert s.dtype == np.float32
    assert np.array_equal(scale[:cout], s) and np.array_equal(shift[:cout], beta - mean * s)
    assert not scale[cout:].any() and not shift[cout:].any()
    # [tap][k][cout] padded, then gathered through the index function
    if i == 0:
        full = np.zeros((1, ks * 16, nt * 32), np.float32)
        full[0, :18, :cout] = w.reshape(cout, 18).T            # k = cin * 9 + tap
    else:
        full = np.zeros((taps, ks * 16, nt * 32), np.float32)
        full[:, :cin, :cout] = w.reshape(cout, cin, taps).transpose(2, 1, 0)
    want = bf16(full)
    got = (img.astype(np.uint32) << 16).view(np.float32)
    tap, kk, c = np.meshgrid(np.arange(full.shape[0]), np.arange(ks * 16), np.arange(nt * 32), indexing="ij")
    idx = ((((tap * ks + (kk >> 4)) * nt + (c >> 5)) * 64 + ((c & 31) | (((kk >> 3) & 1) << 5))) * 8 + (kk & 7))
    assert sorted(idx.ravel().tolist()) == list(range(img.size))        # a bijection onto the image
    assert np.array_equal(got[idx], want)
    assert int((got != 0).sum()) == cout * (18 if i == 0 else cin * taps)
    lw = rng.normal(size=(3, 512)).astype(np.float32)
    limg = np.full(3 * 512, np.nan, np.float32)
    shim.shim_resnet_pack_linear(lw.ctypes.data, limg.ctypes.data)
    assert np.array_equal(limg.reshape(3, 512), bf16(lw))


@pytest.mark.parametrize("net,d", [(18, 3), (18, 5), (18, 7), (18, 9), (18, 15), (34, 5)])
def test_integer_nets_f64_reference_shim_and_torch_f32_agree_in_bits(shim, net, d):
    """Every activation is an integer of at most 256 (asserted on the reference's own statistics), so bf16 storage and any
    summation order are exact: the float64 reference and the shim (the product's pack, fold and index functions) give one
    Q-table at every size, and torch's own f32 eval forward gives it where s^2 is a power of two (d = 3, 7, 15), where its
    mean over the pixels is exact as well."""
    sd = K.integer_state_dict(net, d)
    for _, bn, _ in K.convs(net):                               # the generator's promise about BatchNorm
        var = sd[bn + ".running_var"]
        assert bool((var + torch.tensor(K.EPS, dtype=torch.float32) == 1.0).all())
        assert set(sd[bn + ".weight"].tolist()) <= {0.5, 1.0, 2.0}
        assert all(bool((sd[f"{bn}.{k}"] == sd[f"{bn}.{k}"].round()).all()) for k in ("bias", "running_mean"))
    rows = K.dense_rows_for(d)
    per = K.dense_rows(d, rows)
    ref, stats = K.dense_reference(sd, torch.from_numpy(per))
    assert stats["max_act"] <= 256 and max(stats["conv_sum"], stats["linear_sum"]) < K.CASE_LIMIT
    assert stats["distinct_features"] == 1.0 and len({r.tobytes() for r in ref.numpy()}) == rows
    assert min(stats["changed"].values()) == max(stats["changed"].values()) == 0.0          # nothing is rounded
    assert list(stats["alive"].values())[-1] > 0.04
    gammas = torch.cat([sd[bn + ".weight"] for _, bn, _ in K.convs(net)])
    assert bool((gammas == 0.5).any()) and bool((gammas == 2).any())
    want = ref.float().numpy()
    assert np.array_equal(want.astype(np.float64), ref.numpy())
    if d in K.TORCH_EXACT_SIZES:
        with torch.no_grad():
            q = K.model_of(sd)(torch.from_numpy(per).float())
        assert np.array_equal(q.numpy(), want)
    got = shim_forward(shim, sd, d, per)
    assert np.array_equal(got, want), (net, d, int((got != want).any(axis=1).sum()))


def test_the_heads_order_of_sums_is_the_kernels(shim):
    """Where the head's sums round, their order shows: the shim's head (k_resnet_head's order: a lane's eight channels in
    order, then the butterfly) gives the bits of the numpy restatement of that order, which tests/test_gpu_resnet.py
    holds the kernel to, and a sum in plain channel order gives other bits."""
    sd, per, want, plain = K.head_order_case()
    got = shim_forward(shim, sd, 7, per)
    assert np.array_equal(got, want), int((got != want).any(axis=1).sum())
    assert (plain != want).any() and np.allclose(plain, want, rtol=1e-4, atol=1e-4)     # the case can tell the orders apart


@pytest.mark.parametrize("net,d,dense", K.CASES)
def test_dense_exact_cases_fit_agree_with_the_f32_contract_and_see_every_mutant(shim, net, d, dense):
    """The cases tests/test_gpu_resnet.py holds the kernels to, at the same rows.  exact_dense_case asserts the exactness
    condition with its factor 2 of margin; under it the f32 contract in torch ops (and, at the small sizes, the shim over
    the product's packed images) must give the float64 reference's bits.  The case must round from the dense convolution
    on, tell rows apart, keep part of the last image alive, and give another Q-table in bits under each of K.MUTANTS that
    is not void."""
    rows = K.dense_rows_for(d)
    sd, per, want, stats = K.exact_dense_case(net, d, dense, rows)
    assert per.shape[0] == rows and per.dtype == np.uint8
    assert max(stats["conv_sum"], stats["linear_sum"]) < K.CASE_LIMIT
    names = list(stats["changed"])
    changed = float(np.mean([stats["changed"][n] for n in names[names.index(dense):]]))
    assert changed > 0.001 and stats["max_act"] > 256, stats["changed"]
    assert stats["distinct_features"] == 1.0 and 0.03 < stats["alive"][names[-1]] < 0.3
    assert len({r.tobytes() for r in want}) == rows
    x = torch.from_numpy(per)
    f32 = K.contract_forward(K.model_of(sd), x).numpy()
    assert np.array_equal(f32, want), (net, d, dense, int((f32 != want).any(axis=1).sum()), rows)
    if d <= 7:
        got = shim_forward(shim, sd, d, per)
        assert np.array_equal(got, want), (net, d, dense, int((got != want).any(axis=1).sum()), rows)
    shares, void = {}, []
    for name, switches in K.MUTANTS.items():
        q, _ = K.dense_reference(sd, x, dense, **switches)
        if K.mutant_is_void(name, net, d, dense):               # an exemption checks itself: the mutant really cannot show
            assert np.array_equal(q.numpy(), want.astype(np.float64)), name
            void.append(name)
            continue
        shares[name] = float((q.numpy() != want.astype(np.float64)).any(axis=1).mean())
    print(f"dense ResNet{net} d={d} {dense}: {rows} rows, largest sum of magnitudes conv {stats['conv_sum']:.3g} linear "
          f"{stats['linear_sum']:.3g} of {K.EXACT_LIMIT:.3g}, narrowed {stats['narrowed']}, RNE changed {changed:.4f} of the "
          f"activations from the dense convolution on, alive in the last image {stats['alive'][names[-1]]:.3f}, mutant shares "
          f"{shares}, void {void}")
    assert len(shares) + len(void) == len(K.MUTANTS) == 16 and len(void) <= 1
    assert min(shares.values()) > 0, shares


def test_the_torch_modules_carry_the_references_names_and_load_strictly():
    for net, cls in ((18, T.ResNet18), (34, T.ResNet34)):
        m = cls()
        sd = m.state_dict()
        for key in ("conv1.weight", "bn1.running_var", "bn1.num_batches_tracked", "layer2.0.shortcut.0.weight",
                    "layer4.0.shortcut.1.running_mean", "layer1.1.bn2.bias", "linear.bias"):
            assert key in sd, key
        assert "layer1.0.shortcut.0.weight" not in sd and f"layer4.{2 if net == 18 else 3}.conv1.weight" not in sd
        assert {k for k in sd if not k.endswith("num_batches_tracked")} == set(R.shapes(net))
        assert all(tuple(sd[k].shape) == s for k, s in R.shapes(net).items())
        cls().load_state_dict(K.integer_state_dict(net, 5))     # strict: the names and shapes are the module's
        for d in (3, 5):
            assert tuple(m.eval()(torch.zeros(2, 2, d, d)).shape) == (2, 3)
    assert T.ResNet18(9, 3, "cpu").linear.out_features == 3     # the other nets' constructor arguments are accepted


def test_which_net_is_read_from_keys_and_shapes():
    assert R.which_net(K.integer_state_dict(18, 5)) == 18 and R.which_net(T.ResNet34().state_dict()) == 34
    sd = K.integer_state_dict(18, 5)
    assert R.which_net({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}) == 18
    for bad in ({k: v for k, v in sd.items() if k != "layer3.0.bn2.running_mean"}, {**sd, "layer1.2.conv1.weight": sd["layer1.1.conv1.weight"]},
                {**sd, "layer2.0.shortcut.0.weight": sd["layer2.0.shortcut.0.weight"][:, :-1]},
                {**sd, "linear.weight": sd["linear.weight"][:, :200]}, T.NN_11(5).state_dict(), T.NN_17(5).state_dict()):
        with pytest.raises(ValueError, match="neither"):
            R.which_net(bad)


def test_the_wrapper_is_public_and_fails_loudly_without_a_gpu():
    assert T.ResNetForward.any_rows is True and T.ResNetForward.gathers is False
    assert {"ResNet18", "ResNet34", "ResNetForward"} <= set(T.__all__)
    from toric_rl_decoder_amd import policy
    assert policy.ResNetForward is T.ResNetForward and policy.ResNet18 is T.ResNet18
    assert "eval-mode" in T.ResNetForward.__doc__.lower() and "not a training-mode forward" in T.ResNetForward.__doc__
    with pytest.raises(ValueError):
        T.ResNetForward(T.NN_11(5), 5, "cuda")                  # not a ResNet: refused before the device is asked for
    if not torch.cuda.is_available():
        with pytest.raises(T.ToricEnvError):
            T.ResNetForward(T.ResNet18(), 5, "cuda")
    with pytest.raises((ValueError, T.ToricEnvError)):
        T.ResNetForward(T.ResNet18(), 5, "cpu")


def test_create_rejects_bad_arguments_before_the_device_is_touched():
    L = T.load()
    h = C.c_void_p(None)
    for net, d, max_rows in ((11, 7, 64), (0, 7, 64), (50, 7, 64), (18, 4, 64), (34, 23, 64), (18, 7, 0), (34, 7, -5), (18, 7, (1 << 24) + 1)):
        assert L.tq_resnet_create(C.byref(h), net, d, max_rows, 0) == -1, (net, d, max_rows)     # TQ_E_INVALID
        assert not h.value
    assert L.tq_resnet_create(None, 18, 7, 64, 0) == -1
    assert L.tq_resnet_forward(None, None, 0, 0, None, None) == -1
    assert L.tq_resnet_load(None, None, None, None, None, 1e-5, None) == -1
    assert L.tq_resnet_destroy(None) == 0
