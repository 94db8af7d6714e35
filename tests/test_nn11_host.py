"""The NN_11 forward without a GPU: the host side of toric-rl-decoder_amd/csrc/nn11.hpp -- the pack routine, the index
functions of the weight / activation / linear images and the tap -> source pixel map that the HIP kernels use -- built
with g++ through tests/host_nn11_shim.cpp and driven by a scalar forward under the numerics contract of
include/toricenv.h.  Test-only build: the product itself has no CPU path."""
import ctypes as C

import numpy as np
import pytest
import torch

import toric_rl_decoder_amd as T

import nn11_cases as K
from host_build import build_shim


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "host_nn11_shim.cpp", fast=True, openmp=True)
    lib.shim_nn11_forward.restype = C.c_int
    lib.shim_nn11_forward.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_int64,
                                      C.c_void_p]
    return lib


def shim_forward(shim, sd, d, per):
    w = [np.ascontiguousarray(sd[n + ".weight"].numpy(), np.float32) for n in K.NAMES]
    b = [np.ascontiguousarray(sd[n + ".bias"].numpy(), np.float32) for n in K.NAMES]
    wp = (C.c_void_p * 12)(*[a.ctypes.data for a in w])
    bp = (C.c_void_p * 12)(*[a.ctypes.data for a in b])
    per = np.ascontiguousarray(per, np.uint8)
    q = np.full((per.shape[0], 3), np.nan, np.float32)
    assert shim.shim_nn11_forward(d, wp, bp, per.ctypes.data, per.shape[0], q.ctypes.data) == 0
    return q


@pytest.mark.parametrize("d", K.SIZES)
def test_exact_integer_network_equals_torch_f32_bit_for_bit(shim, d):
    """Every activation is a small integer (asserted on torch's own f32 result), so bf16 storage and any summation
    order are exact: the shim's Q-table must be torch's.  Pins every tap, the three paddings, the odd channel counts
    and their zero padding, and the linear layer's feature order."""
    assert shim.shim_nn11_group(d) == max(1, 256 // (d * d))          # the G tests/test_gpu_nn11.py takes its row counts from
    sd = K.integer_state_dict(d)
    model = K.model_of(sd, d)
    per, _ = K.stack_of(d, 64)
    rows = per.shape[0]
    q_torch = np.empty((rows, 3), np.float32)
    seen, nonzero = set(), 0
    for i in range(0, rows, 256):
        outs, q = K.layer_outputs(model, torch.from_numpy(per[i:i + 256]).float())
        for a in outs:
            assert bool((a == a.round()).all()) and float(a.max()) < 256
        q_torch[i:i + 256] = q.numpy()
        last = outs[-1].flatten(1).to(torch.uint8).numpy()
        seen.update(hash(r.tobytes()) for r in last)
        nonzero += int(last.any(axis=1).sum())
    if d >= 5:
        assert len(seen) >= 0.99 * rows, (len(seen), rows)
    assert nonzero > 0
    got = shim_forward(shim, sd, d, per)
    assert np.array_equal(got, q_torch), (d, int((got != q_torch).any(axis=1).sum()), rows)


def test_the_references_three_roundings_on_the_ties():
    t = torch.tensor(K.TIES + tuple(-v for v in K.TIES), dtype=torch.float64)
    want = {"rne": (256, 260, 260, 264), "trunc": (256, 258, 260, 262), "half_up": (258, 260, 262, 264)}
    for mode, w in want.items():
        assert K.round_bf16(t, mode).tolist() == list(w) + [-v for v in w], mode
    exact = torch.tensor([0, 1, 2, 3, 255, 256, 258, 65536 + 512], dtype=torch.float64)
    for mode in want:
        assert torch.equal(K.round_bf16(exact, mode), exact)


DENSE_CASES = [(d, l) for d in K.SIZES for l in K.DENSE_LAYERS]


@pytest.mark.parametrize("d,dense_layer", DENSE_CASES)
def test_dense_exact_case_shim_f32_contract_and_f64_reference_agree_and_mutants_differ(shim, d, dense_layer):
    """The case tests/test_gpu_nn11.py holds the kernels to, at the same rows.  exact_dense_case asserts the exactness
    condition with its factor 2 of margin; under it the shim (the product's pack and index functions, f32 sums in its
    own order) and the f32 contract in torch ops must both give the f64 reference's bits.  The case must round, tell
    rows apart, and give another Q-table in at least a quarter of the rows under each of K.MUTANTS: a kernel wrong in
    that way cannot pass."""
    rows = K.dense_rows_for(d)
    sd, per, want, stats = K.exact_dense_case(d, dense_layer, rows)
    assert per.shape[0] == rows and per.dtype == np.uint8
    assert max(stats["conv_sum"], stats["linear_sum"]) < K.CASE_LIMIT
    changed = float(np.mean(stats["changed"][dense_layer - 1:]))        # share of the activations from the dense layer on
    assert changed > 0.002 and sum(stats["changed"]) > 0.02, stats["changed"]
    if d >= 5:
        assert stats["distinct_features"] >= 0.85, stats["distinct_features"]
    for l in range(1, 12):                                              # what the generator promises
        w = sd[f"conv{l}.weight"].flatten(1)
        nz = (w != 0).sum(1)
        if l == 1:
            assert int((w.abs() > 256).sum()) == 16 and bool((w.abs() > 256).any(1)[::8].all())
        elif l == dense_layer:
            assert bool((nz == w.shape[1]).all())
        else:
            assert bool((nz[:-1] == K.SPARSE_TAPS).all())
    x = torch.from_numpy(per)
    got = shim_forward(shim, sd, d, per)
    assert np.array_equal(got, want), (d, dense_layer, int((got != want).any(axis=1).sum()), rows)
    f32 = K.contract_forward(K.model_of(sd, d), x).numpy()
    assert np.array_equal(f32, want), (d, dense_layer, int((f32 != want).any(axis=1).sum()), rows)
    shares = {}
    for name, switches in K.MUTANTS.items():
        if K.mutant_is_void(name, d, dense_layer):
            continue
        q, _ = K.dense_reference(sd, x, dense_layer, **switches)
        shares[name] = float((q.numpy() != want.astype(np.float64)).any(axis=1).mean())
    print(f"dense d={d} layer {dense_layer}: {rows} rows, largest sum of magnitudes conv {stats['conv_sum']:.3g} linear "
          f"{stats['linear_sum']:.3g} of {K.EXACT_LIMIT:.3g}, narrowed {stats['narrowed']}, RNE changed {changed:.4f} of the "
          f"activations from the dense layer on, distinct feature rows {stats['distinct_features']:.2f}, smallest mutant "
          f"share {min(shares.values()):.2f} ({min(shares, key=shares.get)})")
    assert len(shares) >= len(K.MUTANTS) - 1
    assert min(shares.values()) >= 0.25, shares


@pytest.mark.parametrize("d,dense_layer", K.WIDE_CASES)
def test_wide_stack_cases_are_exact_and_see_the_stacks_rounding(shim, d, dense_layer):
    """The stacks of the GPU's conversion tests: elements beside 0 / 1, TIES among them.  The u8 one goes through the
    shim; on the f32 one the f32 contract gives the reference's bits, and a conversion that truncates or rounds half-up
    gives another Q-table in at least a quarter of the rows."""
    rows = K.dense_rows_for(d)
    sd, x8, want, stats = K.exact_dense_case(d, dense_layer, rows, K.U8_VALUES)
    assert set(np.unique(x8)) == {0, 1, 2, 255} and max(stats["conv_sum"], stats["linear_sum"]) < K.CASE_LIMIT
    assert np.array_equal(shim_forward(shim, sd, d, x8.astype(np.uint8)), want)
    assert np.array_equal(K.contract_forward(K.model_of(sd, d), torch.from_numpy(x8)).numpy(), want)
    sd, x, want, stats = K.exact_dense_case(d, dense_layer, rows, K.WIDE_VALUES)
    assert set(np.unique(x)) == {0, 1} | set(K.WIDE_VALUES) and max(stats["conv_sum"], stats["linear_sum"]) < K.CASE_LIMIT
    xt = torch.from_numpy(x)
    assert np.array_equal(K.contract_forward(K.model_of(sd, d), xt).numpy(), want)
    assert np.array_equal(K.contract_forward(K.model_of(sd, d), xt.bfloat16()).numpy(), want)
    assert np.array_equal(K.contract_forward(K.model_of(sd, d), xt.half()).numpy(), want)
    for mode in ("trunc", "half_up"):
        q, _ = K.dense_reference(sd, xt, dense_layer, stack_round=mode)
        share = float((q.numpy() != want.astype(np.float64)).any(axis=1).mean())
        print(f"wide stack d={d} layer {dense_layer}: sums conv {stats['conv_sum']:.3g} linear {stats['linear_sum']:.3g}, "
              f"stack rounded by {mode}: {share:.2f} of {rows} rows differ")
        assert share >= 0.25, (mode, share)


@pytest.mark.parametrize("d", (5, 7))
def test_trained_weights_stay_within_twice_the_contracts_own_rounding_error(shim, d):
    """rms error against torch's f32 forward <= 2 x that of the contract restated in torch ops (K.contract_forward): the
    shim sums in another order than torch, which flips single bf16 roundings -- noise of the roundings' own size; a wrong
    tap, bias or pad gives errors of the size of Q itself."""
    sd = K.trained_state_dict(d)
    model = K.model_of(sd, d)
    per, _ = K.stack_of(d, 256)
    x = torch.from_numpy(per).float()
    with torch.no_grad():
        q32 = torch.cat([model(x[i:i + 2048]) for i in range(0, x.shape[0], 2048)])
    yard = torch.cat([K.contract_forward(model, x[i:i + 2048]) for i in range(0, x.shape[0], 2048)])
    got = torch.from_numpy(shim_forward(shim, sd, d, per))
    e_yard, e_got = K.rms(yard, q32), K.rms(got, q32)
    print(f"d={d}: {x.shape[0]} perspectives, Q in [{float(q32.min()):.1f}, {float(q32.max()):.1f}], "
          f"rms error vs f32: yardstick {e_yard:.4f}, shim {e_got:.4f}")
    assert e_yard > 0
    assert e_got <= 2 * e_yard


def test_create_rejects_bad_arguments_before_the_device_is_touched():
    L = T.load()
    h = C.c_void_p(None)
    for d, max_rows in ((4, 64), (8, 64), (23, 64), (1, 64), (7, 0), (7, -5)):
        assert L.tq_nn11_create(C.byref(h), d, max_rows, 0) == -1, (d, max_rows)      # TQ_E_INVALID
        assert not h.value
    assert L.tq_nn11_create(None, 7, 64, 0) == -1
    assert L.tq_nn11_forward(None, None, 0, 0, None, None) == -1
    assert L.tq_nn11_load(None, None, None, None) == -1
    assert L.tq_nn11_destroy(None) == 0


def test_the_wrapper_is_public_and_skips_the_shape_padding():
    assert T.NN11Forward.any_rows is True and "NN11Forward" in T.__all__
    assert not hasattr(T.NN_11(5), "any_rows")
    from toric_rl_decoder_amd.policy import _forward_chunked

    class Rows:
        def __init__(self, any_rows):
            self.seen = []
            if any_rows:
                self.any_rows = True

        def __call__(self, x):
            self.seen.append(x.shape[0])
            return torch.zeros((x.shape[0], 3))

    x = torch.zeros((2500, 2, 3, 3))
    new, old = Rows(True), Rows(False)
    _forward_chunked(new, x, 2048)
    _forward_chunked(old, x, 2048)
    assert new.seen == [2048, 452] and old.seen == [2048, 1024]        # a torch module is padded as before
