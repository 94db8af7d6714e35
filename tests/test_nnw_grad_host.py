"""The wide nets' learner step without a GPU: the host side of toric-rl-decoder_amd/csrc/nnw.hpp and nnw_grad.hpp -- the
forward and dgrad pack routines, the index functions, the chunk arithmetic -- built with g++ through
tests/host_nnw_grad_shim.cpp and driven by a scalar forward + backward under the numerics contract of
include/toricenv.h, against the two cases of tests/nnw_grad_cases.py.  Test-only build: the product has no CPU path."""
import ctypes as C

import numpy as np
import pytest
import torch

import toric_rl_decoder_amd as T

import nnw_cases as K
import nnw_grad_cases as GC
from host_build import build_shim

CASES = ((8, 3), (8, 5), (17, 5))                          # (net, d) of the scalar backward
ROUNDING = ((8, 3), (8, 5), (8, 7), (17, 5))               # (net, d) of the GPU tests' rounding case


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "host_nnw_grad_shim.cpp", fast=True, openmp=True)
    vp = C.c_void_p
    lib.shim_nnw_grad.restype = C.c_int
    lib.shim_nnw_grad.argtypes = [C.c_int, C.c_int, C.POINTER(vp), C.POINTER(vp), vp, C.c_int, vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(vp)]
    lib.shim_nnw_dgrad_image.restype = C.c_int64
    lib.shim_nnw_dgrad_image.argtypes = [C.c_int, C.c_int, vp, vp]
    lib.shim_nnw_dimg_of.restype = C.c_int64
    lib.shim_nnw_dimg_offset.restype = C.c_int64
    lib.shim_nnw_wgrad_chunks.restype = C.c_int64
    lib.shim_nnw_wgrad_chunks.argtypes = [C.c_int, C.c_int64]
    lib.shim_nnw_wpart_elems.restype = C.c_int64
    return lib


def shim_step(shim, c, rows, wv):
    net, d, sd = c["net"], c["d"], c["sd"]
    names = K.names(net)
    wts = [np.ascontiguousarray(sd[n + ".weight"].numpy(), np.float32) for n in names]
    bs = [np.ascontiguousarray(sd[n + ".bias"].numpy(), np.float32) for n in names]
    gw, gb = [np.full_like(a, np.nan) for a in wts], [np.full_like(a, np.nan) for a in bs]
    ptrs = lambda arrs: (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    x = np.ascontiguousarray(c["x"][:rows], np.uint8)
    a, y = c["actions"][:rows].numpy().copy(), c["y"][:rows].numpy().copy()
    wv = wv.numpy().copy()
    q, loss = np.full((rows, 3), np.nan, np.float32), np.full(rows, np.nan, np.float32)
    assert shim.shim_nnw_grad(net, d, ptrs(wts), ptrs(bs), x.ctypes.data, rows, a.ctypes.data, y.ctypes.data, wv.ctypes.data,
                              q.ctypes.data, loss.ctypes.data, ptrs(gw), ptrs(gb)) == 0
    grads = {}
    for n, w_, b_ in zip(names, gw, gb):
        grads[n + ".weight"], grads[n + ".bias"] = w_, b_
    return q, loss, grads


@pytest.mark.parametrize("net,d", CASES)
def test_both_cases_equal_their_references_bit_for_bit(shim, net, d):
    """The scalar host backward over the headers' images at the GPU tests' row counts.  Case 1 (asserted by
    GC.integer_case: nothing rounds, torch's own f32 autograd is the reference, every gradient tensor is non-zero);
    case 2 (GC.rounding_case: G rounds in at least two layers, ties included, every sum exact, float64 autograd is the
    reference)."""
    counts = GC.row_counts(d)
    for c in (GC.integer_case(net, d), GC.rounding_case(net, d)):
        for rows in (counts[-1], counts[1]):
            w, want_loss, want = GC.at_rows(c, rows)
            q, loss, grads = shim_step(shim, c, rows, w)
            assert np.array_equal(q, c["q"][:rows]) and np.array_equal(loss, want_loss)
            for k in GC.params(net):
                assert np.array_equal(grads[k], want[k]), (net, d, rows, k, int((grads[k] != want[k]).sum()))


@pytest.mark.parametrize("net,d", ROUNDING)
def test_every_mutant_changes_some_gradient_tensor_in_bits(net, d):
    """For every (net, d) of the GPU tests' rounding case: each of the seven mutants of nn11_grad_cases.MUTANTS, the
    one-layer ones at the middle of the net, differs from the reference in some gradient tensor; at most one may be
    void, and only one that GC.mutant_is_void names."""
    c = GC.rounding_case(net, d)
    rows = GC.row_counts(d)[-1]
    want = GC.at_rows(c, rows)[2]
    seen = {}
    for name in GC.MUTANTS:
        m = GC.mutant_grads(c, name)
        changed = [k for k in GC.params(net) if not np.array_equal(m[k].float().numpy(), want[k])]
        if GC.mutant_is_void(name, net, d):
            assert not changed, (net, d, name, "named void, yet it changes a gradient")
            continue
        seen[name] = changed
        assert changed, (net, d, name)
    st = c["stats"]
    print(f"nnw grad cases net={net} d={d}: {rows} records, largest sum of magnitudes {st['sum_max']:.3g} of {GC.SUM_LIMIT:.3g}, largest "
          f"|G| {st['g_max']:.0f}, RNE changed {', '.join(f'G{l}: {v:.4f}' for l, v in st['changed'].items() if v > 0)}; tensors changed by "
          f"each mutant: {', '.join(f'{k}: {len(v)}' for k, v in seen.items())}")
    assert st["sum_max"] < GC.SUM_LIMIT and len(GC.rounded_layers(c)) >= 2
    assert len(seen) >= len(GC.MUTANTS) - 1


@pytest.mark.parametrize("net", K.NETS)
def test_the_dgrad_image_element_by_element(shim, net):
    """element (ci, co, tap') of every layer's image, found through the header's fragment index, is
    bf16(W[co][ci][8 - tap']); everything else in the image is the zero padding; the images lie back to back; and the
    (k-steps, n-tiles) of the dgrads are the four shapes the library holds."""
    rng = np.random.default_rng(5 + net)
    ch, L = K.CH[net], K.layers(net)
    cp = lambda c: (c + 31) // 32 * 32
    offset, shapes = 0, set()
    for l in range(2, L + 1):
        cin, cout = ch[l - 1], ch[l]
        w = rng.normal(size=(cout, cin, 3, 3)).astype(np.float32)
        n = shim.shim_nnw_dgrad_image(cin, cout, None, None)
        assert n == 9 * cp(cout) * cp(cin) and shim.shim_nnw_dimg_offset(net, l) == offset
        offset += n
        img = np.full(n, 0xFFFF, np.uint16)
        shim.shim_nnw_dgrad_image(cin, cout, w.ctypes.data, img.ctypes.data)
        want = torch.from_numpy(w).bfloat16().view(torch.int16).numpy().view(np.uint16)
        cos = sorted(set(range(0, cout, 37)) | {cout - 1})
        idx = np.array([[[shim.shim_nnw_dimg_of(cin, cout, ci, co, t) for t in range(9)] for ci in range(cin)] for co in cos])
        assert np.array_equal(img[idx], want[cos].reshape(len(cos), cin, 9)[:, :, ::-1]), l
        assert len(set(idx.ravel().tolist())) == idx.size and 0 <= idx.min() and idx.max() < n
        assert int((img != 0).sum()) == int((want != 0).sum()), l           # what is not a weight is the zero padding
        out = (C.c_int * 2)()
        shim.shim_nnw_dgrad_shape(net, l, out)
        assert (out[0], out[1]) == (cp(cout) // 16, cp(cin) // 32)
        shapes.add((out[0], out[1], l == L))
    assert shim.shim_nnw_dimg_offset(net, L + 1) == offset
    assert shapes == {(16, 8, False), (14, 8, False), (14, 7, False), (14, 7, True)}


def test_the_chunk_arithmetic(shim):
    """nnw_wgrad_persp is a function of d alone, about 2048 rows and never fewer than two records; the chunks of n
    records; a partial image holds the widest layer; and the scratch the header states for max_batch = 4096 at d = 21."""
    lib = shim
    for d in K.SIZES:
        p = lib.shim_nnw_wgrad_persp(d)
        assert p == GC.wgrad_persp(d) == max(2, 2048 // (d * d))
        assert p >= 2 and (p == 2 or (p * d * d <= 2048 < (p + 1) * d * d))
        for n in (1, p - 1, p, p + 1, 2 * p, 2 * p + 1, 4096):
            assert lib.shim_nnw_wgrad_chunks(d, n) == -(-n // p)
        for net in K.NETS:
            L = K.layers(net)
            assert [lib.shim_nnw_layer_pixels(net, l, d) for l in (1, L - 1, L)] == [d * d, d * d, (d - 2) ** 2]
    assert lib.shim_nnw_wpart_elems() == 9 * 256 * 256
    assert lib.shim_nnw_wgrad_persp(21) == 4 and lib.shim_nnw_wgrad_chunks(21, 4096) * lib.shim_nnw_wpart_elems() * 4 == 2304 << 20


def test_create_rejects_bad_arguments_before_the_device_is_touched():
    L = T.load()
    h = C.c_void_p(None)
    for net, d, max_batch in ((11, 7, 64), (0, 7, 64), (18, 7, 64), (8, 4, 64), (8, 23, 64), (17, 1, 64), (8, 7, 0), (8, 7, -5),
                              (17, 7, 4097)):
        assert L.tq_nnw_grad_create(C.byref(h), net, d, max_batch, 0) == -1, (net, d, max_batch)      # TQ_E_INVALID
        assert not h.value
    assert L.tq_nnw_grad_create(None, 8, 7, 64, 0) == -1
    assert L.tq_nnw_grad_step(None, None, 0, 0, None, None, None, None, None, None, None, None) == -1
    assert L.tq_nnw_grad_load(None, None, None, None) == -1
    assert L.tq_nnw_grad_check(None, None) == -1
    assert L.tq_nnw_grad_destroy(None) == 0
    assert "NNWideGrad" in T.__all__ and T.NNWideGrad is T.policy.NNWideGrad
