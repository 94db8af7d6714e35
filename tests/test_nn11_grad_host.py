"""NN_11's learner step without a GPU: the host side of toric-rl-decoder_amd/csrc/nn11.hpp and nn11_grad.hpp -- the
forward and dgrad pack routines, the index functions, the four tap -> source pixel maps and the head -- built with g++
through tests/host_nn11_grad_shim.cpp and driven by a scalar forward + backward under the numerics contract of
include/toricenv.h, against the two cases of tests/nn11_grad_cases.py.  Test-only build: the product has no CPU path."""
import ctypes as C

import numpy as np
import pytest
import torch

import toric_rl_decoder_amd as T

import nn11_cases as K
import nn11_grad_cases as GC
from host_build import build_shim

FULL = 3                                                   # NN11_FULL of csrc/nn11.hpp


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    lib = build_shim(tmp_path_factory, "host_nn11_grad_shim.cpp", fast=True, openmp=True)
    vp = C.c_void_p
    lib.shim_nn11_grad.restype = C.c_int
    lib.shim_nn11_grad.argtypes = [C.c_int, C.POINTER(vp), C.POINTER(vp), vp, C.c_int, vp, vp, vp, vp, vp, C.POINTER(vp), C.POINTER(vp)]
    lib.shim_nn11_dgrad_image.restype = C.c_int64
    lib.shim_nn11_dgrad_image.argtypes = [C.c_int, vp, vp]
    lib.shim_nn11_dimg_of.restype = C.c_int64
    lib.shim_nn11_head.restype = None
    lib.shim_nn11_head.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp]
    return lib


def shim_step(shim, c, d, rows, wv):
    sd = c["sd"]
    wts = [np.ascontiguousarray(sd[n + ".weight"].numpy(), np.float32) for n in K.NAMES]
    bs = [np.ascontiguousarray(sd[n + ".bias"].numpy(), np.float32) for n in K.NAMES]
    gw, gb = [np.full_like(a, np.nan) for a in wts], [np.full_like(a, np.nan) for a in bs]
    ptrs = lambda arrs: (C.c_void_p * 12)(*[a.ctypes.data for a in arrs])
    x = np.ascontiguousarray(c["x"][:rows], np.uint8)
    a, y = c["actions"][:rows].numpy().copy(), c["y"][:rows].numpy().copy()
    wv = wv.numpy().copy()
    q, loss = np.full((rows, 3), np.nan, np.float32), np.full(rows, np.nan, np.float32)
    assert shim.shim_nn11_grad(d, ptrs(wts), ptrs(bs), x.ctypes.data, rows, a.ctypes.data, y.ctypes.data, wv.ctypes.data,
                               q.ctypes.data, loss.ctypes.data, ptrs(gw), ptrs(gb)) == 0
    grads = {}
    for n, w_, b_ in zip(K.NAMES, gw, gb):
        grads[n + ".weight"], grads[n + ".bias"] = w_, b_
    return q, loss, grads


@pytest.mark.parametrize("d", K.SIZES)
def test_both_cases_equal_their_references_bit_for_bit_and_every_mutant_differs(shim, d):
    """At the largest row count of tests/test_gpu_nn11_grad.py.  Case 1 (asserted by GC.integer_case: nothing rounds,
    torch's own f32 autograd is the reference, every gradient tensor is non-zero); case 2 (GC.rounding_case: G rounds,
    ties included, every sum exact, float64 autograd is the reference)."""
    assert shim.shim_nn11_wgrad_persp(d) == GC.wgrad_persp(d)
    counts = GC.row_counts(d)
    for c in (GC.integer_case(d), GC.rounding_case(d)):
        for rows in (counts[-1], counts[len(counts) // 2]):
            w, want_loss, want = GC.at_rows(c, rows)
            q, loss, grads = shim_step(shim, c, d, rows, w)
            assert np.array_equal(q, c["q"][:rows]) and np.array_equal(loss, want_loss)
            for k in GC.PARAMS:
                assert np.array_equal(grads[k], want[k]), (d, rows, k, int((grads[k] != want[k]).sum()))
    rows, want = counts[-1], GC.at_rows(c, counts[-1])[2]
    seen = {}
    for name in GC.MUTANTS:
        if GC.mutant_is_void(name, d):
            continue
        m = GC.mutant_grads(c, name)
        seen[name] = [k for k in GC.PARAMS if not np.array_equal(m[k].float().numpy(), want[k])]
        assert seen[name], (d, name)
    st = c["stats"]
    print(f"nn11 grad cases d={d}: {rows} records, largest sum of magnitudes {st['sum_max']:.3g} of {GC.SUM_LIMIT:.3g}, largest |G| "
          f"{st['g_max']:.0f}, RNE changed {', '.join(f'G{l}: {v:.4f}' for l, v in st['changed'].items())}; tensors changed by each "
          f"mutant: {', '.join(f'{k}: {len(v)}' for k, v in seen.items())}")
    assert len(seen) >= len(GC.MUTANTS) - 1


def test_the_dgrad_image_element_by_element(shim):
    """element (ci, co, tap') of layer l's image, found through the header's fragment index, is bf16(W[co][ci][8 - tap']);
    everything else in the image is the zero padding."""
    rng = np.random.default_rng(5)
    for l in range(2, 12):
        cin, cout = K.CH[l - 1], K.CH[l]
        w = rng.normal(size=(cout, cin, 3, 3)).astype(np.float32)
        n = shim.shim_nn11_dgrad_image(l, None, None)
        assert n == 9 * ((cout + 31) // 32 * 32) * ((cin + 31) // 32 * 32)
        img = np.full(n, 0xFFFF, np.uint16)
        shim.shim_nn11_dgrad_image(l, w.ctypes.data, img.ctypes.data)
        want = torch.from_numpy(w).bfloat16().view(torch.int16).numpy().view(np.uint16)
        idx = np.array([[[shim.shim_nn11_dimg_of(l, ci, co, t) for t in range(9)] for ci in range(cin)] for co in range(0, cout, 7)])
        assert np.array_equal(img[idx], want[::7].reshape(len(range(0, cout, 7)), cin, 9)[:, :, ::-1]), l
        assert len(set(idx.ravel().tolist())) == idx.size and 0 <= idx.min() and idx.max() < n
        assert int((img != 0).sum()) == int((want != 0).sum()), l           # what is not a weight is the zero padding


@pytest.mark.parametrize("d", K.SIZES)
def test_the_full_mode_pixel_map_element_by_element(shim, d):
    """conv11's transpose: output pixel (y, x) of the d x d grid takes tap (ky, kx) from (y + ky - 2, x + kx - 2) of the
    (d-2) x (d-2) grid, or nothing.  Restated through the forward's own valid map: s is the source of (y, x) under tap'
    exactly when (y, x) is the valid-mode source of s under the flipped tap."""
    o = d - 2
    for y in range(d):
        for x in range(d):
            for tap in range(9):
                sy, sx = y + tap // 3 - 2, x + tap % 3 - 2
                want = sy * o + sx if 0 <= sy < o and 0 <= sx < o else -1
                got = shim.shim_nn11_src_pixel(FULL, d, y, x, tap)
                assert got == want, (d, y, x, tap)
                if got >= 0:
                    assert shim.shim_nn11_src_pixel(2, d, got // o, got % o, 8 - tap) == y * d + x


@pytest.mark.parametrize("n", (1, 6, 13, 64, 1000))
def test_the_head_is_the_contract_expression_bit_for_bit(shim, n):
    """arbitrary f32 q, y and w (and w = None) against the contract in f32 torch ops; n = 6 and 13 do not divide evenly"""
    rng = np.random.default_rng(n)
    q = torch.from_numpy((rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-3, 4, (n, 3))).astype(np.float32))
    y = torch.from_numpy((rng.normal(size=n) * 30).astype(np.float32))
    a = torch.from_numpy(rng.integers(0, 3, n))
    for w in (torch.from_numpy(rng.uniform(0.01, 3, n).astype(np.float32)), None):
        loss, dq = GC.head_contract(q, a, y, w)
        qa = np.ascontiguousarray(q.gather(1, a.view(-1, 1)).squeeze(1).numpy())
        got_l, got_g = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
        shim.shim_nn11_head(n, n, qa.ctypes.data, y.numpy().ctypes.data, None if w is None else w.numpy().ctypes.data,
                            got_l.ctypes.data, got_g.ctypes.data)
        assert np.array_equal(got_l, loss.numpy())
        assert np.array_equal(got_g, dq.gather(1, a.view(-1, 1)).squeeze(1).numpy())
        assert int((dq != 0).sum(1).max()) <= 1
        # it is the gradient of mean(loss): torch's autograd in f64 agrees to f32's rounding
        q64 = q.double().requires_grad_(True)
        w64 = torch.ones(n, dtype=torch.float64) if w is None else w.double()
        (w64 * (y.double() - q64.gather(1, a.view(-1, 1)).squeeze(1)) ** 2).mean().backward()
        assert torch.allclose(q64.grad, dq.double(), rtol=1e-6, atol=1e-30)


def test_create_rejects_bad_arguments_before_the_device_is_touched():
    L = T.load()
    h = C.c_void_p(None)
    for d, max_batch in ((4, 64), (23, 64), (1, 64), (7, 0), (7, -5), (7, 4097)):
        assert L.tq_nn11_grad_create(C.byref(h), d, max_batch, 0) == -1, (d, max_batch)      # TQ_E_INVALID
        assert not h.value
    assert L.tq_nn11_grad_create(None, 7, 64, 0) == -1
    assert L.tq_nn11_grad_step(None, None, 0, 0, None, None, None, None, None, None, None, None) == -1
    assert L.tq_nn11_grad_load(None, None, None, None) == -1
    assert L.tq_nn11_grad_check(None, None) == -1
    assert L.tq_nn11_grad_destroy(None) == 0
    assert "NN11Grad" in T.__all__ and "learnerStep" in T.__all__
