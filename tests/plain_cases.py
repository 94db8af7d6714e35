"""Inputs and yardsticks of the plain conv nets (conv3x3 + ReLU layers over a channel tuple, then one linear layer), once
for NN_11 and the wide nets NN_8 / NN_17 (not a test module).  tests/nn11_cases.py and tests/nnw_cases.py bind a family
each (``Plain``) and are what the tests import.

  integer_state_dict   weights under which every activation is a small integer, so that a bf16 / f32-accumulate forward
                       must equal torch's f32 forward bit for bit
  he_state_dict        seeded He-normal weights, for a net without a trained checkpoint
  stack_of             the oracle's perspectives of n lattices reset at p = 0.1
  contract_forward     the numerics contract of include/toricenv.h restated in torch ops: the yardstick for weights that
                       are not integers
  exact_dense_case     a network with one dense layer and real bf16 roundings (ties included) whose every f32 sum is
                       exact, and its Q-table by dense_reference, a float64 forward of the contract with switches for
                       the ways a kernel can be subtly wrong (MUTANTS)
"""
import functools
from dataclasses import dataclass
from typing import Callable

import numpy as np
import torch
import torch.nn.functional as F

from oracle import toric_oracle as O

TIES = (257, 259, 261, 263)                   # integers bf16 cannot hold, each half-way: RNE -> 256, 260, 260, 264
EXACT_LIMIT = float(1 << 24)
CASE_LIMIT = float(1 << 23)                    # what exact_dense_case keeps to: a factor 2 below the limit
SPARSE_TAPS = 4                               # non-zero weights per output channel of a conv layer that is not dense


def sparse_by_row(rng, w, values):
    """SPARSE_TAPS draws from ``values`` at distinct places of every row of ``w``: one rng.choice per row."""
    for o in range(w.shape[0]):
        w[o, rng.choice(w.shape[1], SPARSE_TAPS, replace=False)] = rng.choice(values, SPARSE_TAPS)


def sparse_by_partition(rng, w, values):
    """... the places of all rows by one argpartition of uniform draws: 256 x 2304 weights make row by row slow."""
    at = np.argpartition(rng.random(w.shape), SPARSE_TAPS, axis=1)[:, :SPARSE_TAPS]
    np.put_along_axis(w, at, rng.choice(values, at.shape).astype(np.float64), axis=1)


@dataclass(frozen=True, eq=False)
class Plain:
    """One net and how its cases are drawn.  The draws of the two families differ in small ways that are kept as they
    were first made, so that every case stays the one the kernels were pinned on."""
    number: int                               # 11, 8, 17
    module: type                              # the torch module class; its CHANNELS are the net's
    integer_seed: Callable                    # d -> seed sequence of integer_state_dict
    dense_seed: Callable                      # (d, dense layer) -> seed sequence of _dense_state_dict
    sparse: Callable                          # sparse_by_row or sparse_by_partition
    centre_d3: bool                           # integer_state_dict puts d = 3's +1 of conv2 and later at the centre tap
    alive_conv1: bool                         # under a dense conv2, conv1's last output channel has all weights 1

    @property
    def ch(self):
        return tuple(self.module.CHANNELS)

    @property
    def layers(self):
        return len(self.ch) - 1

    @property
    def names(self):
        return [f"conv{i + 1}" for i in range(self.layers)] + ["linear1"]


def integer_state_dict(net, d):
    """Every output channel of every conv: +1 at one random (input channel, tap) and, with probability 1/2, -1 at
    another; biases 1 with probability 1/4, else 0; linear weights integers in [-8, 8]; linear bias integers in [-3, 3].
    An activation is at most its layer's number + 1.  centre_d3: twenty randomly shifted copies of a 3 x 3 grid end in
    the zero padding, and every row's Q-values would be the same (the -1 keeps its random tap there)."""
    rng = np.random.default_rng(net.integer_seed(d))
    ch, sd = net.ch, {}
    for i in range(net.layers):
        cin, cout = ch[i], ch[i + 1]
        w = np.zeros((cout, cin * 9), np.float32)
        for o in range(cout):
            a, b = rng.choice(cin * 9, 2, replace=False)
            if net.centre_d3 and d == 3 and i > 0:
                a = a // 9 * 9 + 4
            if rng.random() < 0.5:
                w[o, b] = -1
            w[o, a] = 1
        sd[f"conv{i + 1}.weight"] = torch.from_numpy(w.reshape(cout, cin, 3, 3))
        sd[f"conv{i + 1}.bias"] = torch.from_numpy((rng.random(cout) < 0.25).astype(np.float32))
    sd["linear1.weight"] = torch.from_numpy(rng.integers(-8, 9, (3, ch[-1] * (d - 2) ** 2)).astype(np.float32))
    sd["linear1.bias"] = torch.from_numpy(rng.integers(-3, 4, 3).astype(np.float32))
    return sd


def he_state_dict(net, d, seed=0):
    """Seeded He-normal conv weights (std sqrt(2 / fan-in)) and small biases: torch's default init lets a 20-layer ReLU
    stack's signal die out.  linear1: normal of std sqrt(1 / fan-in)."""
    g = torch.Generator().manual_seed(17000 + 100 * net.number + d + seed)
    ch, sd = net.ch, {}
    for i in range(net.layers):
        cin, cout = ch[i], ch[i + 1]
        sd[f"conv{i + 1}.weight"] = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (cin * 9)) ** 0.5
        sd[f"conv{i + 1}.bias"] = torch.randn(cout, generator=g) * 0.01
    fan = ch[-1] * (d - 2) ** 2
    sd["linear1.weight"] = torch.randn((3, fan), generator=g) * (1.0 / fan) ** 0.5
    sd["linear1.bias"] = torch.randn(3, generator=g) * 0.01
    return sd


def model_of(net, sd, d):
    m = net.module(d)
    m.load_state_dict(sd)
    return m.eval()


def stack_of(d, n, seed=7):
    """-> (perspectives (P,2,d,d) uint8, offsets (n+1,) int64) of n lattices reset at p = 0.1."""
    _, st = O.reset_lattices(seed + d, np.arange(n), 0, 0.1, d)
    per, _, _, off = O.generate_perspective_batch(st)
    return np.ascontiguousarray(per, np.uint8), off


def layer_outputs(model, x):
    """torch's own forward, layer by layer -> (list of the post-ReLU activations, q)."""
    outs = []
    with torch.no_grad():
        x = F.pad(x, (1, 1, 1, 1), mode="circular")
        for i in range(model.layers):
            x = F.relu(getattr(model, f"conv{i + 1}")(x))
            outs.append(x)
        return outs, model.linear1(x.flatten(1))


def _r(t, dtype=torch.float32):
    """rounded to bf16, held as ``dtype``"""
    return t.float().bfloat16().to(dtype)


def contract_forward(model, x, dtype=torch.float32):
    """The contract in torch ops: weights .bfloat16().float(), f32 conv2d, .bfloat16().float() after each ReLU, an f32
    linear on rounded weights; biases f32.  ``dtype``: float64 runs the same roundings with float64 sums (what
    order_free_pattern compares with)."""
    with torch.no_grad():
        x = F.pad(_r(x, dtype), (1, 1, 1, 1), mode="circular")
        for i in range(model.layers):
            c = getattr(model, f"conv{i + 1}")
            x = _r(F.relu(F.conv2d(x, _r(c.weight, dtype), c.bias.to(dtype), padding=c.padding)), dtype)
        return F.linear(x.flatten(1), _r(model.linear1.weight, dtype), model.linear1.bias.to(dtype))


def rms(a, b):
    return float(torch.sqrt(torch.mean((a.double() - b.double()) ** 2)))


def greedy_per_lattice(q, off):
    """first maximum over each lattice's (count, 3) slice, as a flat index into the slice."""
    q = q.detach().cpu().numpy()
    return np.array([int(np.argmax(q[off[i]:off[i + 1]].reshape(-1))) for i in range(len(off) - 1)])


# ---- the dense exact case -------------------------------------------------------------------------------------------
# Every term of every sum is an integer and the sum of the terms' magnitudes (the bias included) stays below 2^24, so
# every partial sum in any order -- any cut into chunks, taps and k-steps -- is an integer that f32 holds: whatever order
# a kernel sums in, it gets the one f32 value, and the bf16 rounding after it is a function of that value.  Bit equality
# may then be demanded of a network that is dense and rounds.
def alive_quantile(d):
    """A channel's bias is -ceil of this quantile of its pre-activation.  0.9 keeps a tenth of the activations alive and
    the sums within the limit; d = 3 has nine pixels, and one in ten of them alive carries a change made in one layer to
    Q in too few rows, so it keeps a quarter alive (its sums are the smallest of all sizes)."""
    return 0.75 if d == 3 else 0.9


# switches of dense_reference: each a way a kernel can be wrong that the dense case must see (the host tests)
MUTANTS = {
    "activations truncated": dict(act_round="trunc"),
    "activations rounded half-up": dict(act_round="half_up"),
    "weights truncated": dict(weight_round="trunc"),
    "bias after the ReLU": dict(bias_after_relu=True),
    "circular padding in the dense layer": dict(circular_dense=True),
    "taps of the dense layer transposed": dict(transpose_dense=True),
    "last input channel of the dense layer dropped": dict(drop_last_cin_dense=True),
}


def mutant_is_void(net, name, d, dense_layer):
    """The last conv has no padding to get wrong; at d = 3 the padding variant is exempt as well."""
    return name == "circular padding in the dense layer" and (dense_layer == net.layers or d == 3)


def round_bf16(t, mode="rne", exact=True):
    """f64 tensor -> its values rounded to bf16, as f64; ``exact`` asserts that f32 holds them all (a mutant's need
    not).  rne: torch's own conversion; trunc: toward zero; half_up: the magnitude's half goes up."""
    f = t.float()
    assert not exact or torch.equal(f.double(), t), "a value that f32 does not hold"
    if mode == "rne":
        return f.bfloat16().double()
    u = f.view(torch.int32)
    if mode == "half_up":
        u = u + 0x8000
    return (u & ~0xFFFF).view(torch.float32).double()


def dense_reference(sd, x, dense_layer, act_round="rne", weight_round="rne", bias_after_relu=False, circular_dense=False,
                    transpose_dense=False, drop_last_cin_dense=False, stack_round="rne", fit_bias=False, limit=EXACT_LIMIT,
                    search=None):
    """The contract of include/toricenv.h in float64, in plain torch ops, for a state_dict of any plain net: stack
    elements and weights rounded to bf16, f64 convolutions under the three paddings, + bias, ReLU, rounded to bf16; an
    f64 linear layer on rounded weights.  ``x``: (rows, 2, d, d) tensor of any dtype.  -> (q f64 (rows, 3), stats).

    Asserts for every output of every layer that sum |w a| + |bias| < ``limit``: at 2^24 the exactness condition.
    fit_bias: set each conv bias in ``sd`` to -ceil(alive_quantile(d) quantile of the channel's pre-activation over all
    rows and pixels), layer by layer, before it is used.
    search (a magnitude; with fit_bias, no mutant): the fitting pass of exact_dense_case.  It runs in float32 and stops
    at the first layer whose sum of magnitudes reaches ``search``, returning (None, stats) with that sum in
    stats["conv_sum"]: up to there every f32 sum was exact by the condition itself, so a case that fits is fitted to the
    same biases as in float64, and one that does not is turned down either way.
    The other switches (MUTANTS, and stack_round for the stack's conversion) make a forward that is wrong on purpose; the
    condition does not apply to its sums."""
    L = len(sd) // 2 - 1
    mutant = (act_round != "rne" or weight_round != "rne" or stack_round != "rne" or bias_after_relu or circular_dense
              or transpose_dense or drop_last_cin_dense)
    assert not (mutant and fit_bias) and (search is None or fit_bias)
    check, exact = not mutant, not mutant and limit is not None and search is None
    dt = torch.float64 if search is None else torch.float32

    def rnd(t, mode):
        return round_bf16(t, mode, exact) if search is None else t.bfloat16().float()

    a = rnd(x.to(dt), stack_round)
    a = F.pad(a, (1, 1, 1, 1), mode="circular")
    stats = {"conv_sum": 0.0, "linear_sum": 0.0, "changed": [], "alive": []}
    for l in range(1, L + 1):
        w = sd[f"conv{l}.weight"].to(dt)
        pad = 0 if l in (1, L) else 1
        if l == dense_layer:
            if transpose_dense:
                w = w.transpose(2, 3)
            if drop_last_cin_dense:
                w = w.clone()
                w[:, -1] = 0
            if circular_dense and pad:
                a, pad = F.pad(a, (1, 1, 1, 1), mode="circular"), 0
        w = rnd(w, weight_round)
        pre = F.conv2d(a, w, None, padding=pad)
        if fit_bias:
            qu = torch.quantile(pre.transpose(0, 1).flatten(1).double(), alive_quantile(x.shape[-1]), dim=1)
            sd[f"conv{l}.bias"] = (-torch.ceil(qu)).float()
        b = sd[f"conv{l}.bias"].to(dt)[None, :, None, None]
        if check:
            mag = float((F.conv2d(a.abs(), w.abs(), None, padding=pad) + b.abs()).max())
            assert limit is None or mag < limit, (l, mag)
            stats["conv_sum"] = max(stats["conv_sum"], mag)
            if search is not None and mag >= search:
                return None, stats
        y = F.relu(pre) + b if bias_after_relu else F.relu(pre + b)
        a = rnd(y, act_round)
        stats["changed"].append(float((a != y).double().mean()))
        stats["alive"].append(float((a > 0).double().mean()))
    feat = a.flatten(1)
    lw = rnd(sd["linear1.weight"].to(dt), weight_round)
    lb = sd["linear1.bias"].to(dt)
    if check:
        mag = float((feat.abs() @ lw.abs().T + lb.abs()).max())
        assert limit is None or mag < limit, ("linear1", mag)
        stats["linear_sum"] = mag
    stats["distinct_features"] = len({r.tobytes() for r in feat.numpy()}) / feat.shape[0]
    return feat @ lw.T + lb, stats


def _dense_state_dict(net, d, dense_layer, dense_mag, linear_mag, unit_layers, ties=True):
    """Seeded by net.dense_seed(d, dense_layer); the conv biases are still to be fitted.  How large the sums get depends
    on the draw: the last layers multiply what the dense layer left by a factor that varies from seed to seed by more
    than ten.  A family's seed is one at which all of its cases fit the condition within exact_dense_case's narrowing
    steps, which asserts that they do."""
    rng = np.random.default_rng(net.dense_seed(d, dense_layer))
    ch, L, sd = net.ch, net.layers, {}
    w = rng.integers(-1, 2, (ch[1], 18)).astype(np.float64)              # conv1: dense in {-1, 0, 1} ...
    for i, o in enumerate(range(0, ch[1], 8) if ties else ()):            # ... with a tie in every eighth channel: each
        w[o, rng.integers(18)] = TIES[i % 4] * (1 - (i // 4) % 2 * 2)     # of TIES as often with either sign
    if net.alive_conv1 and dense_layer == 2:                              # the dense layer's last input channel is alive
        w[-1] = 1
    sd["conv1.weight"] = torch.from_numpy(w.reshape(ch[1], 2, 3, 3)).float()
    for l in range(2, L + 1):
        cin, cout = ch[l - 1], ch[l]
        if l == dense_layer:
            w = rng.choice([-2, -1, 1, 2][2 - dense_mag:2 + dense_mag], (cout, cin * 9)).astype(np.float64)
        else:
            w, mag = np.zeros((cout, cin * 9)), 1 if l > L - unit_layers else 2
            net.sparse(rng, w, [-2, -1, 1, 2][2 - mag:2 + mag])
            if l == dense_layer - 1:                                      # the dense layer's last input channel is alive
                w[-1] = rng.choice([-2, -1, 1, 2], cin * 9)
        sd[f"conv{l}.weight"] = torch.from_numpy(w.reshape(cout, cin, 3, 3)).float()
    lw = rng.integers(-linear_mag, linear_mag + 1, (3, ch[-1] * (d - 2) ** 2)).astype(np.float64)
    if ties:
        lw[:, ::97] = rng.choice(TIES, lw[:, ::97].shape) * rng.choice((-1, 1), lw[:, ::97].shape)
    sd["linear1.weight"] = torch.from_numpy(lw).float()
    sd["linear1.bias"] = torch.from_numpy(rng.integers(-3, 4, 3).astype(np.float32))
    for l in range(1, L + 1):
        sd[f"conv{l}.bias"] = torch.zeros(ch[l])
    return sd


_stacks = {}
WIDE_VALUES = (2, 3) + TIES                    # stack elements beside 0 and 1 that a f32 / f16 stack is given
U8_VALUES = (2, 255)                           # ... and a u8 stack (bf16 holds them)
WIDE_SHARE = 0.1                              # of the stack's elements; the rest stay the perspective's 0 / 1


def dense_rows(d, rows):
    """the first ``rows`` perspectives of stack_of(d, ...), uint8"""
    n = 64
    while d not in _stacks or _stacks[d].shape[0] < rows:
        _stacks[d] = stack_of(d, n)[0]
        n *= 2
    return _stacks[d][:rows]


def wide_stack(d, rows, values):
    """dense_rows(d, rows) as f32 with WIDE_SHARE of its elements replaced by draws from ``values``."""
    rng = np.random.default_rng([1101, d, len(values)])
    x = dense_rows(d, rows).astype(np.float32)
    m = rng.random(x.shape) < WIDE_SHARE
    x[m] = rng.choice(values, int(m.sum()))
    return x


# A test module draws a case in more than one test, test by test and not case by case, so the latest few are kept: 8, the
# longest list any module goes through that way (nnw_cases.CASES); NN_11's hundred are each used by one test.  The key
# holds the Plain by identity, and every caller gets the same state_dict and arrays: they are read, never written.
@functools.lru_cache(maxsize=8)
def exact_dense_case(net, d, dense_layer, rows, values=None):
    """-> (state_dict, stack (rows, 2, d, d) numpy, Q-table f32 (rows, 3) numpy, stats of dense_reference).
    The stack: dense_rows(d, rows), uint8; with ``values``, wide_stack(d, rows, values), f32.
    conv1 dense in {-1, 0, 1} with a TIES weight in every eighth output channel; layer ``dense_layer`` dense in
    {-2, -1, 1, 2}; SPARSE_TAPS such weights per output channel elsewhere; conv biases fitted to this stack
    (dense_reference's fit_bias), which keeps a tenth of the activations alive and the sums from growing; linear1 dense
    integers in [-2, 2] with a TIES weight in every 97th column.  Where a sum's magnitude would reach CASE_LIMIT, first
    linear1 is narrowed to [-1, 1], then the dense layer to +-1, then the last k layers' weights to +-1, k = 1, 2, ...
    With ``values`` the weights hold no TIES and every layer is narrowed at once: an element of 263 under a weight of
    263 is 69169 after conv1, and one such feature under a TIES weight of linear1 would spend the limit by itself; the
    stack's elements bring the roundings there.  The fitted network is then held to the condition by the float64
    reference itself."""
    L = net.layers
    x = torch.from_numpy(dense_rows(d, rows) if values is None else wide_stack(d, rows, values))
    steps = ((2, 2, 0), (2, 1, 0)) + tuple((1, 1, k) for k in range(L)) if values is None else ((1, 1, L - 1),)
    for narrowed in steps:
        sd = _dense_state_dict(net, d, dense_layer, *narrowed, ties=values is None)
        q, stats = dense_reference(sd, x, dense_layer, fit_bias=True, limit=None, search=CASE_LIMIT)
        if q is not None and stats["linear_sum"] < CASE_LIMIT:
            break
    q, stats = dense_reference(sd, x, dense_layer, limit=CASE_LIMIT)           # the fitted network, held to the condition
    stats["narrowed"] = narrowed
    q32 = q.float()
    assert torch.equal(q32.double(), q)
    return sd, x.numpy(), q32.numpy(), stats


def group(d):
    return max(1, 256 // (d * d))              # perspectives per workgroup: NN11Geom<D>::G of csrc/nn11.hpp


def dense_rows_for(d):
    """the row count of the dense case at size d: 2 G + 3 perspectives cross the tile, workgroup and pass edges of a
    handle of G + 1 rows"""
    return 2 * group(d) + 3


# ---- NaN and inf ----------------------------------------------------------------------------------------------------
# The contract (include/toricenv.h): NaN and inf go where the torch / numpy expression of the operation sends them.  A
# NaN is compared by position only; an inf by position and sign; everything else bit for bit.  Non-finite values enter a
# case only as literal NaN / inf elements or as one f32 weight beyond bf16's range, never as finite values near
# overflow, so where they end up does not depend on the order of a sum -- which order_free_pattern asserts case by case.
FINITE, NAN, PLUS_INF, MINUS_INF = 0, 1, 2, 3
OVER_BF16 = 3.4e38                             # an f32 that RNE takes to bf16's +inf (the boundary is 0x7f7f8000 = 3.396e38)
WEIGHT_POISONS = ("nan weight", "inf weight", "nan bias")


def as_numpy(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def pattern(a):
    """-> int8 array: FINITE, NAN, PLUS_INF or MINUS_INF per element"""
    a = as_numpy(a)
    return (np.isnan(a) * NAN + np.isposinf(a) * PLUS_INF + np.isneginf(a) * MINUS_INF).astype(np.int8)


def same_pattern(got, want):
    got, want = as_numpy(got), as_numpy(want)
    return got.shape == want.shape and np.array_equal(pattern(got), pattern(want))


def same_bits_nan_equal(got, want):
    """NaNs at the same places (np.isnan equality; payload and sign free), every other element the same bits"""
    got, want = as_numpy(got), as_numpy(want)
    if got.shape != want.shape or got.dtype != want.dtype or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    keep = ~np.isnan(got)
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return np.array_equal(np.ascontiguousarray(got).view(u)[keep], np.ascontiguousarray(want).view(u)[keep])


def order_free_pattern(forward, *args):
    """forward(*args, dtype=...) in f32 and in f64 -> the f32 result, after asserting that both have the same NaN / inf
    pattern and that it holds a non-finite value at all: a case that fails this is not one."""
    q32, q64 = forward(*args, dtype=torch.float32), forward(*args, dtype=torch.float64)
    assert same_pattern(q32, q64), "where NaN / inf end up depends on the precision of the sums: not a case"
    assert pattern(q32).any(), "the poison does not reach the output: not a case"
    return q32


def poisoned_state_dict(sd, weight, bias, kind, at=0, bias_at=0):
    """A copy of ``sd`` with one element replaced (WEIGHT_POISONS): element ``at`` of the flattened tensor ``weight`` by
    NaN or by OVER_BF16, or element ``bias_at`` of ``bias`` by NaN."""
    assert kind in WEIGHT_POISONS, kind
    out = {k: v.clone() for k, v in sd.items()}
    key, value = (bias, float("nan")) if kind == "nan bias" else (weight, float("nan") if kind == "nan weight" else OVER_BF16)
    out[key].view(-1)[bias_at if kind == "nan bias" else at] = value
    if kind == "inf weight":
        assert bool(torch.isfinite(out[key]).all()) and bool(torch.isinf(out[key].bfloat16()).any())
    return out


def poison_rows(d, rows):
    """the rows of a call of ``rows`` perspectives on a handle of G + 1 that get a poisoned stack element: the first, the
    last of a workgroup and the first of the second pass"""
    g = group(d)
    at = sorted({0, g - 1, g + 1})
    assert at[-1] < rows
    return at
