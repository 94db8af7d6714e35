"""Inputs and yardsticks shared by tests/test_nnw_host.py and tests/test_gpu_nnw.py (not a test module):
tests/nn11_cases.py generalised from NN_11 to a channel list, for the wide nets NN_8 (net 8) and NN_17 (net 17).

  integer_state_dict   weights under which every activation is a small integer, so that a bf16 / f32-accumulate forward
                       must equal torch's f32 forward bit for bit
  contract_forward     the numerics contract of include/toricenv.h restated in torch ops: the yardstick for weights that
                       are not integers (he_state_dict: no trained NN_8 / NN_17 checkpoint exists)
  exact_dense_case     a network with one dense layer and real bf16 roundings (ties included) whose every f32 sum is
                       exact, and its Q-table by dense_reference, a float64 forward of the contract with nn11_cases'
                       switches for the ways a kernel can be subtly wrong (MUTANTS)
What does not depend on the network (the stacks, the roundings, the limits, the mutants' names) is nn11_cases' own.
"""
import numpy as np
import torch
import torch.nn.functional as F

import toric_rl_decoder_amd as T

from nn11_cases import (CASE_LIMIT, EXACT_LIMIT, MUTANTS, SPARSE_TAPS, TIES, alive_quantile, dense_rows,  # noqa: F401
                        dense_rows_for, greedy_per_lattice, group, rms, round_bf16, stack_of)

SIZES = tuple(T.SUPPORTED_SIZES)
NETS = (8, 17)
MODULES = {8: T.NN_8, 17: T.NN_17}
CH = {net: tuple(m.CHANNELS) for net, m in MODULES.items()}
FEAT = 200                                    # channels of the last conv layer of both nets

# (net, d, dense layer) of the dense exact cases, at dense_rows_for(d) rows.  Together: G > 1 and G = 1; four and eight
# waves; the dense layer's non-zero input in the first and in the second staged chunk; a dense layer behind the
# 256 -> 224 step; the valid last layer; d = 3's single output pixel.
CASES = ((17, 7, 2), (17, 7, 12), (17, 7, 20), (17, 13, 9), (17, 21, 16), (17, 3, 11), (8, 5, 4), (8, 9, 8))


def layers(net):
    return len(CH[net]) - 1


def names(net):
    return [f"conv{i + 1}" for i in range(layers(net))] + ["linear1"]


def net_of(sd):
    """the net a state_dict of this module's making belongs to, by its layer count"""
    return {2 * (layers(net) + 1): net for net in NETS}[len(sd)]


def integer_state_dict(net, d):
    """Seeded by (net, d).  Every output channel of every conv: +1 at one random (input channel, tap) and, with
    probability 1/2, -1 at another; biases 1 with probability 1/4, else 0; linear weights integers in [-8, 8]; linear
    bias integers in [-3, 3].  An activation is at most its layer's number + 1.  At d = 3 the +1 of conv2 and later stands
    at the centre tap: twenty randomly shifted copies of a 3 x 3 grid end in the zero padding, and every row's Q-values
    would be the same (the -1 keeps its random tap there; CASES has d = 3's taps under a dense layer)."""
    rng = np.random.default_rng([11000, net, d])
    ch, sd = CH[net], {}
    for i in range(layers(net)):
        cin, cout = ch[i], ch[i + 1]
        w = np.zeros((cout, cin * 9), np.float32)
        for o in range(cout):
            a, b = rng.choice(cin * 9, 2, replace=False)
            if d == 3 and i > 0:                                # the +1 at the centre tap, see above
                a = a // 9 * 9 + 4
            if rng.random() < 0.5:
                w[o, b] = -1
            w[o, a] = 1
        sd[f"conv{i + 1}.weight"] = torch.from_numpy(w.reshape(cout, cin, 3, 3))
        sd[f"conv{i + 1}.bias"] = torch.from_numpy((rng.random(cout) < 0.25).astype(np.float32))
    sd["linear1.weight"] = torch.from_numpy(rng.integers(-8, 9, (3, FEAT * (d - 2) ** 2)).astype(np.float32))
    sd["linear1.bias"] = torch.from_numpy(rng.integers(-3, 4, 3).astype(np.float32))
    return sd


def he_state_dict(net, d, seed=0):
    """Seeded He-normal conv weights (std sqrt(2 / fan-in)) and small biases: torch's default init lets a 20-layer ReLU
    stack's signal die out.  linear1: normal of std sqrt(1 / fan-in)."""
    g = torch.Generator().manual_seed(17000 + 100 * net + d + seed)
    ch, sd = CH[net], {}
    for i in range(layers(net)):
        cin, cout = ch[i], ch[i + 1]
        sd[f"conv{i + 1}.weight"] = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (cin * 9)) ** 0.5
        sd[f"conv{i + 1}.bias"] = torch.randn(cout, generator=g) * 0.01
    fan = FEAT * (d - 2) ** 2
    sd["linear1.weight"] = torch.randn((3, fan), generator=g) * (1.0 / fan) ** 0.5
    sd["linear1.bias"] = torch.randn(3, generator=g) * 0.01
    return sd


def model_of(sd, d):
    m = MODULES[net_of(sd)](d)
    m.load_state_dict(sd)
    return m.eval()


def layer_outputs(model, x):
    """torch's own forward, layer by layer -> (list of the post-ReLU activations, q)."""
    outs = []
    with torch.no_grad():
        x = F.pad(x, (1, 1, 1, 1), mode="circular")
        for i in range(model.layers):
            x = F.relu(getattr(model, f"conv{i + 1}")(x))
            outs.append(x)
        return outs, model.linear1(x.flatten(1))


def _r(t):
    return t.bfloat16().float()


def contract_forward(model, x):
    """The contract in torch ops: weights .bfloat16().float(), f32 conv2d, .bfloat16().float() after each ReLU, an f32
    linear on rounded weights; biases f32."""
    with torch.no_grad():
        x = F.pad(_r(x.float()), (1, 1, 1, 1), mode="circular")
        for i in range(model.layers):
            c = getattr(model, f"conv{i + 1}")
            x = _r(F.relu(F.conv2d(x, _r(c.weight), c.bias, padding=c.padding)))
        return F.linear(x.flatten(1), _r(model.linear1.weight), model.linear1.bias)


# ---- the dense exact case: nn11_cases' condition.  Every term of every sum is an integer and the sum of the terms'
# magnitudes (the bias included) stays below CASE_LIMIT = 2^23, a factor 2 below where f32 stops holding every integer:
# every partial sum in any order -- any cut into chunks, taps and k-steps -- is an integer that f32 holds.
def mutant_is_void(name, net, d, dense_layer):
    """The last conv has no padding to get wrong; at d = 3 the padding variant is exempt as well (nn11_cases)."""
    return name == "circular padding in the dense layer" and (dense_layer == layers(net) or d == 3)


def dense_reference(sd, x, dense_layer, act_round="rne", weight_round="rne", bias_after_relu=False, circular_dense=False,
                    transpose_dense=False, drop_last_cin_dense=False, fit_bias=False, limit=EXACT_LIMIT, search=None):
    """nn11_cases.dense_reference for a state_dict of either wide net: the contract of include/toricenv.h in float64, in
    plain torch ops.  ``x``: (rows, 2, d, d) tensor of any dtype.  -> (q f64 (rows, 3), stats).

    Asserts for every output of every layer that sum |w a| + |bias| < ``limit``.
    fit_bias: set each conv bias in ``sd`` to -ceil(alive_quantile(d) quantile of the channel's pre-activation over all
    rows and pixels), layer by layer, before it is used.
    search (a magnitude; with fit_bias, no mutant): the fitting pass of exact_dense_case.  It runs in float32 and stops
    at the first layer whose sum of magnitudes reaches ``search``, returning (None, stats) with that sum in
    stats["conv_sum"]: up to there every f32 sum was exact by the condition itself, so a case that fits is fitted to the
    same biases as in float64, and one that does not is turned down either way.
    The other switches (MUTANTS) make a forward that is wrong on purpose; the condition does not apply to its sums."""
    L = len(sd) // 2 - 1
    mutant = (act_round != "rne" or weight_round != "rne" or bias_after_relu or circular_dense or transpose_dense
              or drop_last_cin_dense)
    assert not (mutant and fit_bias) and (search is None or fit_bias)
    check, exact = not mutant, not mutant and limit is not None and search is None
    dt = torch.float64 if search is None else torch.float32

    def rnd(t, mode):
        return round_bf16(t, mode, exact) if search is None else t.bfloat16().float()

    a = rnd(x.to(dt), "rne")
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


# How large the sums get depends on the draw: the last layers multiply what the dense layer left by a factor that varies
# from seed to seed by more than ten (17, 13, 9: 1.2e6 .. 1.6e7 with every layer narrowed).  This is a seed at which all
# of CASES fit the condition within the narrowing steps; exact_dense_case asserts that they do.
DENSE_SEED = 1704


def _dense_state_dict(net, d, dense_layer, dense_mag, linear_mag, unit_layers):
    """nn11_cases._dense_state_dict over CH[net], seeded by (net, d, dense_layer); the conv biases are still to be
    fitted.  conv1 has a TIES weight in every eighth output channel: each of TIES eight times, four with either sign."""
    rng = np.random.default_rng([DENSE_SEED, net, d, dense_layer])
    ch, L, sd = CH[net], layers(net), {}
    w = rng.integers(-1, 2, (ch[1], 18)).astype(np.float64)
    for i, o in enumerate(range(0, ch[1], 8)):
        w[o, rng.integers(18)] = TIES[i % 4] * (1 - (i // 4) % 2 * 2)
    if dense_layer == 2:                                                  # the dense layer's last input channel is alive
        w[-1] = 1
    sd["conv1.weight"] = torch.from_numpy(w.reshape(ch[1], 2, 3, 3)).float()
    for l in range(2, L + 1):
        cin, cout = ch[l - 1], ch[l]
        if l == dense_layer:
            w = rng.choice([-2, -1, 1, 2][2 - dense_mag:2 + dense_mag], (cout, cin * 9)).astype(np.float64)
        else:
            w, mag = np.zeros((cout, cin * 9)), 1 if l > L - unit_layers else 2
            at = np.argpartition(rng.random(w.shape), SPARSE_TAPS, axis=1)[:, :SPARSE_TAPS]      # distinct places per row
            np.put_along_axis(w, at, rng.choice([-2, -1, 1, 2][2 - mag:2 + mag], at.shape).astype(np.float64), axis=1)
            if l == dense_layer - 1:                                      # the dense layer's last input channel is alive
                w[-1] = rng.choice([-2, -1, 1, 2], cin * 9)
        sd[f"conv{l}.weight"] = torch.from_numpy(w.reshape(cout, cin, 3, 3)).float()
    lw = rng.integers(-linear_mag, linear_mag + 1, (3, FEAT * (d - 2) ** 2)).astype(np.float64)
    lw[:, ::97] = rng.choice(TIES, lw[:, ::97].shape) * rng.choice((-1, 1), lw[:, ::97].shape)
    sd["linear1.weight"] = torch.from_numpy(lw).float()
    sd["linear1.bias"] = torch.from_numpy(rng.integers(-3, 4, 3).astype(np.float32))
    for l in range(1, L + 1):
        sd[f"conv{l}.bias"] = torch.zeros(ch[l])
    return sd


_dense = {}


def exact_dense_case(net, d, dense_layer, rows):
    """-> (state_dict, stack (rows, 2, d, d) uint8 numpy, Q-table f32 (rows, 3) numpy, stats of dense_reference).
    nn11_cases.exact_dense_case on the wide net: the stack is dense_rows(d, rows); conv1 dense in {-1, 0, 1} with TIES;
    layer ``dense_layer`` dense in {-2, -1, 1, 2}; SPARSE_TAPS such weights per output channel elsewhere; conv biases
    fitted to this stack; linear1 dense integers in [-2, 2] with a TIES weight in every 97th column.  Where a sum's
    magnitude would reach CASE_LIMIT, first linear1 is narrowed to [-1, 1], then the dense layer to +-1, then the last
    k layers' weights to +-1, k = 1, 2, ... up to the net's layer count.  The fitted network is then held to the
    condition by the float64 reference itself.  Every case is computed once per process."""
    key = (net, d, dense_layer, rows)
    if key not in _dense:
        x = torch.from_numpy(dense_rows(d, rows))
        for narrowed in ((2, 2, 0), (2, 1, 0)) + tuple((1, 1, k) for k in range(layers(net))):
            sd = _dense_state_dict(net, d, dense_layer, *narrowed)
            q, stats = dense_reference(sd, x, dense_layer, fit_bias=True, limit=None, search=CASE_LIMIT)
            if q is not None and stats["linear_sum"] < CASE_LIMIT:
                break
        q, stats = dense_reference(sd, x, dense_layer, limit=CASE_LIMIT)       # the fitted network, held to the condition
        stats["narrowed"] = narrowed
        q32 = q.float()
        assert torch.equal(q32.double(), q)
        _dense[key] = (sd, x.numpy(), q32.numpy(), stats)
    return _dense[key]
