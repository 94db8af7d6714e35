"""Inputs and yardsticks shared by tests/test_resnet_host.py and tests/test_gpu_resnet.py (not a test module):
tests/nnw_cases.py generalised from a chain of convolutions to the block graph of the BasicBlock ResNets, ResNet18
(net 18) and ResNet34 (net 34), in eval mode.

  integer_state_dict   weights and BatchNorm statistics under which every activation is a small integer, so that a bf16 /
                       f32-accumulate forward must equal the float64 reference bit for bit at every size, and torch's own
                       f32 forward where the pool's s^2 is a power of two (d = 3, 7, 15)
  contract_forward     the numerics contract of include/toricenv.h restated in torch ops: the yardstick for weights that
                       are not integers (he_state_dict: no trained ResNet checkpoint exists)
  exact_dense_case     a network with one dense convolution and real bf16 roundings (ties included) whose every f32 sum is
                       exact, and its Q-table by dense_reference, a float64 forward of the contract with switches for the
                       ways a kernel can be subtly wrong (MUTANTS: nn11_cases' and the block graph's own)
What does not depend on the network (the stacks, the roundings, the limits) is nn11_cases' own.
"""
import numpy as np
import torch
import torch.nn.functional as F

import toric_rl_decoder_amd as T
from toric_rl_decoder_amd import resnet as R

from nn11_cases import (CASE_LIMIT, EXACT_LIMIT, SPARSE_TAPS, TIES, alive_quantile, dense_rows, dense_rows_for,  # noqa: F401
                        greedy_per_lattice, group, rms, round_bf16, stack_of)
from nn11_cases import MUTANTS as CHAIN_MUTANTS

SIZES = tuple(T.SUPPORTED_SIZES)
NETS = (18, 34)
MODULES = {18: T.ResNet18, 34: T.ResNet34}
EPS = 1e-5
UNIT_VAR = np.float32(0.99999)                # float32(0.99999) + float32(1e-5) == 1.0f: the fold's sqrt and / are exact
assert np.float32(UNIT_VAR + np.float32(EPS)) == np.float32(1.0)

# (net, d, dense convolution) of the dense exact cases, at dense_rows_for(d) rows.  d = 3: s = 2, a whole half grid inside
# one tile; behind a 1x1 shortcut; the stride-2 convolution; 512 -> 512, four chunks x four block rows; G = 1; eight waves
# and s = 11; the deeper block list.
CASES = ((18, 3, "layer2.1.conv1"), (18, 5, "layer2.0.conv2"), (18, 7, "layer4.0.conv1"), (18, 9, "layer4.1.conv2"),
         (18, 15, "layer3.1.conv1"), (18, 21, "layer1.1.conv2"), (34, 7, "layer3.5.conv2"))

# switches of dense_reference: each a way a kernel can be wrong that the dense cases must see (tests/test_resnet_host.py)
MUTANTS = dict(CHAIN_MUTANTS)
MUTANTS.update({
    "residual added after the ReLU": dict(residual_after_relu=True),
    "residual not added": dict(no_residual=True),
    "shortcut image not rounded to bf16": dict(shortcut_unrounded=True),
    "shift dropped": dict(drop_shift=True),
    "scale folded into the weights before rounding": dict(fold_scale=True),
    "stride-2 source at (2y+ky, 2x+kx)": dict(stride_offset=True),
    "1x1 reads tap 0": dict(one_by_one_tap0=True),
    "pool divided by d^2": dict(pool_by_d2=True),
    "conv1 circular": dict(stem_circular=True),
})


# integer_state_dict's draw per (net, d), 0 elsewhere: the residual sums of random +-1 taps grow or die out from draw to
# draw; at these every activation of dense_rows(d, dense_rows_for(d)) stays within the 256 up to which bf16 holds every
# integer, every row gets its own Q-values and some of the last image is alive (tests/test_resnet_host.py asserts it)
INTEGER_DRAW = {(18, 5): 2, (18, 7): 2, (18, 11): 3, (34, 5): 7, (34, 9): 25}
INTEGER_CASES = tuple((18, d) for d in SIZES) + ((34, 5), (34, 9))
TORCH_EXACT_SIZES = (3, 7, 15)                # s^2 = 4, 16, 64: torch's own mean over the pixels is exact there


def convs(net):
    return R.convs(net)


def half(d):
    return (d + 1) // 2


def graph(net):
    """-> the stem's (conv, bn) and a list of blocks (conv1, bn1, conv2, bn2, shortcut (conv, bn) or None, stride)."""
    cs = convs(net)
    blocks, i = [], 1
    while i < len(cs):
        sc = i + 2 < len(cs) and ".shortcut." in cs[i + 2][0]
        stride = 2 if cs[i][0].startswith("layer4.0.") else 1
        blocks.append((cs[i][:2], cs[i + 1][:2], cs[i + 2][:2] if sc else None, stride))
        i += 3 if sc else 2
    return cs[0][:2], blocks


def feeder(net, dense):
    """the convolution that writes the image ``dense`` reads: the block's conv1 for a conv2, else the conv2 of the block
    before (the stem for the first block); with the identity shortcut its last channel passes through the ReLU of the sum"""
    names = [c for c, _, _ in convs(net) if ".shortcut." not in c]
    return names[names.index(dense) - 1]


def net_of(sd):
    return R.which_net(sd)


def model_of(sd):
    m = MODULES[net_of(sd)]()
    m.load_state_dict(sd)
    return m.eval()


def _with_counters(sd, net):
    for _, bn, _ in convs(net):
        sd[bn + ".num_batches_tracked"] = torch.tensor(7)
    return sd


def integer_state_dict(net, d, draw=None):
    """Seeded by (net, d, draw); ``draw`` defaults to INTEGER_DRAW's.  Every output channel of every convolution: +1 at one
    random (input channel, tap) and, with probability 1/2, -1 at another.  BatchNorm: running_var = float32(0.99999), so
    that var + eps == 1.0f exactly and the fold (and torch's own eval BatchNorm) is exact; gamma 1, or with probability
    1/8 each 2 and 0.5; beta and the running mean small integers.  A channel with gamma 2 and an even beta holds even
    values only; gamma 0.5 is given only to a channel all of whose taps read such even channels (and its mean is even), so
    that every activation is an integer.  A block's second convolution always has its -1 and a mean of 1 or 2: its sum is
    then more often negative than positive, which keeps the residual sums from doubling block by block.  Linear weights
    integers in [-8, 8], linear bias integers in [-3, 3].  At d = 3 the +1 of every convolution but the stem stands at
    the centre tap (nnw_cases: shifted copies of a 3 x 3 grid end in the zero padding).  dense_reference asserts that
    every sum stays below its limit; the tests assert from its statistics that no activation exceeds 256."""
    rng = np.random.default_rng([18000, net, d, INTEGER_DRAW.get((net, d), 0) if draw is None else draw])
    sd = {}
    stem, blocks = graph(net)
    shape = {c: s for c, _, s in convs(net)}

    def make(conv, bn, even_in, mean_from, both=False):
        cout, cin, k, _ = shape[conv]
        w = np.zeros((cout, cin, k * k), np.float32)
        gamma, beta = np.ones(cout, np.float32), rng.integers(-1, 2, cout).astype(np.float32)
        ev = np.flatnonzero(even_in) if even_in is not None else np.zeros(0, np.int64)
        for o in range(cout):
            u = rng.random()
            halve = u < 0.125 and ev.size >= 2
            chans = rng.choice(ev if halve else cin, 2, replace=False)
            taps = rng.integers(0, k * k, 2)
            if d == 3 and k == 3 and cin > 2:
                taps[0] = 4
            if rng.random() < 0.5 or both:
                w[o, chans[1], taps[1]] = -1
            w[o, chans[0], taps[0]] = 1
            if halve:
                gamma[o] = 0.5
            elif u > 0.875:
                gamma[o], beta[o] = 2, 2 * rng.integers(0, 2)
        sd[conv + ".weight"] = torch.from_numpy(w.reshape(shape[conv]))
        sd[bn + ".weight"], sd[bn + ".bias"] = torch.from_numpy(gamma), torch.from_numpy(beta)
        mean = rng.integers(*mean_from, cout).astype(np.float32)
        mean[gamma == 0.5] *= 2                                 # half an even mean is an integer
        sd[bn + ".running_mean"] = torch.from_numpy(mean)
        sd[bn + ".running_var"] = torch.full((cout,), float(UNIT_VAR))
        return (gamma == 2) & (beta % 2 == 0)

    x_even = make(*stem, None, (0, 2))
    for c1, c2, sc, _ in blocks:
        mid_even = make(*c1, x_even, (0, 2))
        cut_even = make(*sc, x_even, (0, 2)) if sc else x_even
        x_even = make(*c2, mid_even, (1, 3), both=True) & cut_even
    sd["linear.weight"] = torch.from_numpy(rng.integers(-8, 9, (3, 512)).astype(np.float32))
    sd["linear.bias"] = torch.from_numpy(rng.integers(-3, 4, 3).astype(np.float32))
    return _with_counters(sd, net)


def he_state_dict(net, seed=0):
    """Seeded He-normal conv weights (std sqrt(2 / fan-in)); BatchNorm statistics random but sane: running_var uniform in
    [0.5, 2], running_mean and beta normal of std 0.1, gamma 1 + normal of std 0.1.  linear: normal of std sqrt(1 / 512),
    small bias.  No trained ResNet checkpoint exists in the reference."""
    g = torch.Generator().manual_seed(18000 + 100 * net + seed)
    sd = {}
    for conv, bn, shape in convs(net):
        fan = shape[1] * shape[2] * shape[3]
        sd[conv + ".weight"] = torch.randn(shape, generator=g) * (2.0 / fan) ** 0.5
        sd[bn + ".weight"] = 1 + 0.1 * torch.randn(shape[0], generator=g)
        sd[bn + ".bias"] = 0.1 * torch.randn(shape[0], generator=g)
        sd[bn + ".running_mean"] = 0.1 * torch.randn(shape[0], generator=g)
        sd[bn + ".running_var"] = 0.5 + 1.5 * torch.rand(shape[0], generator=g)
    sd["linear.weight"] = torch.randn((3, 512), generator=g) * (1.0 / 512) ** 0.5
    sd["linear.bias"] = torch.randn(3, generator=g) * 0.01
    return _with_counters(sd, net)


def fold(sd, bn, eps=EPS):
    """The contract's fold in f32, every operation rounded once: s = gamma / sqrt(var + eps), t = beta - mean s."""
    s = sd[bn + ".weight"].float() / torch.sqrt(sd[bn + ".running_var"].float() + torch.tensor(eps, dtype=torch.float32).to(sd[bn + ".weight"].device))
    return s, sd[bn + ".bias"].float() - sd[bn + ".running_mean"].float() * s


def _r(t, dtype=torch.float32):
    """rounded to bf16, held as ``dtype``"""
    return t.float().bfloat16().to(dtype)


def contract_forward(model, x, eps=EPS, dtype=torch.float32):
    """The contract in torch ops, f32: weights and the stack .bfloat16().float(), f32 conv2d, acc s + t with the folded
    f32 vectors, the residual added before the ReLU, .bfloat16().float() after each ReLU and on the shortcut convolution's
    image, the pool as an f32 sum, the linear layer on rounded weights, divided by s^2, + bias.  ``dtype``: float64 runs
    the same roundings and the same f32 fold with float64 sums (what plain_cases.order_free_pattern compares with)."""
    sd = model.state_dict()
    stem, blocks = graph(net_of(sd))

    def r(t):
        return _r(t, dtype)

    def cv(a, conv, bn, stride=1):
        w = r(sd[conv + ".weight"])
        s, t = (v.to(dtype) for v in fold(sd, bn, eps))
        return F.conv2d(a, w, stride=stride, padding=w.shape[-1] // 2) * s[None, :, None, None] + t[None, :, None, None]

    with torch.no_grad():
        a = r(F.relu(cv(r(x), *stem)))
        for c1, c2, sc, stride in blocks:
            mid = r(F.relu(cv(a, *c1, stride)))
            res = r(cv(a, *sc, stride)) if sc else a
            a = r(F.relu(cv(mid, *c2) + res))
        pooled = a.sum((2, 3))
        return pooled @ r(sd["linear.weight"]).T / float(a.shape[2] * a.shape[3]) + sd["linear.bias"].to(dtype)


# ---- the float64 reference.  Every term of every sum is a multiple of one power of two and the sum of the terms'
# magnitudes (scale, shift and residual included) stays below the limit, so every partial sum in any order -- any cut into
# chunks, taps and k-steps -- is a value that f32 holds.
def mutant_is_void(name, net, d, dense):
    """A mutant that cannot show in a case: the unrounded shortcut image where the dense convolution lies in layer4.1,
    behind the last shortcut convolution.  Ahead of the dense convolution the activations of such a case are small integers,
    and so are the shortcut images: bf16 holds every one of them, and rounding changes nothing.
    tests/test_resnet_host.py asserts that the mutated reference of an exempted case gives the unmutated Q-table in bits."""
    return name == "shortcut image not rounded to bf16" and dense.startswith("layer4.1.")


def _conv(a, w, stride, circular=False, offset=False, tap0=False):
    if w.shape[-1] == 3:
        a = F.pad(a, (1, 1, 1, 1), mode="circular") if circular else F.pad(a, (1, 1, 1, 1))
        if offset:                                              # source (2y + ky, 2x + kx): one further down and right
            a = F.pad(a[:, :, 1:, 1:], (0, 1, 0, 1))
        return F.conv2d(a, w, stride=stride)
    if tap0:                                                    # the 1x1 reads (y - 1, x - 1) of the zero-padded grid
        a = F.pad(a, (1, 0, 1, 0))[:, :, :-1, :-1]
    return F.conv2d(a, w, stride=stride)


def dense_reference(sd, x, dense=None, act_round="rne", weight_round="rne", bias_after_relu=False, circular_dense=False,
                    transpose_dense=False, drop_last_cin_dense=False, residual_after_relu=False, no_residual=False,
                    shortcut_unrounded=False, drop_shift=False, fold_scale=False, stride_offset=False, one_by_one_tap0=False,
                    pool_by_d2=False, stem_circular=False, fit=False, limit=EXACT_LIMIT, eps=EPS):
    """The contract of include/toricenv.h in float64, in plain torch ops, over the block graph of the state_dict's net.
    ``x``: (rows, 2, d, d) tensor of any dtype; ``dense``: the name of the dense convolution (the chain mutants act there).
    -> (q f64 (rows, 3) holding f32 values, stats).

    Asserts for every output of every convolution that sum |w a| |s| + |t| + |r| < ``limit``, and the same of the head.
    The head's quotient and sum are rounded to f32 one after the other: f64 holds both exactly enough for that to be the
    correctly rounded f32 operation.
    fit: set each BatchNorm's running mean in ``sd`` to the integer at which the shift is about -ceil(alive_quantile(d)
    quantile of the channel's acc s + r over all rows and pixels), convolution by convolution, before it is used (a
    shortcut convolution: the median, since no ReLU follows).
    The other switches (MUTANTS) make a forward that is wrong on purpose; the condition does not apply to its sums."""
    mutant = (act_round != "rne" or weight_round != "rne" or bias_after_relu or circular_dense or transpose_dense
              or drop_last_cin_dense or residual_after_relu or no_residual or shortcut_unrounded or drop_shift or fold_scale
              or stride_offset or one_by_one_tap0 or pool_by_d2 or stem_circular)
    assert not (mutant and fit)
    check, exact = not mutant, not mutant and limit is not None
    d = x.shape[-1]
    stem, blocks = graph(net_of(sd))
    stats = {"conv_sum": 0.0, "linear_sum": 0.0, "changed": {}, "alive": {}, "max_act": 0.0}

    def cv(a, conv, bn, stride, r=None, relu=True, rounded=True):
        w = sd[conv + ".weight"].double()
        is_dense = conv == dense
        if is_dense and transpose_dense:
            w = w.transpose(2, 3)
        if is_dense and drop_last_cin_dense:
            w = w.clone()
            w[:, -1] = 0
        s, t = (v.double() for v in fold(sd, bn, eps))
        if fold_scale:
            w, s = round_bf16(w * s[:, None, None, None], weight_round, False), torch.ones_like(s)
        else:
            w = round_bf16(w, weight_round, exact)
        kw = dict(stride=stride, circular=(is_dense and circular_dense) or (conv == "conv1" and stem_circular),
                  offset=stride_offset and stride == 2 and w.shape[-1] == 3, tap0=one_by_one_tap0)
        acc = _conv(a, w, **kw)
        s4 = s[None, :, None, None]
        if fit:
            pre = acc * s4 + (r if r is not None else 0)
            qu = torch.quantile(pre.transpose(0, 1).flatten(1), alive_quantile(d) if relu else 0.5, dim=1)
            gamma, beta = sd[bn + ".weight"].double(), sd[bn + ".bias"].double()
            sd[bn + ".running_mean"] = torch.ceil((torch.ceil(qu) + beta) / gamma).float()
            t = fold(sd, bn, eps)[1].double()
        t4 = 0 if drop_shift else t[None, :, None, None]
        if r is None or no_residual:
            r = 0
        if check:
            mag = float((_conv(a.abs(), w.abs(), **kw) * s4.abs() + t[None, :, None, None].abs() + (r.abs() if torch.is_tensor(r) else 0)).max())
            assert limit is None or mag < limit, (conv, mag)
            stats["conv_sum"] = max(stats["conv_sum"], mag)
        if not relu:
            y = acc * s4 + t4
        elif bias_after_relu:
            y = F.relu(acc * s4 + r) + t4
        elif residual_after_relu:
            y = F.relu(acc * s4 + t4) + r
        else:
            y = F.relu(acc * s4 + t4 + r)
        out = round_bf16(y, act_round, exact) if rounded else y
        stats["changed"][conv] = float((out != y).double().mean())
        stats["alive"][conv] = float((out > 0).double().mean())
        stats["max_act"] = max(stats["max_act"], float(out.abs().max()))
        return out

    a = cv(round_bf16(x.double(), "rne", exact), *stem, 1)
    for c1, c2, sc, stride in blocks:
        mid = cv(a, *c1, stride)
        r = cv(a, *sc, stride, relu=False, rounded=not shortcut_unrounded) if sc else a
        a = cv(mid, *c2, 1, r=r)
    pooled = a.sum((2, 3))
    lw = round_bf16(sd["linear.weight"].double(), weight_round, exact)
    lb = sd["linear.bias"].double()
    if check:
        mag = float((pooled.abs() @ lw.abs().T).max())
        assert limit is None or mag < limit, ("linear", mag)
        stats["linear_sum"] = mag
    stats["distinct_features"] = len({r_.tobytes() for r_ in pooled.numpy()}) / pooled.shape[0]
    stats["pooled"] = pooled
    npix = d * d if pool_by_d2 else a.shape[2] * a.shape[3]
    q = ((pooled @ lw.T) / npix).float().double()
    return (q + lb).float().double(), stats


def head_in_kernel_order(pooled, lin_w, lin_b, npix):
    """The head of the contract in numpy f32, in k_resnet_head's order of sums: lane l of 64 sums S[c] bf16(W[a][c]) over its
    channels c = 8 l .. 8 l + 7 in order, every product and sum rounded once; the butterfly over the lanes (xor 32, 16,
    .., 1), read at lane 0; / npix; + bias.  ``pooled``: (rows, 512) channel sums that f32 holds (dense_reference's
    stats["pooled"]).  -> f32 (rows, 3).  Where the sums are not exact this order is the one right answer in bits."""
    S = pooled.numpy().astype(np.float32)
    assert np.array_equal(S.astype(np.float64), pooled.numpy())
    W = lin_w.float().bfloat16().float().numpy()
    q = np.empty((S.shape[0], 3), np.float32)
    for a in range(3):
        prod = (S * W[a][None, :]).reshape(S.shape[0], 64, 8)       # f32 products, rounded once
        lane = np.zeros((S.shape[0], 64), np.float32)
        for j in range(8):
            lane = lane + prod[:, :, j]
        for m in (32, 16, 8, 4, 2, 1):
            lane = lane + lane[:, np.arange(64) ^ m]
        q[:, a] = lane[:, 0] / np.float32(npix) + lin_b.float().numpy()[a]
    return q


def head_order_case(net=18, d=7):
    """An integer net (every activation and channel sum exact) under a linear layer of seeded normal weights, so that the
    head's sums round and their order shows: -> (state_dict, stack uint8, Q-table f32 by head_in_kernel_order, the same
    sums in plain channel order f32)."""
    sd = integer_state_dict(net, d)
    g = torch.Generator().manual_seed(18500 + d)
    sd["linear.weight"] = torch.randn((3, 512), generator=g)
    sd["linear.bias"] = torch.randn(3, generator=g)
    per = dense_rows(d, dense_rows_for(d))
    _, stats = dense_reference(sd, torch.from_numpy(per), limit=None)
    npix = half(d) ** 2
    want = head_in_kernel_order(stats["pooled"], sd["linear.weight"], sd["linear.bias"], npix)
    S = stats["pooled"].numpy().astype(np.float32)
    W = sd["linear.weight"].bfloat16().float().numpy()
    plain = np.zeros((S.shape[0], 3), np.float32)
    for c in range(512):
        plain = plain + S[:, c:c + 1] * W[:, c][None, :]
    plain = plain / np.float32(npix) + sd["linear.bias"].numpy()[None, :]
    return sd, per, want, plain


# The seed at which all of CASES fit the condition within the narrowing steps; exact_dense_case asserts that they do.
DENSE_SEED = 1801
DENSE_SPARSE_TAPS = 2                         # non-zero weights per output channel of a convolution that is not dense: with
                                              # nn11_cases' 4 the residual sums outgrow the limit within a few blocks
DENSE_GAMMAS = (1.0, 2.0, 3.0)                # integers, so that every activation is one; 3 is no power of two, so folding
                                              # it into a TIES weight before the rounding gives another bf16 value


def _dense_state_dict(net, d, dense, dense_mag, linear_mag, other_mag, gamma_share):
    """Seeded by (net, d, dense).  The stem dense in {-1, 0, 1} with a TIES weight and gamma 3 in every eighth output
    channel; convolution ``dense`` dense in {-2, -1, 1, 2} (with ``dense_mag`` 1: +-1); DENSE_SPARSE_TAPS such weights per output
    channel elsewhere (+-1 in every convolution if ``unit``); gamma from DENSE_GAMMAS (1 everywhere if ``unit``), beta integers in
    [-2, 2], running_var = float32(0.99999); the running means are still to be fitted.  linear: integers in
    [-linear_mag, linear_mag] with a TIES weight in columns 0 and 257 (the pooled sums are s^2 times an activation)."""
    rng = np.random.default_rng([DENSE_SEED, net, d, sum(map(ord, dense))])
    sd = {}
    for conv, bn, shape in convs(net):
        cout, cin, k, _ = shape
        n = cin * k * k
        gamma = rng.choice(DENSE_GAMMAS, cout, p=(1 - gamma_share, gamma_share / 2, gamma_share / 2))
        if conv == "conv1":
            w = rng.integers(-1, 2, (cout, n)).astype(np.float64)
            for i, o in enumerate(range(0, cout, 8)):
                w[o, rng.integers(n)] = TIES[i % 4] * (1 - (i // 4) % 2 * 2)
                gamma[o] = 3.0
        elif conv == dense:
            w = rng.choice([-2, -1, 1, 2][2 - dense_mag:2 + dense_mag], (cout, n)).astype(np.float64)
        else:
            w, mag = np.zeros((cout, n)), other_mag
            taps = min(DENSE_SPARSE_TAPS, n)
            at = np.argpartition(rng.random(w.shape), taps, axis=1)[:, :taps]
            np.put_along_axis(w, at, rng.choice([-2, -1, 1, 2][2 - mag:2 + mag], at.shape).astype(np.float64), axis=1)
            if conv == feeder(net, dense):                      # the dense convolution's last input channel is alive
                w[-1] = rng.choice([-2, -1, 1, 2], n)
        sd[conv + ".weight"] = torch.from_numpy(w.reshape(shape)).float()
        sd[bn + ".weight"] = torch.from_numpy(gamma).float()
        sd[bn + ".bias"] = torch.from_numpy(rng.integers(-2, 3, cout).astype(np.float32))
        sd[bn + ".running_mean"] = torch.zeros(cout)
        sd[bn + ".running_var"] = torch.full((cout,), float(UNIT_VAR))
    lw = rng.integers(-linear_mag, linear_mag + 1, (3, 512)).astype(np.float64)
    lw[:, ::257] = rng.choice(TIES, lw[:, ::257].shape) * rng.choice((-1, 1), lw[:, ::257].shape)
    sd["linear.weight"] = torch.from_numpy(lw).float()
    sd["linear.bias"] = torch.from_numpy(rng.integers(-3, 4, 3).astype(np.float32))
    return _with_counters(sd, net)


# (dense_mag, linear_mag, other_mag, gamma_share) of _dense_state_dict, tried in turn
NARROWING = ((2, 1, 1, 0.2), (2, 1, 1, 0.1), (2, 1, 1, 0.05), (2, 1, 1, 0.025), (2, 1, 1, 0.0125), (2, 1, 1, 0.0), (1, 1, 1, 0.0))
_dense = {}


def exact_dense_case(net, d, dense, rows):
    """-> (state_dict, stack (rows, 2, d, d) uint8 numpy, Q-table f32 (rows, 3) numpy, stats of dense_reference).
    The stack is dense_rows(d, rows); the network _dense_state_dict's, its running means fitted to this stack.  Where a
    sum's magnitude would reach CASE_LIMIT, first linear is narrowed to [-1, 1], then the dense convolution to +-1, then
    every other convolution to +-1 with gamma 1.  The fitted network is then held to the condition by the float64
    reference itself.  Every case is computed once per process."""
    key = (net, d, dense, rows)
    if key not in _dense:
        x = torch.from_numpy(dense_rows(d, rows))
        for narrowed in NARROWING:
            sd = _dense_state_dict(net, d, dense, *narrowed)
            _, stats = dense_reference(sd, x, dense, fit=True, limit=None)
            if max(stats["conv_sum"], stats["linear_sum"]) < CASE_LIMIT:
                break
        q, stats = dense_reference(sd, x, dense, limit=CASE_LIMIT)             # the fitted network, held to the condition
        stats["narrowed"] = narrowed
        _dense[key] = (sd, x.numpy(), q.float().numpy(), stats)
    return _dense[key]
