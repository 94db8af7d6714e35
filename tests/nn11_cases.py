"""Inputs and yardsticks shared by tests/test_nn11_host.py and tests/test_gpu_nn11.py (not a test module).

  integer_state_dict   weights under which every activation of NN_11 is a small integer, so that a bf16 / f32-accumulate
                       forward must equal torch's f32 forward bit for bit
  stack_of             the oracle's perspectives of n lattices reset at p = 0.1
  contract_forward     the numerics contract of include/toricenv.h restated in torch ops: the yardstick for trained weights
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import toric_rl_decoder_amd as T
from oracle import toric_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = tuple(T.SUPPORTED_SIZES)
CH = T.NN_11.CHANNELS
NAMES = [f"conv{i + 1}" for i in range(11)] + ["linear1"]


def integer_state_dict(d):
    """Seeded by d.  Every output channel of every conv: +1 at one random (input channel, tap) and, with probability
    1/2, -1 at another; biases 1 with probability 1/4, else 0; linear weights integers in [-8, 8]; linear bias integers
    in [-3, 3]."""
    rng = np.random.default_rng(11000 + d)
    sd = {}
    for i in range(11):
        cin, cout = CH[i], CH[i + 1]
        w = np.zeros((cout, cin * 9), np.float32)
        for o in range(cout):
            a, b = rng.choice(cin * 9, 2, replace=False)
            w[o, a] = 1
            if rng.random() < 0.5:
                w[o, b] = -1
        sd[f"conv{i + 1}.weight"] = torch.from_numpy(w.reshape(cout, cin, 3, 3))
        sd[f"conv{i + 1}.bias"] = torch.from_numpy((rng.random(cout) < 0.25).astype(np.float32))
    sd["linear1.weight"] = torch.from_numpy(rng.integers(-8, 9, (3, 64 * (d - 2) ** 2)).astype(np.float32))
    sd["linear1.bias"] = torch.from_numpy(rng.integers(-3, 4, 3).astype(np.float32))
    return sd


def trained_state_dict(d):
    from safetensors.torch import load_file
    return load_file(os.path.join(GOLDEN, f"nn11_d{d}_converged.safetensors"))


def model_of(sd, d):
    m = T.NN_11(d)
    m.load_state_dict(sd)
    return m.eval()


def stack_of(d, n, seed=7):
    """-> (perspectives (P,2,d,d) uint8, offsets (n+1,) int64) of n lattices reset at p = 0.1."""
    _, st = O.reset_lattices(seed + d, np.arange(n), 0, 0.1, d)
    per, _, _, off = O.generate_perspective_batch(st)
    return np.ascontiguousarray(per, np.uint8), off


def layer_outputs(model, x):
    """torch's own forward, layer by layer -> (list of the eleven post-ReLU activations, q)."""
    outs = []
    with torch.no_grad():
        x = F.pad(x, (1, 1, 1, 1), mode="circular")
        for i in range(11):
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
        for i in range(11):
            c = getattr(model, f"conv{i + 1}")
            x = _r(F.relu(F.conv2d(x, _r(c.weight), c.bias, padding=c.padding)))
        return F.linear(x.flatten(1), _r(model.linear1.weight), model.linear1.bias)


def rms(a, b):
    return float(torch.sqrt(torch.mean((a.double() - b.double()) ** 2)))


def greedy_per_lattice(q, off):
    """first maximum over each lattice's (count, 3) slice, as a flat index into the slice."""
    q = q.detach().cpu().numpy()
    return np.array([int(np.argmax(q[off[i]:off[i + 1]].reshape(-1))) for i in range(len(off) - 1)])
