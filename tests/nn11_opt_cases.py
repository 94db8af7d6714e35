"""Inputs and yardsticks shared by tests/test_nn11_opt_host.py and tests/test_gpu_nn11_opt.py (not a test module): NN_11's
optimizer step (include/toricenv.h, DESIGN.md 3.8, csrc/nn11_opt.hpp), whose contract has one right answer in bits.

  consts        nn11_opt_consts restated in Python doubles, each cast to f32 once
  update        the contract per element in numpy f32, one astype(float32) per operation; ``mutant`` names one of MUTANTS,
                the ways a kernel can be subtly wrong
  tensor_case   p, g and the state of one tensor from a seeded generator: zeros in g and in the state, |g| from 1e-22 to
                1e2 (g^2 underflows, is subnormal, is normal), both signs, subnormal v, elements whose p + update is an
                exact tie and elements that the update moves by less than half an ulp (both asserted)
  model_case    that for the 24 parameter tensors of NN_11(d), with the reference's answer; asserts that every mutant of the
                kind differs from the reference in bits
  change_error  the accuracy criterion: relative L2 error of the accumulated change against a float64 run
"""
import math

import numpy as np

from nn11_cases import CH, NAMES, PARAMS  # noqa: F401

f32 = np.float32
HYPER = dict(lr=0.00025, betas=(0.9, 0.999), eps=1e-8, alpha=0.99)      # Learner_mp.py:81-84, torch's defaults for the rest
STEPS = (1, 2, 1000)                                                     # bias corrections far from and near to 1
KINDS = ("Adam", "RMSprop")
MARGIN = 1.25                                                            # two orderings of the same few roundings

MUTANTS = {
    "m as beta1 m + c1 g": ("Adam",),
    "c3 (g g)": KINDS,
    "eps inside the square root": ("Adam",),
    "division by cb dropped": ("Adam",),
    "v c2 + x as one fused multiply-add": KINDS,
    "update applied with the other sign": KINDS,
    "g / sqrt(s + ce)": ("RMSprop",),
}


def shapes(d):
    out = {}
    for i in range(11):
        out[f"conv{i + 1}.weight"], out[f"conv{i + 1}.bias"] = (CH[i + 1], CH[i], 3, 3), (CH[i + 1],)
    out["linear1.weight"], out["linear1.bias"] = (3, 64 * (d - 2) ** 2), (3,)
    return out


def consts(kind, t, lr=HYPER["lr"], betas=HYPER["betas"], eps=HYPER["eps"], alpha=HYPER["alpha"]):
    """-> dict of np.float32 scalars; b1 is only a mutant's"""
    b1, b2 = betas
    if kind == "Adam":
        return dict(c1=f32(1 - b1), c2=f32(b2), c3=f32(1 - b2), cb=f32(math.sqrt(1 - b2 ** t)), ce=f32(eps),
                    cs=f32(-(lr / (1 - b1 ** t))), b1=f32(b1))
    return dict(ca=f32(alpha), c3=f32(1 - alpha), ce=f32(eps), cs=f32(-lr))


def _r(x):
    return np.asarray(x).astype(f32)


def update(kind, c, p, g, m, v, mutant=None):
    """numpy f32 arrays -> (p', m', v'); RMSprop: m is ignored and m' is None, v is the square average"""
    assert mutant is None or kind in MUTANTS[mutant], (kind, mutant)
    with np.errstate(all="ignore"):
        decay = c["c2"] if kind == "Adam" else c["ca"]
        x = _r(c["c3"] * _r(g * g)) if mutant == "c3 (g g)" else _r(_r(c["c3"] * g) * g)
        if mutant == "v c2 + x as one fused multiply-add":
            v1 = (v.astype(np.float64) * np.float64(decay) + x.astype(np.float64)).astype(f32)
        else:
            v1 = _r(_r(v * decay) + x)
        cs = f32(-c["cs"]) if mutant == "update applied with the other sign" else c["cs"]
        if kind == "Adam":
            m1 = _r(_r(c["b1"] * m) + _r(c["c1"] * g)) if mutant == "m as beta1 m + c1 g" else _r(m + _r(c["c1"] * _r(g - m)))
            if mutant == "eps inside the square root":
                den = _r(np.sqrt(_r(v1 + c["ce"])) / c["cb"])
            elif mutant == "division by cb dropped":
                den = _r(np.sqrt(v1) + c["ce"])
            else:
                den = _r(_r(np.sqrt(v1) / c["cb"]) + c["ce"])
            return _r(p + _r(cs * _r(m1 / den))), m1, v1
        den = np.sqrt(_r(v1 + c["ce"])) if mutant == "g / sqrt(s + ce)" else _r(np.sqrt(v1) + c["ce"])
        return _r(p + _r(cs * _r(g / den))), None, v1


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _signed_log(rng, n, lo, hi):
    return (rng.choice((-1.0, 1.0), n) * 10.0 ** rng.uniform(lo, hi, n)).astype(f32)


def tensor_case(shape, kind, t, seed):
    """-> dict(p, g, m, v, ties, stuck) of f32 arrays of ``shape`` (m None for RMSprop).  ties / stuck: how many elements
    have an exact tie in p + update / are not moved by a non-zero update."""
    n = int(np.prod(shape))
    rng = np.random.default_rng([1208, seed, t, kind == "Adam", n])
    g = _signed_log(rng, n, -22, 2)
    g[rng.random(n) < 0.1] = 0
    m = _signed_log(rng, n, -12, 1)
    v = np.abs(_signed_log(rng, n, -44, 2))                               # subnormal below 1.2e-38
    first = rng.random(n) < 0.15                                         # as on the first step
    m[first], v[first] = 0, 0
    c = consts(kind, t)
    u = update(kind, c, np.zeros(n, f32), g, m, v)[0]                    # 0 + update = the update itself
    p = _signed_log(rng, n, -4, 0)
    role = rng.random(n)
    stuck = (role < 0.1) & (u != 0)
    p[stuck] = _signed_log(rng, int(stuck.sum()), 2, 4)                  # half an ulp of p is above any |update| here
    # a tie: p a multiple of U = 2 lowbit(u), with p + u inside the binade whose ulp is U, is an odd multiple of U / 2
    normal = (np.abs(u) >= 1e-30) & (np.abs(u) < 1e10)
    tie = (role >= 0.1) & (role < 0.25) & normal
    mant = (bits(u) & 0x7FFFFF) | 0x800000
    low = (mant & -mant).astype(np.float64) * np.ldexp(1.0, ((bits(u) >> 23) & 0xFF).astype(np.int64) - 150)
    k = rng.integers((1 << 23) - (1 << 21), (1 << 23) + 1, n).astype(np.float64)
    pt = (np.sign(u) * k * 2 * low)
    assert np.array_equal(pt[tie].astype(f32).astype(np.float64), pt[tie])
    p[tie] = pt[tie].astype(f32)
    exact = p.astype(np.float64) + u.astype(np.float64)
    got = update(kind, c, p, g, m, v)[0]
    is_tie = tie & (np.abs(exact - got.astype(np.float64)) == low)
    out = dict(p=p.reshape(shape), g=g.reshape(shape), m=None if kind != "Adam" else m.reshape(shape), v=v.reshape(shape),
               ties=int(is_tie.sum()), stuck=int((stuck & (got == p)).sum()))
    return out


_tensors = {}


def _tensor(name, shape, kind, t):
    """one tensor's case with the reference's answer and which mutants it tells apart; kept (the conv layers do not
    depend on d, so the sizes share them)"""
    key = (name, shape, kind, t)
    if key not in _tensors:
        c = consts(kind, t)
        tc = tensor_case(shape, kind, t, PARAMS.index(name))
        tc["want"] = update(kind, c, tc["p"], tc["g"], tc["m"], tc["v"])
        tc["differs"] = {}
        for mu, kinds in MUTANTS.items():
            if kind in kinds:
                got = update(kind, c, tc["p"], tc["g"], tc["m"], tc["v"], mutant=mu)
                tc["differs"][mu] = any(a is not None and not same_bits(a, b) for a, b in zip(got, tc["want"]))
        _tensors[key] = tc
    return _tensors[key]


def model_case(d, kind, t):
    """-> {parameter name: dict(p, g, m, v, want=(p', m', v'), ...)} for NN_11(d).  Asserted: g^2 underflows, is subnormal
    and is normal; the state has zeros and subnormals; there are ties and stuck elements; every mutant of the kind
    differs from the reference in bits in p' or the state."""
    c = consts(kind, t)
    case = {name: _tensor(name, shape, kind, t) for name, shape in shapes(d).items()}
    g = np.concatenate([tc["g"].ravel() for tc in case.values()])
    with np.errstate(all="ignore"):
        x = _r(_r(c["c3"] * g) * g)
    tiny = np.finfo(f32).tiny
    assert ((x == 0) & (g != 0)).any() and ((x > 0) & (x < tiny)).any() and (x >= tiny).any() and (g == 0).any() and (g < 0).any()
    v = np.concatenate([tc["v"].ravel() for tc in case.values()])
    assert (v == 0).any() and ((v > 0) & (v < tiny)).any()
    ties, stuck = sum(tc["ties"] for tc in case.values()), sum(tc["stuck"] for tc in case.values())
    assert ties >= 100 and stuck >= 100, (ties, stuck)
    for mu, kinds in MUTANTS.items():
        assert kind not in kinds or any(tc["differs"][mu] for tc in case.values()), mu
    return case


def change_error(p_end, p_start, p_end_ref64):
    """relative L2 error of the accumulated change p_end - p_start against the float64 run's"""
    ref = np.asarray(p_end_ref64, np.float64) - np.asarray(p_start, np.float64)
    got = np.asarray(p_end, np.float64) - np.asarray(p_start, np.float64)
    return float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
