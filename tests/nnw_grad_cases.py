"""Inputs and yardsticks shared by tests/test_nnw_grad_host.py and tests/test_gpu_nnw_grad.py (not a test module): the
learner step of the wide nets NN_8 and NN_17 (include/toricenv.h) on the two cases of
tests/plain_grad_cases.py, bound to nets 8 and 17 through nnw_cases.BOUND.  The one-layer mutants are applied at the
middle of the net."""
import nnw_cases as K
import plain_grad_cases as G
from plain_grad_cases import (LEARNER_POISONS, MUTANT_LAYER, MUTANTS, SUM_LIMIT, RoundBoth, head_contract, manual_backward,  # noqa: F401
                              play_memory, poisoned_batch, reference_backward, tie_records, _rounded_weights)

NETS = K.NETS


def layers(net):
    return K.layers(net)


def mutant_layer(net):
    """the layer a one-layer mutant is applied at: the middle of the net"""
    return layers(net) // 2 + 1


def mutant_switches(net, name):
    """MUTANTS[name] with NN_11's mutant layer replaced by this net's"""
    return G.mutant_switches(name, mutant_layer(net))


def mutant_is_void(name, net, d):
    """No mutant is void at any (net, d) the tests use -- NN_8 at d = 3, 5, 7 and NN_17 at d = 5: the wide nets' last
    channels stay alive at d = 3 as well, where NN_11's die.  tests/test_nnw_grad_host.py runs every mutant at those
    sizes: one named here must change nothing, any other some gradient tensor."""
    return False


def wgrad_persp(d):
    """records per wgrad workgroup: nnw_wgrad_persp of csrc/nnw_grad.hpp"""
    return max(2, 2048 // (d * d))


def row_counts(d):
    """one record; one more than a conv workgroup's perspectives; one more than a wgrad chunk's records (a two-chunk sum)"""
    return sorted({1, K.group(d) + 1, wgrad_persp(d) + 1})


def rounded_layers(c):
    """the layers whose G the case saw changed by RNE"""
    return [l for l, v in c["stats"]["changed"].items() if v > 0]


def _rounding_check(d, stats):
    assert len(rounded_layers({"stats": stats})) >= 2, stats["changed"]             # at least two layers


_cases = {}
BOUND = {net: G.GradCases(K.BOUND[net], tag={"net": net}, seed=lambda d, kind, net=net: [1108, net, d, kind == "rounding"],
                          row_counts=row_counts, g_max=256, rounding_check=_rounding_check, mutant_layer=mutant_layer(net),
                          cache=_cases, keep=6) for net in NETS}


def params(net):
    """the 2 (L + 1) gradient tensors, in model.parameters() order"""
    return BOUND[net].params


def at_rows(c, n, as_f64=False):
    return BOUND[c["net"]].at_rows(c, n, as_f64)


def integer_case(net, d):
    return BOUND[net].integer_case(d)


def rounding_case(net, d):
    return BOUND[net].rounding_case(d)


def mutant_grads(c, name):
    return BOUND[c["net"]].mutant_grads(c, name)
