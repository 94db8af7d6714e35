"""Inputs and yardsticks shared by tests/test_nn11_grad_host.py and tests/test_gpu_nn11_grad.py (not a test module): the
learner step of NN_11 (include/toricenv.h) on cases with one right answer in bits --
tests/plain_grad_cases.py bound to NN_11."""
import nn11_cases as K
import plain_grad_cases as G
from plain_grad_cases import (LEARNER_POISONS, MUTANT_LAYER, MUTANTS, SUM_LIMIT, RoundBoth, head_contract, manual_backward,  # noqa: F401
                              play_memory, poisoned_batch, reference_backward, tie_records, _rounded_weights)

CH, NAMES, PARAMS = K.CH, K.NAMES, K.PARAMS                             # PARAMS: the 24 gradient tensors


def mutant_is_void(name, d):
    """d = 3: conv10's and conv11's last channels are dead on every row (the forward's own masks), and what conv9's
    carries back dies under conv8's mask: no dgrad's last output channel reaches a parameter gradient."""
    return d == 3 and name == "last output channel dropped in one dgrad"


def rounding_layers(d):
    """the layers whose G the rounding case must see changed by RNE.  d = 3 has one pixel in G_11 and nine in G_10; the
    integer network's one or two weights per channel then add at most two bf16 values of one exponent, which bf16 holds:
    from G_9 on nothing rounds at that size, on any rows."""
    return (11, 10) if d == 3 else tuple(range(11, 5, -1))


def wgrad_persp(d):
    """records per wgrad workgroup: nn11_wgrad_persp of csrc/nn11_grad.hpp"""
    return max(2, 1024 // (d * d))


def row_counts(d):
    """the conv kernels' tile and workgroup edges, three counts around the wgrad workgroup's record count and one beyond
    twice that count"""
    g, p = K.group(d), wgrad_persp(d)
    return sorted({1, g, g + 1, 2 * g + 1, 2 * g + 3, p - 1, p, p + 1, 2 * p + 1})


def _rounding_check(d, stats):
    for l in rounding_layers(d):
        assert stats["changed"][l] > 0, (l, stats["changed"])


# at d >= 5 at least 5 % of every conv weight gradient of the integer case is non-zero
BOUND = G.GradCases(K.NET, tag={}, seed=lambda d, kind: [1107, d, kind == "rounding"], row_counts=row_counts, g_max=128,
                    rounding_check=_rounding_check, mutant_layer=MUTANT_LAYER, cache={}, keep=4, min_conv_share=0.05)
at_rows, integer_case, rounding_case, mutant_grads = BOUND.at_rows, BOUND.integer_case, BOUND.rounding_case, BOUND.mutant_grads
