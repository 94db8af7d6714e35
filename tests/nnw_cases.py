"""Inputs and yardsticks shared by tests/test_nnw_host.py and tests/test_gpu_nnw.py (not a test module):
tests/plain_cases.py bound to the wide nets NN_8 (net 8) and NN_17 (net 17).  No trained NN_8 / NN_17 checkpoint exists:
he_state_dict stands in for one."""
import toric_rl_decoder_amd as T

import plain_cases as P
from plain_cases import (CASE_LIMIT, EXACT_LIMIT, MUTANTS, SPARSE_TAPS, TIES, alive_quantile, contract_forward,  # noqa: F401
                         dense_reference, dense_rows, dense_rows_for, greedy_per_lattice, group, layer_outputs, rms,
                         round_bf16, stack_of)

SIZES = tuple(T.SUPPORTED_SIZES)
NETS = (8, 17)
MODULES = {8: T.NN_8, 17: T.NN_17}
DENSE_SEED = 1704                             # a seed at which all of CASES fit the condition (P._dense_state_dict)
BOUND = {net: P.Plain(net, m, integer_seed=lambda d, net=net: [11000, net, d],
                      dense_seed=lambda d, l, net=net: [DENSE_SEED, net, d, l], sparse=P.sparse_by_partition,
                      centre_d3=True, alive_conv1=True) for net, m in MODULES.items()}
CH = {net: b.ch for net, b in BOUND.items()}
FEAT = 200                                    # channels of the last conv layer of both nets

# (net, d, dense layer) of the dense exact cases, at dense_rows_for(d) rows.  Together: G > 1 and G = 1; four and eight
# waves; the dense layer's non-zero input in the first and in the second staged chunk; a dense layer behind the
# 256 -> 224 step; the valid last layer; d = 3's single output pixel.
CASES = ((17, 7, 2), (17, 7, 12), (17, 7, 20), (17, 13, 9), (17, 21, 16), (17, 3, 11), (8, 5, 4), (8, 9, 8))


def layers(net):
    return BOUND[net].layers


def names(net):
    return BOUND[net].names


def net_of(sd):
    """the net a state_dict of this module's making belongs to, by its layer count"""
    return {2 * (layers(net) + 1): net for net in NETS}[len(sd)]


def integer_state_dict(net, d):
    return P.integer_state_dict(BOUND[net], d)


def he_state_dict(net, d, seed=0):
    return P.he_state_dict(BOUND[net], d, seed)


def model_of(sd, d):
    return P.model_of(BOUND[net_of(sd)], sd, d)


def mutant_is_void(name, net, d, dense_layer):
    return P.mutant_is_void(BOUND[net], name, d, dense_layer)


def exact_dense_case(net, d, dense_layer, rows):
    return P.exact_dense_case(BOUND[net], d, dense_layer, rows)
