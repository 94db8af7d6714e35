"""Inputs and yardsticks shared by tests/test_nn11_host.py and tests/test_gpu_nn11.py (not a test module):
tests/plain_cases.py bound to NN_11, and what only NN_11 has (a trained checkpoint, the stack-conversion cases)."""
import os

import toric_rl_decoder_amd as T

import plain_cases as P
from plain_cases import (CASE_LIMIT, EXACT_LIMIT, MUTANTS, SPARSE_TAPS, TIES, U8_VALUES, WIDE_SHARE,  # noqa: F401
                         WIDE_VALUES, alive_quantile, contract_forward, dense_reference, dense_rows, dense_rows_for,
                         greedy_per_lattice, group, layer_outputs, rms, round_bf16, stack_of, wide_stack)

NET = P.Plain(11, T.NN_11, integer_seed=lambda d: 11000 + d, dense_seed=lambda d, l: [1100, d, l], sparse=P.sparse_by_row,
              centre_d3=False, alive_conv1=False)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZES = tuple(T.SUPPORTED_SIZES)
CH = NET.ch
NAMES = NET.names
PARAMS = [f"{n}.{k}" for n in NAMES for k in ("weight", "bias")]        # the 24 tensors, in model.parameters() order
DENSE_LAYERS = tuple(range(2, 12))
WIDE_CASES = ((7, 2), (7, 6), (7, 11), (13, 8))       # (d, dense_layer) of the stack-conversion tests


def integer_state_dict(d):
    return P.integer_state_dict(NET, d)


def trained_state_dict(d):
    from safetensors.torch import load_file
    return load_file(os.path.join(GOLDEN, f"nn11_d{d}_converged.safetensors"))


def model_of(sd, d):
    return P.model_of(NET, sd, d)


def mutant_is_void(name, d, dense_layer):
    return P.mutant_is_void(NET, name, d, dense_layer)


def exact_dense_case(d, dense_layer, rows, values=None):
    return P.exact_dense_case(NET, d, dense_layer, rows, values)
