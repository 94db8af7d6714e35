"""What the three families' forward entry points share and a host test cannot see (csrc/abi_forward.hpp): the walk over
a call's rows in passes of max_rows, with the stack's bytes per row taken from d and the dtype.  A call cut into four
passes, the last one short, gives the bits of the same rows in one pass -- for NN_11, a wide net and a ResNet, a float32
and a uint8 stack; and NN_11's row list is walked the same way over a stack that stays where it is."""
import numpy as np
import pytest
import torch

import nn11_cases
import nnw_cases
import resnet_cases

pytestmark = pytest.mark.gpu
D = 5
MAX_ROWS = nn11_cases.group(D) - 1             # a pass ends inside a workgroup's group of perspectives
ROWS = 3 * MAX_ROWS + 2                        # four passes, the last one of 2 rows


@pytest.fixture(scope="module")
def T():
    import toric_rl_decoder_amd as T
    assert torch.cuda.is_available()
    T.load()
    return T


def handles(T, family):
    """(the handle of MAX_ROWS rows a pass, the handle that holds ROWS in one pass)"""
    if family == "NN_11":
        sd = nn11_cases.trained_state_dict(D)
        return [T.NN11Forward(sd, D, "cuda", max_rows=m) for m in (MAX_ROWS, ROWS)]
    if family == "NN_8":
        sd = nnw_cases.he_state_dict(8, D)
        return [T.NNWideForward(sd, D, "cuda", max_rows=m) for m in (MAX_ROWS, ROWS)]
    sd = resnet_cases.he_state_dict(18)
    return [T.ResNetForward(sd, D, "cuda", max_rows=m) for m in (MAX_ROWS, ROWS)]


@pytest.mark.parametrize("family", ["NN_11", "NN_8", "ResNet18"])
def test_four_passes_give_the_bits_of_one(T, family):
    assert ROWS == 29 and -(-ROWS // MAX_ROWS) == 4 and ROWS % MAX_ROWS == 2
    walked, whole = handles(T, family)
    x = torch.from_numpy(nn11_cases.dense_rows(D, ROWS)).cuda()
    assert x.dtype == torch.uint8 and tuple(x.shape) == (ROWS, 2, D, D)
    for dt in (torch.float32, torch.uint8):                     # 4 bytes and 1 byte per element: another stride per pass
        stack = x.to(dt)
        want = whole(stack)
        assert bool(torch.isfinite(want).all()) and torch.unique(want, dim=0).shape[0] > ROWS // 2     # a mix-up of rows shows
        got = walked(stack)
        assert got.dtype == torch.float32 and tuple(got.shape) == (ROWS, 3)
        assert torch.equal(got, want), (family, dt, int((got != want).any(dim=1).sum()))
    if family == "NN_11":
        rng = np.random.default_rng(29)
        rows = torch.from_numpy(rng.integers(0, ROWS, 2 * MAX_ROWS + 5).astype(np.int32)).cuda()   # three passes, with repeats
        assert torch.equal(walked(stack, rows), walked(stack)[rows.long()])
        assert torch.equal(walked(stack, rows), whole(stack, rows))
        walked.check()
        whole.check()
    walked.close()
    whole.close()
