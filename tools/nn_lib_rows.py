#!/usr/bin/env python3
"""nn_lib_rows.py TREE OUT.json: the library's rows of the four nn_*_bench tools, without the torch rows' minutes.

TREE is a checkout of this repository with its library built (this one, or another commit's, to compare two).  Runs the
tools' own case functions with their defaults, all cases in this one process, with stock torch's paths replaced by
trivial work, so that only the rows that run the library's code take time.  The torch_* rows of the result are
meaningless."""
import importlib.util
import json
import os
import sys
import time

root, out = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, root)
import torch
import toric_rl_decoder_amd as T
from toric_rl_decoder_amd import policy

_real = policy._forward_chunked


def _fc(model, persp, chunk, pad_to=1024, backing=None, out=None, rows=None):
    if isinstance(model, torch.nn.Module):                     # a stock torch forward: skipped
        return out.zero_()
    return _real(model, persp, chunk, pad_to=pad_to, backing=backing, out=out, rows=rows)


policy._forward_chunked = _fc


class CheapNN11(T.NN_11):                                      # NN_11's parameters, a trivial torch forward / backward
    def forward(self, x):
        s = sum(p.sum() for p in self.parameters())
        return (s * 0).expand(x.shape[0], 3)


T.NN_11 = CheapNN11


def tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "tools", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


fb, gb, wb, rb = tool("nn_forward_bench"), tool("nn_grad_bench"), tool("nn_wide_bench"), tool("nn_resnet_bench")
cases = [("nn_forward_bench", "d%d" % d, lambda d=d: fb.one_size(d, 7, 5, 2, 1 << 16)) for d in (7, 9)]
cases += [("nn_grad_bench", "d%d" % d, lambda d=d: gb.one_size(d, 7, 5, 2)) for d in (7, 9)]
cases += [("nn_wide_bench", "NN_%d_d%d" % (n, d), lambda n=n, d=d: wb.one(n, d, 7, 5, 2, 1 << 13)) for n in (8, 17) for d in (7, 9)]
cases += [("nn_resnet_bench", "ResNet18_d%d" % d, lambda d=d: rb.one(18, d, 7, 5, 2, 1 << 12)) for d in (7, 9)]
res = {}
for t, c, fn in cases:
    t0 = time.time()
    res.setdefault(t, {})[c] = fn()
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("%s %s %s: %.1f s" % (root, t, c, time.time() - t0), flush=True)
