#!/usr/bin/env python3
"""One selectActionEnvSet call, dense against sparse -> profiles/select_sparse_bench.json.

Dense forwards every perspective; sparse (EnvSet.selectPlan -> NN11Forward(persp, rows) -> the planned selection) only
the R of P perspectives the epsilon-greedy selection reads.  For d = 7 and 9, 4096 and 65 536 lattices, a u8 stack, the
lattices taken from a few steps of policy play at the reference's epsilon schedule (trained weights where
tests/golden has them), and three epsilon settings: all 0 (nothing to save: what the plan and the second read-back cost),
the reference's schedule calculateEpsilon(0.8, 7, n), all 1.  Dense and sparse alternate in seven pairs; each takes the
median of its calls after a warm-up, timed by HIP events around the whole call (its read-backs included).  Per setting:
ms per call, R / P, the spread of the seven medians, and whether sparse was faster in every pair.

Each (size, lattices) runs in a process of its own under a time limit; the first one that fails stops the run.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLAY_STEPS = 4


def reference_eps(n, eps=0.8, alpha=7.0):
    import numpy as np
    return eps ** (1.0 + alpha * np.arange(n) / max(n - 1, 1))          # src/util_actor.py:294-312


def one_case(d, n, pairs, reps, warmup):
    import numpy as np
    import torch
    import toric_rl_decoder_amd as T

    dev = "cuda:0"
    path = os.path.join(ROOT, "tests", "golden", "nn11_d%d_converged.safetensors" % d)
    torch.manual_seed(0)
    model = T.NN_11(d, 3).to(dev).eval()
    trained = os.path.exists(path)
    if trained:
        from safetensors.torch import load_file
        model.load_state_dict(load_file(path))
    fwd = T.NN11Forward(model, d, dev, max_rows=1 << 16)
    envs = T.EnvSet(T.make("toric-code-v0", {"size": d, "min_qubit_errors": 0, "p_error": 0.1}), n, device=dev, seed=d,
                    numpy_io=False)
    envs.resetAll()
    sched = reference_eps(n)
    for _ in range(PLAY_STEPS):                                 # policy play
        act, _ = T.selectActionEnvSet(envs, fwd, sched, dtype=torch.uint8)
        envs.actorStep(act)
    P = int(envs.perspectiveCounts()[1][-1])

    def call(eps, sparse):
        return T.selectActionEnvSet(envs, fwd, eps, dtype=torch.uint8, sparse=sparse)

    def median_ms(eps, sparse):
        for _ in range(warmup):
            call(eps, sparse)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        for _ in range(reps):
            t0.record()
            call(eps, sparse)
            t1.record()
            t1.synchronize()
            out.append(t0.elapsed_time(t1))
        out.sort()
        return out[len(out) // 2]

    res = {"d": d, "lattices": n, "perspectives": P, "trained_weights": trained, "settings": {}}
    for name, eps in (("eps_0", np.zeros(n)), ("reference_schedule", sched), ("eps_1", np.ones(n))):
        eps = torch.from_numpy(np.ascontiguousarray(eps)).to(dev)
        a_d, q_d = (x.clone() for x in call(eps, False))
        a_s, q_s = call(eps, True)
        assert torch.equal(a_d, a_s) and torch.equal(q_d.view(torch.int32), q_s.view(torch.int32)), name
        R = envs.selectPlan(eps).R
        dense, sparse = [], []
        for _ in range(pairs):
            dense.append(median_ms(eps, False))
            sparse.append(median_ms(eps, True))
        md, ms = sorted(dense)[pairs // 2], sorted(sparse)[pairs // 2]
        res["settings"][name] = {
            "rows_forwarded": R, "R_over_P": round(R / max(P, 1), 4),
            "dense_pair_medians_ms": [round(x, 4) for x in dense], "sparse_pair_medians_ms": [round(x, 4) for x in sparse],
            "dense_ms": round(md, 4), "sparse_ms": round(ms, 4), "sparse_over_dense": round(ms / md, 4),
            "sparse_minus_dense_ms": round(ms - md, 4),
            "dense_spread_ms": round(max(dense) - min(dense), 4), "sparse_spread_ms": round(max(sparse) - min(sparse), 4),
            "sparse_faster_in_every_pair": all(s < x for s, x in zip(sparse, dense))}
    envs.check()
    fwd.check()
    envs.close()
    fwd.close()
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sizes", type=int, nargs="+", default=[7, 9])
    ap.add_argument("--lattices", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--timeout", type=int, default=400, help="seconds per (size, lattices)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_sparse_bench.json"))
    ap.add_argument("--case", type=int, nargs=2, metavar=("D", "N"), help="(internal) run one case in this process and print its JSON")
    a = ap.parse_args()
    if a.case:
        print(json.dumps(one_case(a.case[0], a.case[1], a.pairs, a.reps, a.warmup)))
        return
    res = {"pairs": a.pairs, "reps": a.reps, "warmup": a.warmup, "play_steps": PLAY_STEPS, "stack": "u8", "cases": []}
    for d in a.sizes:
        for n in a.lattices:
            cmd = [sys.executable, os.path.abspath(__file__), "--case", str(d), str(n), "--pairs", str(a.pairs), "--reps", str(a.reps),
                   "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
            if p.returncode != 0:
                print("d=%d, %d lattices failed with exit status %d: stopping" % (d, n, p.returncode), file=sys.stderr)
                sys.exit(1)
            case = json.loads(p.stdout.decode().strip().splitlines()[-1])
            res["device"] = case.pop("device")
            res["cases"].append(case)
            print("d=%d, %d lattices: done" % (d, n), file=sys.stderr, flush=True)
    sched = [c["settings"]["reference_schedule"] for c in res["cases"]]
    res["sparse_faster_in_every_pair_at_the_reference_schedule"] = all(s["sparse_faster_in_every_pair"] for s in sched)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
