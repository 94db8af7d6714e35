#!/usr/bin/env python3
"""NN_11 optimizer step: torch's optimizer + re-pack against the one-launch HIP step -> profiles/nn11_opt_bench.json.

For d = 7 and d = 9 and batches of 32, 256 and 4096 records (perspectives from eps = 1 play, random actions, targets and
importance weights), with Adam at lr 0.00025:
  tail   old  torch.optim.Adam(...).step() (torch's default implementation) + NN11Grad.load(): what learnerStep ran
              before NN11Optimizer;
         new  NN11Optimizer.step() (tq_nn11_grad_opt_step), which re-packs itself;
  step   NN11Grad.backward followed by that tail, old and new.
The whole step is timed again with RMSprop at d = 7, 256 records.  Every path has its own copy of the trained weights,
its own handle and its own optimizer.  Old and new alternate in seven pairs; each pair takes the median of its calls
after warm-ups, timed by HIP events.  Per path: ms per call and the spread of the seven medians; per case the ratio
old / new (above 1: the new path is faster) and whether new was faster in every pair.  Nothing is gated: the figures
are reported as they come out.

Each size runs in a process of its own under a time limit; the first one that fails stops the run.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (32, 256, 4096)
LR = 0.00025
RMSPROP_AT = (7, 256)


def one_size(d, pairs, reps, warmup):
    import torch
    import toric_rl_decoder_amd as T

    dev = "cuda:0"
    envs = T.EnvSet(T.make("toric-code-v0", {"size": d, "min_qubit_errors": 0, "p_error": 0.1}), 1024, device=dev, seed=d,
                    numpy_io=False)
    envs.resetAll()
    for _ in range(4):                                         # eps = 1 play
        envs.actorStep(None)
    per, _, _ = envs.generatePerspective(dtype=torch.float32)
    assert per.shape[0] >= max(BATCHES), per.shape
    per = per[:max(BATCHES)].clone()
    envs.check()
    envs.close()

    path = os.path.join(ROOT, "tests", "golden", "nn11_d%d_converged.safetensors" % d)
    sd = None
    if os.path.exists(path):
        from safetensors.torch import load_file
        sd = load_file(path)

    def fresh(B, kind, new):
        torch.manual_seed(0)
        m = T.NN_11(d, 3).to(dev).train()
        if sd is not None:
            m.load_state_dict(sd)
        grad = T.NN11Grad(m, d, dev, max_batch=B)
        if new:
            return grad, T.NN11Optimizer(grad, kind, lr=LR)
        return grad, (torch.optim.Adam if kind == "Adam" else torch.optim.RMSprop)(m.parameters(), lr=LR)

    g = torch.Generator(device=dev).manual_seed(d)
    actions = torch.randint(0, 3, (max(BATCHES),), generator=g, device=dev)
    y = torch.rand(max(BATCHES), generator=g, device=dev) * 20 - 10
    w = torch.rand(max(BATCHES), generator=g, device=dev) * 0.9 + 0.1

    def median_ms(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        for _ in range(reps):
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            out.append(t0.elapsed_time(t1))
        out.sort()
        return out[len(out) // 2]

    def measure(B, kind, whole):
        s, a, yy, ww = per[:B], actions[:B], y[:B], w[:B]
        old_grad, old_opt = fresh(B, kind, False)
        new_grad, new_opt = fresh(B, kind, True)

        def old():
            if whole:
                old_grad.backward(s, a, yy, ww)
            old_opt.step()
            old_grad.load()

        def new():
            if whole:
                new_grad.backward(s, a, yy, ww)
            new_opt.step()

        for grad in (old_grad, new_grad):                      # the .grad tensors that a tail alone steps on
            grad.backward(s, a, yy, ww)
        paths = {"old": old, "new": new}
        for fn in paths.values():                              # the optimizer's state
            fn()
        times = {k: [] for k in paths}
        for _ in range(pairs):
            for k, fn in paths.items():
                times[k].append(median_ms(fn))
        for grad in (old_grad, new_grad):
            grad.check()
            grad.close()
        r = {}
        for k, ts in times.items():
            m = sorted(ts)[pairs // 2]
            r[k] = {"pair_medians_ms": [round(x, 4) for x in ts], "ms": round(m, 4), "spread_ms": round(max(ts) - min(ts), 4)}
        r["old_over_new"] = round(r["old"]["ms"] / r["new"]["ms"], 3)
        r["new_faster_in_every_pair"] = all(x < z for x, z in zip(times["new"], times["old"]))
        return r

    res = {"batches": {}}
    for B in BATCHES:
        res["batches"]["b%d" % B] = {"tail_adam": measure(B, "Adam", False), "step_adam": measure(B, "Adam", True)}
        if (d, B) == RMSPROP_AT:
            res["batches"]["b%d" % B]["step_rmsprop"] = measure(B, "RMSprop", True)
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=280, help="seconds per size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn11_opt_bench.json"))
    ap.add_argument("--size", type=int, help="(internal) run one size in this process and print its JSON")
    a = ap.parse_args()
    if a.size:
        print(json.dumps(one_size(a.size, a.pairs, a.reps, a.warmup)))
        return
    res = {"pairs": a.pairs, "reps": a.reps, "warmup": a.warmup, "lr": LR, "sizes": {}}
    for d in (7, 9):
        cmd = [sys.executable, os.path.abspath(__file__), "--size", str(d), "--pairs", str(a.pairs), "--reps", str(a.reps),
               "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
        if p.returncode != 0:
            print("d=%d failed with exit status %d: stopping" % (d, p.returncode), file=sys.stderr)
            sys.exit(1)
        res["sizes"]["d%d" % d] = json.loads(p.stdout.decode().strip().splitlines()[-1])
        res["device"] = res["sizes"]["d%d" % d].pop("device")
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
