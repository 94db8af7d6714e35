#!/usr/bin/env python3
"""NN_11 learner step: stock torch against the hand-written HIP step -> profiles/nn11_grad_bench.json.

For d = 7 and d = 9 and batches of 32, 256 and 4096 records (perspectives from eps = 1 play, random actions, targets and
importance weights), one gradient step with Adam on the f32 master parameters:
  old  torch f32 forward + loss + backward + step, and the same under bf16 autocast, after their warm-up (MIOpen picks
       its kernels there);
  new  policy.NN11Grad.backward (tq_nn11_grad_step) + step + NN11Grad.load().
Every path has its own copy of the trained weights and its own optimizer.  Old and new alternate in seven pairs; each
pair takes the median of its calls after warm-ups, timed by HIP events.  Per path: ms per step, records/s and the spread
of the seven medians; per batch size the ratio torch bf16 autocast / NN11Grad (above 1: the new step is faster).  Nothing
is gated: the figures are reported as they come out.

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

    def fresh():
        torch.manual_seed(0)
        m = T.NN_11(d, 3).to(dev).train()
        if sd is not None:
            m.load_state_dict(sd)
        return m, torch.optim.Adam(m.parameters(), lr=1e-6)

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

    res = {"batches": {}}
    for B in BATCHES:
        s, a, yy, ww = per[:B], actions[:B], y[:B], w[:B]
        m32, o32 = fresh()
        mbf, obf = fresh()
        mnn, onn = fresh()
        grad = T.NN11Grad(mnn, d, dev, max_batch=B)

        def torch_step(m, o, autocast):
            o.zero_grad(set_to_none=False)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                q = m(s).float().gather(1, a.view(-1, 1)).squeeze(1)
            (ww * (yy - q) ** 2).mean().backward()
            o.step()

        def nn11_step():
            grad.backward(s, a, yy, ww)
            onn.step()
            grad.load()

        paths = {"torch_f32": lambda: torch_step(m32, o32, False), "torch_bf16_autocast": lambda: torch_step(mbf, obf, True),
                 "nn11_grad": nn11_step}
        for fn in paths.values():                              # MIOpen's warm-up, the .grad tensors, Adam's state
            fn()
        times = {k: [] for k in paths}
        for _ in range(pairs):
            for k, fn in paths.items():                        # old, old, new: one pair
                times[k].append(median_ms(fn))
        grad.check()
        grad.close()
        r = {"paths": {}}
        for k, ts in times.items():
            m = sorted(ts)[pairs // 2]
            r["paths"][k] = {"pair_medians_ms": [round(x, 4) for x in ts], "ms_per_step": round(m, 4),
                             "records_per_s": round(B / (m * 1e-3), 1), "spread_ms": round(max(ts) - min(ts), 4)}
        r["torch_bf16_over_nn11_grad"] = round(r["paths"]["torch_bf16_autocast"]["ms_per_step"] / r["paths"]["nn11_grad"]["ms_per_step"], 3)
        r["torch_f32_over_nn11_grad"] = round(r["paths"]["torch_f32"]["ms_per_step"] / r["paths"]["nn11_grad"]["ms_per_step"], 3)
        r["nn11_grad_faster_than_bf16_in_every_pair"] = all(x < z for x, z in zip(times["nn11_grad"], times["torch_bf16_autocast"]))
        res["batches"]["b%d" % B] = r
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=280, help="seconds per size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn11_grad_bench.json"))
    ap.add_argument("--size", type=int, help="(internal) run one size in this process and print its JSON")
    a = ap.parse_args()
    if a.size:
        print(json.dumps(one_size(a.size, a.pairs, a.reps, a.warmup)))
        return
    res = {"pairs": a.pairs, "reps": a.reps, "warmup": a.warmup, "optimizer": "Adam", "sizes": {}}
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
