#!/usr/bin/env python3
"""NN_8 / NN_17 learner step: stock torch against the hand-written HIP step -> profiles/nnw_grad_bench.json.

After tools/nn_grad_bench.py.  For each net, d = 7 and d = 9 and batches of 32, 256 and 4096 records (perspectives from
eps = 1 play, random actions, targets and importance weights; seeded He-normal weights, as no trained NN_8 / NN_17
checkpoint exists), one gradient step with torch's Adam on the f32 master parameters:
  old  torch f32 forward + loss + backward + step, and the same under bf16 autocast, after their warm-up (MIOpen picks
       its kernels there);
  new  policy.NNWideGrad.backward (tq_nnw_grad_step) + step + NNWideGrad.load().
Every path has its own copy of the weights and its own optimizer.  Old and new alternate in pairs; each pair takes the
median of its calls after warm-ups, timed by HIP events.  Per path: ms per step, records/s and the spread of the pair
medians; per batch size the ratios torch / NNWideGrad (above 1: the new step is faster).  Nothing is gated: the figures
are reported as they come out, slower cases included.

Each (net, size) runs in a process of its own under a time limit; the first one that fails stops the run.  The output
file is rewritten after every (net, size), so a run that is stopped keeps what it measured.  On an MI355X a size of
NN_8 took about 200 s and NN_17 at d = 7 more than 260 s (--timeout).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (32, 256, 4096)
NETS = (8, 17)
SIZES = (7, 9)


def one_size(net, d, pairs, reps, warmup):
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

    cls = {8: T.NN_8, 17: T.NN_17}[net]

    def fresh():
        m = cls(d, 3).to(dev).train()
        g = torch.Generator().manual_seed(100 * net + d)
        with torch.no_grad():
            for name, p in m.named_parameters():
                if name.endswith("weight"):
                    fan = p[0].numel()
                    p.copy_(torch.randn(p.shape, generator=g) * ((2.0 if p.dim() == 4 else 1.0) / fan) ** 0.5)
                else:
                    p.copy_(torch.randn(p.shape, generator=g) * 0.01)
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
        grad = T.NNWideGrad(mnn, d, dev, max_batch=B)

        def torch_step(m, o, autocast):
            o.zero_grad(set_to_none=False)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                q = m(s).float().gather(1, a.view(-1, 1)).squeeze(1)
            (ww * (yy - q) ** 2).mean().backward()
            o.step()

        def nnw_step():
            grad.backward(s, a, yy, ww)
            onn.step()
            grad.load()

        paths = {"torch_f32": lambda: torch_step(m32, o32, False), "torch_bf16_autocast": lambda: torch_step(mbf, obf, True),
                 "nnw_grad": nnw_step}
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
        r["torch_bf16_over_nnw_grad"] = round(r["paths"]["torch_bf16_autocast"]["ms_per_step"] / r["paths"]["nnw_grad"]["ms_per_step"], 3)
        r["torch_f32_over_nnw_grad"] = round(r["paths"]["torch_f32"]["ms_per_step"] / r["paths"]["nnw_grad"]["ms_per_step"], 3)
        r["nnw_grad_faster_than_bf16_in_every_pair"] = all(x < z for x, z in zip(times["nnw_grad"], times["torch_bf16_autocast"]))
        res["batches"]["b%d" % B] = r
    res["device"] = torch.cuda.get_device_name(0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nets", type=int, nargs="+", default=list(NETS), choices=NETS)
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--timeout", type=int, default=600, help="seconds per (net, size)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nnw_grad_bench.json"))
    ap.add_argument("--size", type=int, help="(internal) run one size of --nets' first net in this process and print its JSON")
    a = ap.parse_args()
    if a.size:
        print(json.dumps(one_size(a.nets[0], a.size, a.pairs, a.reps, a.warmup)))
        return
    res = {"pairs": a.pairs, "reps": a.reps, "warmup": a.warmup, "optimizer": "Adam", "weights": "seeded He-normal", "nets": {}}
    for net in a.nets:
        res["nets"]["nn%d" % net] = {}
        for d in a.sizes:
            cmd = [sys.executable, os.path.abspath(__file__), "--nets", str(net), "--size", str(d), "--pairs", str(a.pairs),
                   "--reps", str(a.reps), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
            if p.returncode != 0:
                print("net %d d=%d failed with exit status %d: stopping" % (net, d, p.returncode), file=sys.stderr)
                sys.exit(1)
            one = json.loads(p.stdout.decode().strip().splitlines()[-1])
            res["device"] = one.pop("device")
            res["nets"]["nn%d" % net]["d%d" % d] = one
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
            print("net %d d=%d done" % (net, d), file=sys.stderr, flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
