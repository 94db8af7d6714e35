#!/usr/bin/env python3
"""ResNet18 eval-mode forward: stock torch against the hand-written HIP forward -> profiles/resnet_forward_bench.json.

For d = 7 and d = 9, the reference launcher's sizes, one chunk of 16 384 perspectives from eps = 1 play:
  old  torch f32 on the f32 stack, and torch bf16 autocast on the bf16 stack, both through policy._forward_chunked at
       one fixed shape, after its warm-up (MIOpen picks its kernels there), the module in eval mode;
  new  policy.ResNetForward (tq_resnet_forward) on the bf16 stack, through the same _forward_chunked.
Old and new alternate in seven pairs; each pair takes the median of its calls after warm-ups, timed by HIP events.
Per path: ms per chunk, perspectives/s, TFLOP/s by the convolutions' FLOP count, the fraction of the part's 2.5 PFLOP/s
bf16 matrix rate, and the spread of the seven medians.  The baseline is torch; nothing is gated on these numbers.
Weights: seeded He-normal with random, sane BatchNorm statistics (no trained ResNet checkpoint exists); timing does not
depend on them.

Each (net, size) runs in a process of its own under a time limit; the first one that fails stops the run.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = 16384
PEAK_BF16 = 2.5e15           # 1024 SIMDs x 1024 FLOP/cycle x 2.4 GHz


def flop_per_persp(net, d):  # the convolutions: layer4 writes the half grid of side (d + 1) / 2
    from toric_rl_decoder_amd.resnet import convs
    half = ((d + 1) // 2) ** 2
    return 2.0 * sum(co * ci * kh * kw * (half if name.startswith("layer4") else d * d) for name, _, (co, ci, kh, kw) in convs(net))


def one(net, d, pairs, reps, warmup, max_rows):
    import torch
    import toric_rl_decoder_amd as T
    from toric_rl_decoder_amd.policy import _forward_chunked

    dev = "cuda:0"
    envs = T.EnvSet(T.make("toric-code-v0", {"size": d, "min_qubit_errors": 0, "p_error": 0.1}), 2048, device=dev, seed=d,
                    numpy_io=False)
    envs.resetAll()
    for _ in range(4):                                         # eps = 1 play
        envs.actorStep(None)
    stacks = {}
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        per, _, _ = envs.generatePerspective(dtype=dt)
        assert per.shape[0] >= ROWS, per.shape
        stacks[name] = per[:ROWS].clone()
    envs.check()
    envs.close()

    cls = {18: T.ResNet18, 34: T.ResNet34}[net]
    model = cls().to(dev).eval()
    g = torch.Generator().manual_seed(100 * net + d)
    with torch.no_grad():
        for name, p in model.state_dict().items():
            if p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / p[0].numel()) ** 0.5)
            elif name == "linear.weight":
                p.copy_(torch.randn(p.shape, generator=g) * (1.0 / p[0].numel()) ** 0.5)
            elif name.endswith("running_var"):
                p.copy_(0.5 + 1.5 * torch.rand(p.shape, generator=g))
            elif name.endswith("num_batches_tracked"):
                continue
            elif name.endswith("weight"):                       # a BatchNorm's gamma
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            else:                                               # beta, running_mean, linear.bias
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    fwd = T.ResNetForward(model, d, dev, max_rows=max_rows)
    q_buf = torch.empty((ROWS, 3), dtype=torch.float32, device=dev)

    def old_f32():
        return _forward_chunked(model, stacks["f32"], ROWS, pad_to=ROWS, out=q_buf)

    def old_bf16():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return _forward_chunked(model, stacks["bf16"], ROWS, pad_to=ROWS, out=q_buf)

    def new_bf16():
        return _forward_chunked(fwd, stacks["bf16"], ROWS, out=q_buf)

    paths = {"torch_f32": old_f32, "torch_bf16_autocast": old_bf16, "resnet_bf16": new_bf16}

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

    q32 = old_f32().clone()                                    # also MIOpen's warm-up of both torch paths
    qbf = old_bf16().clone()
    qn = new_bf16().clone()
    rms = lambda a: float((a - q32).double().pow(2).mean().sqrt())
    err = {"resnet_rms_vs_f32": rms(qn), "autocast_rms_vs_f32": rms(qbf), "q_rms": float(q32.double().pow(2).mean().sqrt())}
    times = {k: [] for k in paths}
    for _ in range(pairs):
        for k, fn in paths.items():                            # old, old, new: one pair
            times[k].append(median_ms(fn))
    flop = flop_per_persp(net, d)
    res = {"net": "ResNet%d" % net, "d": d, "rows": ROWS, "flop_per_perspective": flop, "max_rows": max_rows, **err, "paths": {}}
    for k, ts in times.items():
        m = sorted(ts)[pairs // 2]
        tf = ROWS * flop / (m * 1e-3) / 1e12
        res["paths"][k] = {"pair_medians_ms": [round(x, 4) for x in ts], "ms_per_chunk": round(m, 4),
                           "perspectives_per_s": round(ROWS / (m * 1e-3), 1), "tflops": round(tf, 2),
                           "fraction_of_bf16_peak": round(tf * 1e12 / PEAK_BF16, 4), "spread_ms": round(max(ts) - min(ts), 4)}
    med = lambda k: res["paths"][k]["ms_per_chunk"]
    res["torch_f32_over_resnet"] = round(med("torch_f32") / med("resnet_bf16"), 3)
    res["torch_bf16_over_resnet"] = round(med("torch_bf16_autocast") / med("resnet_bf16"), 3)
    res["resnet_faster_than_autocast_in_every_pair"] = all(a < b for a, b in zip(times["resnet_bf16"], times["torch_bf16_autocast"]))
    res["device"] = torch.cuda.get_device_name(0)
    fwd.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-rows", type=int, default=1 << 12, help="rows per pass of the ResNetForward handle")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per (net, size)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resnet_forward_bench.json"))
    ap.add_argument("--one", nargs=2, type=int, metavar=("NET", "D"), help="(internal) run one case in this process and print its JSON")
    a = ap.parse_args()
    if a.one:
        print(json.dumps(one(a.one[0], a.one[1], a.pairs, a.reps, a.warmup, a.max_rows)))
        return
    res = {"pairs": a.pairs, "reps": a.reps, "warmup": a.warmup, "rows": ROWS, "peak_bf16_flops": PEAK_BF16, "cases": {}}
    for net in (18,):
        for d in (7, 9):
            cmd = [sys.executable, os.path.abspath(__file__), "--one", str(net), str(d), "--pairs", str(a.pairs), "--reps", str(a.reps),
                   "--warmup", str(a.warmup), "--max-rows", str(a.max_rows)]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                print("ResNet%d d=%d ran into its time limit: stopping" % (net, d), file=sys.stderr)
                sys.exit(1)
            if p.returncode != 0:
                print("ResNet%d d=%d failed with exit status %d: stopping" % (net, d, p.returncode), file=sys.stderr)
                sys.exit(1)
            r = json.loads(p.stdout.decode().strip().splitlines()[-1])
            res["device"] = r.pop("device")
            res["cases"]["ResNet%d_d%d" % (net, d)] = r
            print("ResNet%d d=%d: torch f32 %.2f ms, autocast %.2f ms, resnet %.2f ms" % (
                net, d, r["paths"]["torch_f32"]["ms_per_chunk"], r["paths"]["torch_bf16_autocast"]["ms_per_chunk"],
                r["paths"]["resnet_bf16"]["ms_per_chunk"]), file=sys.stderr, flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
