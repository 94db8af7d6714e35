#!/usr/bin/env python3
"""NN_11 forward: stock torch against the hand-written HIP forward -> profiles/nn11_forward_bench.json.

For d = 7 and d = 9, one chunk of 65 536 perspectives from eps = 1 play:
  old  torch f32 on the f32 stack, and torch bf16 autocast on the bf16 stack, both through policy._forward_chunked at
       one fixed shape (bench.py's 16 384-row calls), after its warm-up (MIOpen picks its kernels there);
  new  policy.NN11Forward (tq_nn11_forward) on the u8 stack and on the bf16 stack.
Old and new alternate in seven pairs; each pair takes the median of its calls after warm-ups, timed by HIP events.
Per path: ms per chunk, perspectives/s, TFLOP/s by bench.py's FLOP count for this network, the fraction of the part's
2.5 PFLOP/s bf16 matrix rate, and the spread of the seven medians.  `accepted`: the new forward on the bf16 stack was
faster than torch bf16 autocast in each of the seven pairs at both sizes.

Each size runs in a process of its own under a time limit; the first one that fails stops the run.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = 65536
OLD_CHUNK = 16384
PEAK_BF16 = 2.5e15           # 1024 SIMDs x 1024 FLOP/cycle x 2.4 GHz
CH = (2, 128, 128, 120, 111, 104, 103, 90, 80, 73, 71, 64)


def flop_per_persp(d):       # bench.py's count: the eleven convolutions
    return 2.0 * sum(CH[i] * CH[i + 1] * 9 * ((d - 2) ** 2 if i == 10 else d * d) for i in range(11))


def one_size(d, pairs, reps, warmup, max_rows):
    import torch
    import toric_rl_decoder_amd as T
    from toric_rl_decoder_amd.policy import _forward_chunked

    dev = "cuda:0"
    n = 4096
    envs = T.EnvSet(T.make("toric-code-v0", {"size": d, "min_qubit_errors": 0, "p_error": 0.1}), n, device=dev, seed=d,
                    numpy_io=False)
    envs.resetAll()
    for _ in range(4):                                         # eps = 1 play
        envs.actorStep(None)
    stacks = {}
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16), ("u8", torch.uint8)):
        per, _, _ = envs.generatePerspective(dtype=dt)
        assert per.shape[0] >= ROWS, per.shape
        stacks[name] = per[:ROWS].clone()
    envs.check()
    envs.close()

    path = os.path.join(ROOT, "tests", "golden", "nn11_d%d_converged.safetensors" % d)
    torch.manual_seed(0)
    model = T.NN_11(d, 3).to(dev).eval()
    if os.path.exists(path):
        from safetensors.torch import load_file
        model.load_state_dict(load_file(path))
    fwd = T.NN11Forward(model, d, dev, max_rows=max_rows)
    q_buf = torch.empty((ROWS, 3), dtype=torch.float32, device=dev)

    def old_f32():
        return _forward_chunked(model, stacks["f32"], OLD_CHUNK, pad_to=OLD_CHUNK, out=q_buf)

    def old_bf16():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return _forward_chunked(model, stacks["bf16"], OLD_CHUNK, pad_to=OLD_CHUNK, out=q_buf)

    paths = {"torch_f32": old_f32, "torch_bf16_autocast": old_bf16, "nn11_u8": lambda: fwd(stacks["u8"]),
             "nn11_bf16": lambda: fwd(stacks["bf16"])}

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
    qn = fwd(stacks["bf16"])
    assert torch.equal(qn, fwd(stacks["u8"]))
    err = {"nn11_rms_vs_f32": float((qn - q32).double().pow(2).mean().sqrt()),
           "autocast_rms_vs_f32": float((qbf - q32).double().pow(2).mean().sqrt())}
    times = {k: [] for k in paths}
    for _ in range(pairs):
        for k, fn in paths.items():                            # old, old, new, new: one pair
            times[k].append(median_ms(fn))
    res = {"rows": ROWS, "flop_per_perspective": flop_per_persp(d), "max_rows": max_rows, **err, "paths": {}}
    for k, ts in times.items():
        m = sorted(ts)[pairs // 2]
        tf = ROWS * flop_per_persp(d) / (m * 1e-3) / 1e12
        res["paths"][k] = {"pair_medians_ms": [round(x, 4) for x in ts], "ms_per_chunk": round(m, 4),
                           "perspectives_per_s": round(ROWS / (m * 1e-3), 1), "tflops": round(tf, 2),
                           "fraction_of_bf16_peak": round(tf * 1e12 / PEAK_BF16, 4), "spread_ms": round(max(ts) - min(ts), 4)}
    res["nn11_bf16_faster_in_every_pair"] = all(a < b for a, b in zip(times["nn11_bf16"], times["torch_bf16_autocast"]))
    res["torch_bf16_over_nn11_bf16"] = round(res["paths"]["torch_bf16_autocast"]["ms_per_chunk"] / res["paths"]["nn11_bf16"]["ms_per_chunk"], 3)
    res["device"] = torch.cuda.get_device_name(0)
    fwd.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-rows", type=int, default=1 << 16, help="rows per pass of the NN11Forward handle")
    ap.add_argument("--timeout", type=int, default=400, help="seconds per size")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nn11_forward_bench.json"))
    ap.add_argument("--size", type=int, help="(internal) run one size in this process and print its JSON")
    a = ap.parse_args()
    if a.size:
        print(json.dumps(one_size(a.size, a.pairs, a.reps, a.warmup, a.max_rows)))
        return
    res = {"pairs": a.pairs, "reps": a.reps, "warmup": a.warmup, "old_chunk": OLD_CHUNK, "peak_bf16_flops": PEAK_BF16, "sizes": {}}
    for d in (7, 9):
        cmd = [sys.executable, os.path.abspath(__file__), "--size", str(d), "--pairs", str(a.pairs), "--reps", str(a.reps),
               "--warmup", str(a.warmup), "--max-rows", str(a.max_rows)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.timeout)
        if p.returncode != 0:
            print("d=%d failed with exit status %d: stopping" % (d, p.returncode), file=sys.stderr)
            sys.exit(1)
        res["sizes"]["d%d" % d] = json.loads(p.stdout.decode().strip().splitlines()[-1])
        res["device"] = res["sizes"]["d%d" % d].pop("device")
    res["accepted"] = all(s["nn11_bf16_faster_in_every_pair"] for s in res["sizes"].values())
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    sys.exit(0 if res["accepted"] else 1)


if __name__ == "__main__":
    main()
