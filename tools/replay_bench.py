#!/usr/bin/env python3
"""Replay memory timings -> one JSON line (profiles/README.md).

Device part (default): HIP-event times of the device replay memory after a warm-up --
  * ingest: save_block of one 65 536 x 8-slot block (every slot a transition) at d=7 and d=9, capacity 10^6;
  * sample_batch latency at capacity 10^6 (filled) for B = 16, 256, 1024 (sample + records + faithful revert);
  * update_priorities latency for the same B.
Host part (--host REFERENCE_DIR): the reference's own PrioritizedReplayMemory (src/ReplayMemory.py) on the CPU, one
process: save rate, and sample(B) + priority_update rate, at capacity 10^6; --merge FILE adds the device line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_part(reps, warmup):
    import torch
    import toric_rl_decoder_amd as T
    from toric_rl_decoder_amd import wire

    dev = "cuda:0"
    cap, n_slots = 10 ** 6, 65536 * 8

    def block(d, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        buf = torch.randint(0, 256, (wire.block_bytes(d, n_slots),), dtype=torch.uint8, device=dev, generator=g)
        s = wire.sections(d, n_slots)
        off = s["action"][0]
        a = torch.randint(1, 4, (n_slots,), dtype=torch.int32, device=dev, generator=g) << 24
        buf[off:off + 4 * n_slots].view(torch.int32).copy_(a)
        off = s["priority"][0]
        buf[off:off + 4 * n_slots].view(torch.float32).uniform_(0.01, 10.0, generator=g)
        return buf

    def timed(fn, n):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        for _ in range(n):
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            out.append(t0.elapsed_time(t1))
        out.sort()
        return {"median_ms": round(out[len(out) // 2], 5), "min_ms": round(out[0], 5)}

    res = {"capacity": cap, "ingest_slots": n_slots, "reps": reps, "warmup": warmup, "device": torch.cuda.get_device_name(0)}
    for d in (7, 9):
        mem = T.PrioritizedReplayMemory(cap, 0.6, d=d, device=dev, seed=1)
        b = block(d, d)
        res[f"ingest_d{d}"] = timed(lambda: mem.save_block(b), reps)
        res[f"ingest_d{d}"]["block_bytes"] = int(b.numel())
        mem.check()
        if d == 7:
            assert mem.filled_size() == cap
            for B in (16, 256, 1024):
                res[f"sample_batch_B{B}"] = timed(lambda: mem.sample_batch(B, 0.4), reps)
                idx = mem.sample_batch(B, 0.4)[6]
                pr = torch.rand(B, device=dev, dtype=torch.float64)
                res[f"update_B{B}"] = timed(lambda: mem.update_priorities(idx, pr), reps)
            mem.check()
        mem.close()
        del b
    return res


def host_part(ref, seconds):
    import random
    sys.path.insert(0, ref)
    import src.ReplayMemory as RM

    cap = 10 ** 6
    mem = RM.PrioritizedReplayMemory(cap, 0.6)
    rng = random.Random(1)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(1000):
            mem.save(n, rng.uniform(0.01, 10.0))
            n += 1
    save_rate = n / (time.perf_counter() - t0)
    out = {"host_cpus": os.cpu_count(), "host_process_threads": 1, "host_capacity": cap, "host_filled": mem.filled_size(),
           "host_save_per_s": round(save_rate, 1)}
    for B in (16, 256, 1024):
        k, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            _, _, idx, _ = mem.sample(B, 0.4)
            mem.priority_update(idx, [rng.uniform(0.01, 10.0) for _ in idx])
            k += 1
        dt = (time.perf_counter() - t0) / k
        out[f"host_sample_update_B{B}_ms"] = round(1e3 * dt, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host", metavar="REFERENCE_DIR", help="time the reference's host replay memory instead")
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--merge", metavar="FILE", help="with --host: a device line to merge into")
    a = ap.parse_args()
    if a.host:
        res = json.load(open(a.merge)) if a.merge else {}
        res.update(host_part(a.host, a.seconds))
    else:
        res = device_part(a.reps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
