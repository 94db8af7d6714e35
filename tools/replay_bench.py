#!/usr/bin/env python3
"""Replay memory timings -> one JSON line (profiles/README.md).

Device part (default): HIP-event times of the device replay memory after a warm-up --
  * ingest: save_block of one 65 536 x 8-slot block (every slot a transition) at d=7 and d=9, capacity 10^6;
  * sample_batch latency at capacity 10^6 (filled) for B = 16, 256, 1024 (sample + records + faithful revert);
  * update_priorities latency for the same B.
  --lib SO: with another build of libtoricenv.so (a parent commit's, for an A/B in alternating processes).
Targets leg (--targets): the learner's target side at capacity 10^6 (actor-written records), B = 32, 256, 1024 and
d = 7, 9, old path against new, each the median of 200 calls after 20 warm-ups, timed alternately in seven pairs --
  * old: sample_batch's f32 next_state -> generatePerspectiveBatch -> segment_max + the torch target expression;
  * new: next_perspectives(indices) -> td_target, on the same random Q-table;
  and the kernel launches of each, counted from the code (profiles/replay_targets_bench.json).
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


# kernel launches of one call of each path of the targets leg, read off the code (the 8-byte read-back of P is a copy)
OLD_LAUNCHES = ["f32 -> u8 cast (torch)", "k_pack_states", "k_scan_partials", "k_scan_final", "k_pack_states",
                "k_persp_stream", "counts.max (torch)", "clamp (torch)", "to int32 (torch)", "k_segment_max",
                "~terminal (torch)", "to float (torch)", "* discount (torch)", "* target (torch)", "reward + (torch)",
                "clamp (torch)"]
NEW_LAUNCHES = ["k_replay_next_planes", "k_scan_final", "k_replay_next_planes", "k_persp_stream", "k_td_target"]


def targets_part(reps=200, warmup=20, pairs=7):
    import torch
    import toric_rl_decoder_amd as T

    dev = "cuda:0"
    cap, n_envs, steps = 10 ** 6, 65536, 8

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

    res = {"capacity": cap, "reps": reps, "warmup": warmup, "pairs": pairs, "device": torch.cuda.get_device_name(0),
           "launches_old": len(OLD_LAUNCHES), "launches_new": len(NEW_LAUNCHES), "launches_old_list": OLD_LAUNCHES,
           "launches_new_list": NEW_LAUNCHES, "points": {}}
    ok = True
    for d in (7, 9):
        mem = T.PrioritizedReplayMemory(cap, 0.6, d=d, device=dev, seed=1)
        env = T.make("toric-code-v0", {"size": d, "min_qubit_errors": 0, "p_error": 0.1})
        gpu = T.EnvSet(env, n_envs, device=dev, seed=d, numpy_io=False)
        gpu.resetAll()
        blk = gpu.newTransitionBlock(steps=steps)
        for _ in range(2):                                 # 2 x 524 288 records fill the 10^6
            for t in range(steps):
                gpu.actorStep(None, block=blk, slot=t)
            blk.computePriorities(n_envs, steps, torch.rand((steps + 1, n_envs, 3), device=dev), 0.95)
            mem.save_block(blk)
        gpu.check()
        gpu.close()
        assert mem.filled_size() == cap
        for B in (32, 256, 1024):
            _, _, reward, next_state, terminal, _, idx = mem.sample_batch(B, 0.4)
            P = int(mem.next_perspectives(idx)[3][-1])
            q = torch.randn((P, 3), device=dev)

            def old():
                _, _, counts, offsets = T.generatePerspectiveBatch(d // 2, d, next_state, device=dev, return_offsets=True)
                largest = torch.clamp(counts.max(), min=1).to(torch.int32).reshape(1)
                target = T.segment_max(q, offsets, largest)
                return (reward + (~terminal).type(torch.float) * 0.95 * target).clamp(-100, 100)

            def new():
                _, _, _, offsets = mem.next_perspectives(idx)
                return T.td_target(q, offsets, reward, terminal, 0.95)

            assert torch.equal(old(), new())
            t_old, t_new = [], []
            for _ in range(pairs):
                t_old.append(median_ms(old))
                t_new.append(median_ms(new))
            m_old, m_new = sorted(t_old)[pairs // 2], sorted(t_new)[pairs // 2]
            spread = max(t_old) - min(t_old)
            accepted = m_new <= m_old + spread
            ok &= accepted
            res["points"][f"d{d}_B{B}"] = {"perspectives": P, "old_ms": [round(x, 5) for x in t_old],
                                           "new_ms": [round(x, 5) for x in t_new], "old_median_ms": round(m_old, 5),
                                           "new_median_ms": round(m_new, 5), "old_spread_ms": round(spread, 5),
                                           "new_over_old": round(m_new / m_old, 4), "accepted": bool(accepted)}
        mem.check()
        mem.close()
    res["accepted"] = bool(ok)
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
    ap.add_argument("--targets", action="store_true", help="the learner-target leg: old data path against new")
    ap.add_argument("--host", metavar="REFERENCE_DIR", help="time the reference's host replay memory instead")
    ap.add_argument("--seconds", type=float, default=5.0)
    ap.add_argument("--merge", metavar="FILE", help="with --host: a device line to merge into")
    ap.add_argument("--lib", metavar="SO", help="load this libtoricenv.so (another commit's build) instead of the tree's")
    a = ap.parse_args()
    if a.lib:
        from toric_rl_decoder_amd import _lib
        _lib.LIB_PATH = os.path.abspath(a.lib)
    if a.targets:
        res = targets_part()
        print(json.dumps(res))
        sys.exit(0 if res["accepted"] else 1)
    if a.host:
        res = json.load(open(a.merge)) if a.merge else {}
        res.update(host_part(a.host, a.seconds))
    else:
        res = device_part(a.reps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
