#!/usr/bin/env python3
"""What the two events per step of T.ExploreLoop cost on the write's stream (MI355X): the loop timed (wall clock over
200 steps, the stack write's own time from every 8th step's events subtracted) with the cross-stream events left out
one by one, and with "write(t) is done" recorded behind the write (`*_record`) instead of signalled by its dispatch.  Leaving one out breaks the ORDER the loop needs (results are not checked here): this is a cost table only.
Usage (GPU box): python tools/overlap_cost.py [lattices=65536] [d=7] [reps=4] [modes, comma separated]"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import toric_rl_decoder_amd as T  # noqa: E402


class CostLoop(T.ExploreLoop):
    """ExploreLoop.step with the two cross-stream orderings switchable (a cost experiment: the results are NOT valid
    without them)."""
    wait_on_A = True       # stream A waits for scan(t) of stream B
    record_on_A = "bound"  # "write(t) done", which stream B waits for before step(t+1): "bound" = signalled by the write's own
                           # dispatch (the loop's way), "record" = an event recorded on stream A behind the write, False = left out

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.recorded = [torch.cuda.Event() for _ in range(2)]
        self.host_in_wait = []     # seconds the host spent inside each "stream B waits for write(t-1)" call

    def step(self, bracket=None):
        envs, t, k = self.envs, self.t, self.t & 1
        off = self._row(t)
        if self.overlap and self.wait_on_A == "host":
            self.scanned[k].synchronize()
        elif self.overlap and self.wait_on_A:
            self.A.wait_event(self.scanned[k])
        if bracket is not None:
            bracket[0].record(self.A)
        envs.writePerspectives(self.stack, self.positions, off, done=self.written[k] if self.overlap and self.record_on_A == "bound" else None)
        if bracket is not None:
            bracket[1].record(self.A)
        if self.overlap and self.record_on_A == "record":
            self.recorded[k].record(self.A)
        with torch.cuda.stream(self.B):
            if self.overlap and t > 0 and self.record_on_A == "bound":
                h0 = time.perf_counter()
                self.written[k ^ 1].wait(self.B)
                self.host_in_wait.append(time.perf_counter() - h0)
            elif self.overlap and t > 0 and self.record_on_A == "record":
                self.B.wait_event(self.recorded[k ^ 1])
            blk = self.blocks[(t // self.flush) % len(self.blocks)]
            envs.actorStep(None, block=blk, slot=t % self.flush, want_actions=True)
            if (t + 1) % self.flush == 0:
                blk.computePriorities(envs.no_envs, self.flush, None, 0.95)
            envs.perspectiveCounts(self._row(t + 1))
            if self.overlap:
                self.scanned[k ^ 1].record(self.B)
        self.t = t + 1


def setup(n, d):
    """Lattices at a steady spread of episode ages, ONE stack buffer for every mode (the write rate belongs to the buffer)."""
    env = T.make("toric-code-v0", {"size": d, "p_error": 0.1})
    envs = T.EnvSet(env, n, seed=5, numpy_io=False)
    envs.resetAll()
    for t in range(76):
        idx = torch.arange(t, n, 76, dtype=torch.int32, device=envs.device)
        if idx.numel():
            envs.resetTerminalEnvs(idx)
        envs.actorStep(None, want_actions=False)
    nq = 2 * d * d
    stack = T.alloc_stack(n * nq, d, torch.float32, envs.device)
    pos = torch.empty((n * nq, 3), dtype=torch.int32, device=envs.device)
    offs = torch.zeros((8, (n + 2) & ~1), dtype=torch.int64, device=envs.device)
    blocks = [envs.newTransitionBlock(steps=8) for _ in range(2)]
    return envs, stack, pos, offs, blocks


def run(ctx, mode, steps=200):
    envs, stack, pos, offs, blocks = ctx
    loop = CostLoop(envs, stack, pos, offs, blocks=blocks, flush=8, overlap=mode != "serial", pace="device")
    loop.wait_on_A = "host" if mode.startswith("host_wait") else mode not in ("no_wait_on_A", "no_events")
    loop.record_on_A = False if mode in ("no_record_on_A", "no_events") else ("record" if mode.endswith("_record") else "bound")
    for _ in range(20):
        loop.step()
    loop.drain()
    torch.cuda.synchronize()
    evs = []
    t0 = time.perf_counter()
    for i in range(steps):
        if i % 8 == 0:
            e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            evs.append(e)
            loop.step(e)
        else:
            loop.step()
    loop.drain()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    w = float(np.mean([a.elapsed_time(b) for a, b in evs]))
    hw = loop.host_in_wait[-steps:]
    return 1e3 * dt, w, (1e6 * float(np.mean(hw)), 1e6 * float(np.max(hw))) if hw else None


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
    d = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    modes = sys.argv[4].split(",") if len(sys.argv) > 4 else ["serial", "overlap", "overlap_record", "host_wait", "host_wait_record"]
    print(f"{n} lattices, d={d}, one buffer, modes in turn: ms per step, stack write ms (events, every 8th step), difference in us")
    ctx = setup(n, d)
    for rep in range(reps):
        for mode in modes:
            step_ms, write_ms, hw = run(ctx, mode)
            print(f"  {mode:16s} {step_ms:.4f}  {write_ms:.4f}  {1e3 * (step_ms - write_ms):6.1f}"
                  + ("   host in the wait call: mean %.1f us, max %.1f" % hw if hw else ""), flush=True)
    ctx[0].check()
    ctx[0].close()


if __name__ == "__main__":
    main()
