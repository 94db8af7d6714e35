// What one step of the environment does to ONE lattice, written once for device and host builds.
//
// The kernels in kernels.hpp keep everything that is about threads (indexing, the loads and stores of the SoA
// planes, atomicOr on the error latch, the wave-cooperative reset) and call the functions below for everything that
// is about a lattice; a host build that includes this header runs the same statements on one lattice after the
// other.  The functions work on Lat<D>::State and plain values, touch memory only through a BlockView that is
// passed in, use no wave intrinsics and have no early return (k_actor_step keeps every lane alive to its end).
#pragma once
#include <stdint.h>

#include "lattice.hpp"

namespace tq {

enum { PL_X0 = 0, PL_X1 = 1, PL_Z0 = 2, PL_Z1 = 3, PL_V = 4, PL_P = 5 };
// bits of the error latch (32 is ERR_INTERNAL of stream_write.hpp)
enum { ERR_ACTION = 1, ERR_CAPACITY = 2, ERR_RESET_DUP = 4, ERR_RESET_ROUNDS = 8, ERR_INDEX = 16 };

// Position of the k-th set bit (k < popc) of the concatenated hit mask [E0 | E1] as a flat
// qubit index layer*DD + row*D + col -- the k-th entry of the reference's positions list.
template <int D>
TQ_HD int kth_hit(const typename Lat<D>::B& e0, const typename Lat<D>::B& e1, int k) {
    constexpr int W = Lat<D>::W;
    constexpr int DD = Lat<D>::DD;
    int base = 0;
    uint64_t word = 0;
    bool found = false;
#pragma unroll
    for (int l = 0; l < 2; ++l) {
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const uint64_t wv = l ? e1.w[j] : e0.w[j];
            const int c = popc64(wv);
            const bool here = !found && k < c;
            word = here ? wv : word;
            base = here ? l * DD + 64 * j : base;
            k = (found || here) ? k : k - c;
            found = found || here;
        }
    }
    // position of the k-th set bit of `word` (k < popc(word)): binary search on popcounts, six steps,
    // no data-dependent loop (a wave pays for its slowest lane)
    uint32_t w32 = (uint32_t)word;
    int posn = 0;
    {
        const int c = popc32(w32);
        const bool up = k >= c;
        k = up ? k - c : k; posn = up ? 32 : 0; w32 = up ? (uint32_t)(word >> 32) : w32;
    }
#pragma unroll
    for (int s = 16; s >= 1; s >>= 1) {
        const int c = popc32(w32 & ((1u << s) - 1u));
        const bool up = k >= c;
        k = up ? k - c : k; posn += up ? s : 0; w32 = up ? (w32 >> s) : w32;
    }
    return base + posn;
}

// validated decode of action = [layer,row,col,op]
template <int D>
TQ_HD bool action_ok(int layer, int row, int col, int op) {
    return ((unsigned)layer < 2u) & ((unsigned)row < (unsigned)D) & ((unsigned)col < (unsigned)D) &
           ((unsigned)(op - 1) < 3u);
}
// op == 0 is "no action" (what tq_select_action emits for a lattice without defects): the step is
// counted, nothing changes, and no error is latched.
TQ_HD bool action_noop(int op) { return op == 0; }

// Pure exploration (eps = 1), the non-greedy branch of _selectActionBatch_prime (numba/util_actor.py:97-98): a
// uniformly drawn defect-adjacent qubit and a uniform op.  False, and the no-op action, for a lattice without defects.
template <int D>
TQ_HD bool explore_action(const typename Lat<D>::B& v, const typename Lat<D>::B& p, uint64_t seed, uint32_t env,
                          uint32_t episode, uint32_t step, int& layer, int& row, int& col, int& op) {
    using L = Lat<D>;
    typename L::B e0, e1;
    L::hit_masks(v, p, e0, e1);
    const int n = e0.popc() + e1.popc();
    const bool ok = n > 0;
    layer = row = col = op = 0;
    if (ok) {
        const U4 w = draw(seed, env, episode, step, DOMAIN_SEL, 0);
        const int h = kth_hit<D>(e0, e1, (int)mulhi32(w.y, (uint32_t)n));
        layer = h >= L::DD;
        const int rem = h - layer * L::DD;
        row = rem / D; col = rem - row * D;
        op = 1 + (int)mulhi32(w.z, 3);
    }
    return ok;
}

// env.step on one lattice: the action (if `ok`; otherwise nothing changes), the new syndrome, the reward.
// Returns the terminal flag.
template <int D>
TQ_HD int step_lattice(typename Lat<D>::State& s, bool ok, int layer, int row, int col, int op, float terminal_reward,
                       float& reward) {
    using L = Lat<D>;
    const int before = s.v.popc() + s.p.popc();
    if (ok) L::apply(s, layer, row, col, op);
    L::syndrome(s);
    const int after = s.v.popc() + s.p.popc();
    const int terminal = after == 0;
    reward = terminal ? terminal_reward : (float)(before - after);
    return terminal;
}

// ------------------------------------------------------------------ packed transition block
struct BlockView {     // SoA sections of a packed transition block (see include/toricenv.h)
    uint64_t* pv; uint64_t* pp; uint64_t* nv; uint64_t* np;
    uint32_t* action; float* reward; float* priority; uint8_t* terminal;
    int64_t cap;
};
TQ_HD int64_t align8(int64_t x) { return (x + 7) & ~(int64_t)7; }
TQ_HD BlockView block_view(void* base, int W, int64_t cap) {
    BlockView b;
    char* p = (char*)base;
    b.cap = cap;
    b.pv = (uint64_t*)p; p += 8 * (int64_t)W * cap;
    b.pp = (uint64_t*)p; p += 8 * (int64_t)W * cap;
    b.nv = (uint64_t*)p; p += 8 * (int64_t)W * cap;
    b.np = (uint64_t*)p; p += 8 * (int64_t)W * cap;
    b.action = (uint32_t*)p; p += align8(4 * cap);
    b.reward = (float*)p; p += align8(4 * cap);
    b.priority = (float*)p; p += align8(4 * cap);
    b.terminal = (uint8_t*)p;
    return b;
}
TQ_HD int64_t block_bytes(int W, int64_t cap) {
    return 4 * 8 * (int64_t)W * cap + 3 * align8(4 * cap) + align8(cap);
}

// The four checks of the acted qubit in ITS OWN centred frame -- v[gs,gs], v[gs+1,gs], p[gs,gs], p[gs,gs-1], for
// either layer (centred-frame property) -- so the perspective of the post-step syndrome is the
// perspective of the pre-step syndrome with these bits flipped: Z component -> the two vertices, X component
// -> the two plaquettes.  (perspective() is linear over GF(2).)
template <int D>
TQ_HD void centred_flip(int op, typename Lat<D>::B& dv, typename Lat<D>::B& dp) {
    using L = Lat<D>;
    constexpr int GS = L::GS;
    dv = L::B::zero(); dp = L::B::zero();
    const int fx = (op == 1) | (op == 2), fz = (op >> 1) & 1;
    dv.flip(GS * D + GS, fz); dv.flip((GS + 1) * D + GS, fz);
    dp.flip(GS * D + GS, fx); dp.flip(GS * D + GS - 1, fx);
}

template <int D>
TQ_HD void write_transition(const BlockView& b, int64_t slot, const typename Lat<D>::B& v0, const typename Lat<D>::B& p0,
                            const typename Lat<D>::B& v1, const typename Lat<D>::B& p1, int layer, int row, int col, int op,
                            float reward, int terminal, bool stepped = false) {
    using L = Lat<D>;
    constexpr int W = L::W;
    typename L::B a, c;
    L::perspective(v0, p0, layer, row, col, a, c);
#pragma unroll
    for (int k = 0; k < W; ++k) { b.pv[(int64_t)k * b.cap + slot] = a.w[k]; b.pp[(int64_t)k * b.cap + slot] = c.w[k]; }
    if (stepped) {                                            // (v1,p1) = (v0,p0) after `op` on this very qubit
        typename L::B dv, dp;
        centred_flip<D>(op, dv, dp);
        a = a ^ dv; c = c ^ dp;
    } else {
        L::perspective(v1, p1, layer, row, col, a, c);
    }
#pragma unroll
    for (int k = 0; k < W; ++k) { b.nv[(int64_t)k * b.cap + slot] = a.w[k]; b.np[(int64_t)k * b.cap + slot] = c.w[k]; }
    // action rewritten to the centred frame (util_actor.py:256,261)
    b.action[slot] = (uint32_t)layer | ((uint32_t)L::GS << 8) | ((uint32_t)L::GS << 16) | ((uint32_t)op << 24);
    b.reward[slot] = reward;
    b.terminal[slot] = (uint8_t)terminal;
}

// A slot without a transition (no-op or rejected action): action word 0 (op = 0 marks the slot
// invalid for tq_transition_unpack / wire.decode), everything else zero -- never stale data.
template <int D>
TQ_HD void write_empty_slot(const BlockView& b, int64_t slot) {
    constexpr int W = Lat<D>::W;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        b.pv[(int64_t)k * b.cap + slot] = 0; b.pp[(int64_t)k * b.cap + slot] = 0;
        b.nv[(int64_t)k * b.cap + slot] = 0; b.np[(int64_t)k * b.cap + slot] = 0;
    }
    b.action[slot] = 0u;
    b.reward[slot] = 0.f;
    b.terminal[slot] = 0;
}

// ------------------------------------------------------------------ p_error schedule
struct PerrSchedule {
    int strategy;          // TQ_PERR_*
    double p_default, p_start, p_final, p_delta;
};

// p_error of the reset that ends `episode`, for a handle with a schedule (strategy != TQ_PERR_FIXED; a fixed handle
// resets with p_default and has no roof).  `roof` is the lattice's p_roof: the caller loads it, gets the raised
// value back and stores it.  TQ_PERR_LINEAR resets at the roof, TQ_PERR_RANDOM uniformly in [p_start, roof).
TQ_HD double scheduled_p_error(const PerrSchedule& sched, double& roof, uint64_t seed, uint32_t env, uint32_t episode) {
    roof += sched.p_delta;
    roof = roof < sched.p_final ? roof : sched.p_final;
    double p = roof;
    if (sched.strategy == 2) {
        const U4 w = draw(seed, env, episode, 0, DOMAIN_PERR, 0);
        const double span = roof - sched.p_start;
        const double t = span * u01(w.x);
        p = sched.p_start + t;
    }
    return p;
}

}  // namespace tq
