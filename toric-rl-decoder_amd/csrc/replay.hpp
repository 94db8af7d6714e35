// Prioritized replay memory on the device: a sum tree in f64 over a packed SoA ring of transitions.
//
// The semantics are those of the reference's PrioritizedReplayMemory / SumTree (src/ReplayMemory.py:45-152,
// src/SumTree.py); the C-ABI (tq_replay_*) and the contract are in include/toricenv.h, the design in DESIGN.md §3.5.
//
// Tree: L levels in heap order, leaf i holds record i; its index arithmetic, the geometry of the rebuild chunks and of
// the sampler's segments, and the descent step are sum_tree.hpp's, for host and device.  Between calls every internal
// node is fl(left + right): no kernel adds into the tree with atomics, so the tree is a function of its leaves.
//   * ingest: flags (action word != 0) -> the project's two-level scan (scan.hpp) -> k_replay_ingest copies the
//     non-empty slots in slot order to ring positions (cursor + k) % capacity and writes their leaves;
//   * range rebuild: k_replay_chunks reduces 2048-leaf subtrees in LDS (one workgroup each, every internal node of the
//     subtree written) and k_replay_top, one workgroup, the levels above them;
//   * scatter update with last-wins (k_replay_stamp / k_replay_scatter) and the rebuild of the touched paths
//     (k_replay_paths, one workgroup, level by level);
//   * k_replay_sample: B sequential draws in ONE workgroup, the reference's sample loop with its += diff semantics;
//   * k_replay_gather<D>: records at given indices -> the learner's batch tensors (dataToBatch, util_learner.py:7-46);
//   * k_replay_next_planes<D>: the next-state planes of the records at given indices, as they are, into the layout the
//     stack writer reads (+ their perspective counts): the learner's target side without the f32 detour.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"
#include "sum_tree.hpp"

namespace tq {

constexpr int RP_MAX_BATCH = 4096;       // draws per sample call: the pick list lives in LDS (48 KiB)
constexpr int64_t RP_MAX_CAPACITY = int64_t(1) << 26;

// error latch of a replay handle (tq_replay_check)
enum { RP_ERR_LEAF = 1, RP_ERR_UNDERFILLED = 2, RP_ERR_INDEX = 4 };

struct ReplayDev {        // device-resident state of a handle
    int64_t cursor;       // next ring position (SumTree.cursor)
    int64_t filled;       // SumTree.size
    int err;              // RP_ERR_* latch
    int werr;             // ERR_* latch of the stack writer (tq_replay_next_persp_write); read with `err`, which it follows
};

struct RingView {         // the wire block's sections without the priority section (the leaves carry it)
    uint64_t* pv; uint64_t* pp; uint64_t* nv; uint64_t* np;
    uint32_t* action; float* reward; uint8_t* terminal;
    int64_t cap;
};
__host__ __device__ inline int64_t ring_bytes(int W, int64_t cap) { return 4 * 8 * (int64_t)W * cap + 2 * align8(4 * cap) + align8(cap); }
__host__ __device__ inline RingView ring_view(void* base, int W, int64_t cap) {
    RingView r;
    char* p = (char*)base;
    r.cap = cap;
    r.pv = (uint64_t*)p; p += 8 * (int64_t)W * cap;
    r.pp = (uint64_t*)p; p += 8 * (int64_t)W * cap;
    r.nv = (uint64_t*)p; p += 8 * (int64_t)W * cap;
    r.np = (uint64_t*)p; p += 8 * (int64_t)W * cap;
    r.action = (uint32_t*)p; p += align8(4 * cap);
    r.reward = (float*)p; p += align8(4 * cap);
    r.terminal = (uint8_t*)p;
    return r;
}

// every LDS / global write of the workgroup before the barrier is seen by every read after it
__device__ __forceinline__ void rp_sync() {
    __threadfence();
    __syncthreads();
}
// the same within one wavefront (LDS only)
__device__ __forceinline__ void rp_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------ ingest
__global__ __launch_bounds__(256) void k_replay_flags(const uint32_t* __restrict__ action, int64_t n, int32_t* __restrict__ flags) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n) flags[s] = action[s] != 0u;
}

// slot s of the block with a transition is record k = offsets[s] of the block; of the `total` records only the last
// `capacity` survive (as if saved one by one); record k goes to ring position (cursor + k) % capacity.
// leaf = pow((double)priority_f32, alpha) (ReplayMemory.py:77).
__global__ __launch_bounds__(256) void k_replay_ingest(BlockView b, const int64_t* __restrict__ offsets, RingView r, int W,
                                                       double* __restrict__ leaves, double alpha,
                                                       const ReplayDev* __restrict__ st) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= b.cap) return;
    const uint32_t a = b.action[s];
    if (a == 0u) return;
    const int64_t total = offsets[b.cap], k = offsets[s];
    if (k < total - r.cap) return;
    const int64_t pos = (st->cursor + k) % r.cap;
    for (int w = 0; w < W; ++w) {
        r.pv[(int64_t)w * r.cap + pos] = b.pv[(int64_t)w * b.cap + s];
        r.pp[(int64_t)w * r.cap + pos] = b.pp[(int64_t)w * b.cap + s];
        r.nv[(int64_t)w * r.cap + pos] = b.nv[(int64_t)w * b.cap + s];
        r.np[(int64_t)w * r.cap + pos] = b.np[(int64_t)w * b.cap + s];
    }
    r.action[pos] = a;
    r.reward[pos] = b.reward[s];
    r.terminal[pos] = b.terminal[s];
    leaves[pos] = pow((double)b.priority[s], alpha);
}

// ------------------------------------------------------------------ canonical rebuild
// One workgroup per chunk of S = 2^clg leaves: every internal node of the chunk's subtree, from the leaves up to the
// chunk root.  first_from_cursor: chunk_of the cursor's chunk and blockIdx.x (the range an ingest touched starts at the
// cursor before it); otherwise chunk blockIdx.x.
// Rebuilding a canonical subtree changes nothing, so a chunk outside the touched range may be rebuilt too.
__global__ __launch_bounds__(256) void k_replay_chunks(double* __restrict__ tree, int L, int clg, int64_t nchunks,
                                                       const ReplayDev* __restrict__ st, int first_from_cursor) {
    __shared__ double buf[2][1 << RP_CHUNK_LG];
    const int tid = threadIdx.x;
    const int64_t c = first_from_cursor ? chunk_of(st->cursor >> clg, blockIdx.x, nchunks) : (int64_t)blockIdx.x;
    const int S = 1 << clg;
    const int64_t leaf0 = leaf_node(L, c * S);
    for (int i = tid; i < S; i += 256) buf[0][i] = tree[leaf0 + i];
    __syncthreads();
    int src = 0, lvl = L - 2;
    for (int n = S >> 1; n >= 1; n >>= 1, --lvl) {
        const int64_t base = level_first(lvl) + c * n;
        for (int i = tid; i < n; i += 256) {
            const double v = buf[src][2 * i] + buf[src][2 * i + 1];
            buf[src ^ 1][i] = v;
            tree[base + i] = v;
        }
        __syncthreads();
        src ^= 1;
    }
}

// Levels ltop-1 .. 0 from the chunk roots at level ltop (one workgroup).  offsets_total != NULL (ingest): then
// cursor += n and filled = min(filled + n, capacity) for the n = *offsets_total records just ingested.
__global__ __launch_bounds__(1024) void k_replay_top(double* __restrict__ tree, int ltop, ReplayDev* __restrict__ st,
                                                     const int64_t* __restrict__ offsets_total, int64_t cap) {
    const int tid = threadIdx.x;
    for (int lvl = ltop - 1; lvl >= 0; --lvl) {
        for (int64_t a = level_first(lvl) + tid; a < level_first(lvl + 1); a += 1024) tree[a] = tree[left_child(a)] + tree[left_child(a) + 1];
        rp_sync();
    }
    if (offsets_total && tid == 0) {
        const int64_t m = *offsets_total;
        st->cursor = (st->cursor + m % cap) % cap;
        st->filled = st->filled + m < cap ? st->filled + m : cap;
    }
}

// ------------------------------------------------------------------ scatter update (priority_update)
// last occurrence of an index wins, as in the reference's loop (ReplayMemory.py:132-133): the stamp of a leaf is the
// largest (serial << 32 | j) over the updates j that name it; serial grows with every update call.
__device__ __forceinline__ bool rp_index_ok(int64_t i, const ReplayDev* st) { return i >= 0 && i < st->filled; }

__global__ __launch_bounds__(256) void k_replay_stamp(const int64_t* __restrict__ idx, int64_t n, unsigned long long* __restrict__ stamp,
                                                      unsigned long long serial, ReplayDev* __restrict__ st) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t i = idx[j];
    if (!rp_index_ok(i, st)) { atomicOr(&st->err, RP_ERR_INDEX); return; }
    atomicMax(&stamp[i], (serial << 32) | (unsigned long long)j);
}

__global__ __launch_bounds__(256) void k_replay_scatter(const int64_t* __restrict__ idx, const double* __restrict__ p, int64_t n,
                                                        const unsigned long long* __restrict__ stamp, unsigned long long serial,
                                                        double* __restrict__ leaves, double alpha, const ReplayDev* __restrict__ st) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t i = idx[j];
    if (!rp_index_ok(i, st)) return;
    if (stamp[i] == ((serial << 32) | (unsigned long long)j)) leaves[i] = pow(p[j], alpha);
}

// the ancestors of the updated leaves, level by level from the bottom (one workgroup); a node shared by several paths
// is written by several threads, all with the same value
__global__ __launch_bounds__(1024) void k_replay_paths(const int64_t* __restrict__ idx, int64_t n, double* __restrict__ tree, int L,
                                                       const ReplayDev* __restrict__ st) {
    for (int lvl = L - 2; lvl >= 0; --lvl) {
        for (int64_t j = threadIdx.x; j < n; j += 1024) {
            const int64_t i = idx[j];
            if (!rp_index_ok(i, st)) continue;
            const int64_t a = ancestor_at(L, i, lvl), lc = left_child(a);
            tree[a] = tree[lc] + tree[lc + 1];
        }
        rp_sync();
    }
}

// reset_alpha (ReplayMemory.py:135-145) over the leaves [0, filled).  faithful: the reference's
// pow(pow(leaf, -alpha_old), alpha_new); otherwise the inverse it meant, pow(pow(leaf, 1/alpha_old), alpha_new).
// A zero leaf stays 0 (the reference raises ZeroDivisionError on 0.0 ** -alpha).
__global__ __launch_bounds__(256) void k_replay_realpha(double* __restrict__ leaves, const ReplayDev* __restrict__ st, double a_old,
                                                        double a_new, int faithful) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= st->filled) return;
    const double v = leaves[i];
    if (v == 0.0) return;
    leaves[i] = pow(pow(v, faithful ? -a_old : 1.0 / a_old), a_new);
}

// ------------------------------------------------------------------ sample
// PrioritizedReplayMemory.sample (ReplayMemory.py:85-124): B draws one after another.  Draw k: value = u_k * root,
// descend with value <= left ? left : (value -= left, right); the picked leaf then counts as 0 for the following draws
// (priority_update([index], [0]), :116): every ancestor a of it becomes fl(a - v) -- the reference's += diff, in pick
// order.  The tree in memory is never written here: the effective values live in LDS --
//   * the top RP_STAGE_LEVELS levels, staged and corrected in place after every pick;
//   * below them, the subtree of depth <= RP_SEG under the current node is fetched (one round trip) and the picks that
//     lie under that node are applied to it, in pick order, before the descent goes on through it.
// Wave 0 draws (its values are wave-uniform); the whole workgroup stages the tree and computes the weights.
// u: caller's uniforms f64[B], or NULL: Philox4x32-10 keyed by `seed`, counter (call lo, call hi, 0, 5<<24 | k),
// u = ((w0>>5)*2^26 + (w1>>6)) * 2^-53 (Python's random.random construction).
//
// The steps of one draw (wave 0, every value wave-uniform) that are plain arithmetic are sum_tree.hpp's: descend_staged,
// seg_fetch, seg_walk, and one lane's share of the two below.  The draw's uniform in [0, 1):
__device__ __forceinline__ double rp_uniform(const double* __restrict__ u, uint64_t seed, uint64_t call, int k) {
    if (u) return u[k];
    const U4 w = philox4x32_10((uint32_t)call, (uint32_t)(call >> 32), 0u, (DOMAIN_REPLAY << 24) | (uint32_t)k, (uint32_t)seed,
                               (uint32_t)(seed >> 32));
    return ((double)(w.x >> 5) * 67108864.0 + (double)(w.y >> 6)) * (1.0 / 9007199254740992.0);
}
// Of the k earlier picks those under `node` (of level lvl) off the fetched segment, in pick order.
__device__ __forceinline__ void rp_seg_apply_picks(double* seg, const int32_t* pleaf, const double* pv, int k, int L, int64_t node,
                                                   int lvl, int depth, int lane) {
    for (int c0 = 0; c0 < k; c0 += 64) {
        uint64_t mask = __ballot(c0 + lane < k && leaf_under(L, pleaf[c0 + lane], node, lvl));
        while (mask) {
            const int j = c0 + __ffsll((unsigned long long)mask) - 1;
            mask &= mask - 1;
            seg_apply_pick(seg, L, node, lvl, depth, pleaf[j], pv[j], lane);
            rp_wave_sync();
        }
    }
}
// The pick of draw k: into the pick list and the outputs, and off its staged ancestors.
__device__ __forceinline__ void rp_record_pick(double* stg, double* pv, int32_t* pleaf, int k, int L, int T, int64_t leaf, double cur,
                                               int64_t filled, int64_t* __restrict__ idx_out, double* __restrict__ prio_out,
                                               ReplayDev* __restrict__ st, int lane) {
    if (lane == 0) {
        pleaf[k] = (int32_t)leaf;
        pv[k] = cur;
        idx_out[k] = leaf;
        prio_out[k] = cur;
        if (leaf >= filled) atomicOr(&st->err, RP_ERR_LEAF);
    }
    stage_correct(stg, L, T, leaf, cur, lane);
}
// The weights of the B picks (whole workgroup): (1/capacity/priority)^beta, 0 for priority <= 1e-16, normalised by
// their maximum (:112-121); pv holds the priorities and is overwritten.
__device__ __forceinline__ void rp_weights(double* pv, double* wred, int B, int64_t cap, double beta, double* __restrict__ w_out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double wmax = 0.0;
    for (int k = tid; k < B; k += 256) {
        const double p = pv[k];
        const double w = p > 1e-16 ? pow(1.0 / (double)cap / p, beta) : 0.0;
        pv[k] = w;
        wmax = w > wmax ? w : wmax;
    }
    for (int o = 32; o > 0; o >>= 1) { const double t = __shfl_xor(wmax, o, 64); wmax = t > wmax ? t : wmax; }
    if (lane == 0) wred[wave] = wmax;
    __syncthreads();
    wmax = wred[0];
    for (int i = 1; i < 4; ++i) wmax = wred[i] > wmax ? wred[i] : wmax;
    for (int k = tid; k < B; k += 256) w_out[k] = wmax > 0.0 ? pv[k] / wmax : 0.0;   // all zero: the reference raises
}

__global__ __launch_bounds__(256) void k_replay_sample(const double* __restrict__ tree, int L, int64_t cap, int B, double beta,
                                                       const double* __restrict__ u, uint64_t seed, uint64_t call,
                                                       int64_t* __restrict__ idx_out, double* __restrict__ prio_out,
                                                       double* __restrict__ w_out, ReplayDev* __restrict__ st) {
    __shared__ double stg[tree_nodes(RP_STAGE_LEVELS)];
    __shared__ double pv[RP_MAX_BATCH];
    __shared__ int32_t pleaf[RP_MAX_BATCH];
    __shared__ double seg[seg_words(RP_SEG)];
    __shared__ double wred[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t filled = st->filled;
    if (filled < B) {                               // the reference returns (None, None, None) (:108-109)
        if (tid == 0) atomicOr(&st->err, RP_ERR_UNDERFILLED);
        for (int k = tid; k < B; k += 256) { idx_out[k] = -1; prio_out[k] = 0.0; w_out[k] = 0.0; }
        return;
    }
    const int T = staged_levels(L);
    for (int i = tid; i < (int)tree_nodes(T); i += 256) stg[i] = tree[i];
    __syncthreads();
    if (wave == 0) {
        for (int k = 0; k < B; ++k) {
            double value = rp_uniform(u, seed, call, k) * stg[0], cur = stg[0];
            int64_t node = descend_staged(stg, T, value, cur);
            for (int lvl = T - 1; lvl < L - 1;) {
                const int depth = seg_depth(L, lvl);
                seg_fetch(seg, tree, node, depth, lane);
                rp_wave_sync();
                rp_seg_apply_picks(seg, pleaf, pv, k, L, node, lvl, depth, lane);
                node = seg_child_node(node, depth, seg_walk(seg, depth, value, cur));
                lvl += depth;
                rp_wave_sync();                                             // seg is reloaded by the next segment
            }
            rp_record_pick(stg, pv, pleaf, k, L, T, leaf_of_node(L, node), cur, filled, idx_out, prio_out, st, lane);
            rp_wave_sync();
        }
    }
    __syncthreads();
    rp_weights(pv, wred, B, cap, beta, w_out);
}

// ------------------------------------------------------------------ gather
// records at idx[0..n) -> dataToBatch's tensors (util_learner.py:7-46): state / next_state f32[n,2,d,d], op - 1 as
// int64, reward f32, terminal bool (u8 0/1), and the raw action i32[n,4]; any output may be NULL.  An index outside
// [0, filled) latches RP_ERR_INDEX and its row is written as zeros: nothing outside the filled records is read.
template <int D>
__global__ __launch_bounds__(256) void k_replay_gather(RingView r, const int64_t* __restrict__ idx, int64_t n,
                                                       ReplayDev* __restrict__ st, float* __restrict__ state,
                                                       float* __restrict__ next_state, int64_t* __restrict__ op1,
                                                       float* __restrict__ reward, uint8_t* __restrict__ terminal,
                                                       int32_t* __restrict__ action) {
    using L = Lat<D>;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * L::NQ) return;
    const int64_t row = t / L::NQ;
    const int c = (int)(t - row * L::NQ);
    const int64_t i = idx[row];
    const bool ok = rp_index_ok(i, st);
    if (!ok && c == 0) atomicOr(&st->err, RP_ERR_INDEX);
    const int bit = c < L::DD ? c : c - L::DD;
    const int64_t wi = (int64_t)(bit >> 6) * r.cap + (ok ? i : 0);
    if (state) state[t] = ok ? (float)(((c < L::DD ? r.pv : r.pp)[wi] >> (bit & 63)) & 1) : 0.f;
    if (next_state) next_state[t] = ok ? (float)(((c < L::DD ? r.nv : r.np)[wi] >> (bit & 63)) & 1) : 0.f;
    if (c == 0) {
        const uint32_t a = ok ? r.action[i] : 0u;
        if (op1) op1[row] = (int64_t)(a >> 24) - 1;
        if (action) {
            action[4 * row] = a & 255;
            action[4 * row + 1] = (a >> 8) & 255;
            action[4 * row + 2] = (a >> 16) & 255;
            action[4 * row + 3] = a >> 24;
        }
        if (reward) reward[row] = ok ? r.reward[i] : 0.f;
        if (terminal) terminal[row] = ok ? r.terminal[i] : 0;
    }
}

// ------------------------------------------------------------------ next-state planes for the stack writer
// nv / np of the records at idx[0..n) -> vp = u64[2][W][n], what k_pack_states makes of u8 grids and k_persp_stream
// reads; one thread per (index, word), blockIdx.y = the word.  counts != NULL: the threads of word 0 also leave the
// record's perspective count (Lat::persp_count of the whole planes: of the syndrome alone, whatever the terminal byte
// says) and their block's level-1 sum for the scan.  An index outside [0, filled) reads nothing: its planes are zero,
// its count 0, and RP_ERR_INDEX is latched.
template <int D>
__global__ __launch_bounds__(256) void k_replay_next_planes(RingView r, const int64_t* __restrict__ idx, int64_t n,
                                                            ReplayDev* __restrict__ st, uint64_t* __restrict__ vp,
                                                            int32_t* __restrict__ counts, int64_t* __restrict__ part256) {
    using L = Lat<D>;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int k = blockIdx.y;
    int cnt = 0;
    if (e < n) {
        const int64_t i = idx[e];
        const bool ok = rp_index_ok(i, st);
        vp[(int64_t)k * n + e] = ok ? r.nv[(int64_t)k * r.cap + i] : 0ull;
        vp[((int64_t)L::W + k) * n + e] = ok ? r.np[(int64_t)k * r.cap + i] : 0ull;
        if (k == 0) {
            if (!ok) atomicOr(&st->err, RP_ERR_INDEX);
            if (counts) {
                typename L::B v = L::B::zero(), p = L::B::zero();
                if (ok) {
#pragma unroll
                    for (int w = 0; w < L::W; ++w) { v.w[w] = r.nv[(int64_t)w * r.cap + i]; p.w[w] = r.np[(int64_t)w * r.cap + i]; }
                }
                cnt = L::persp_count(v, p);
                counts[e] = cnt;
            }
        }
    }
    if (counts && k == 0) block_count_partial(cnt, part256);      // (uniform over the workgroup)
}

}  // namespace tq
