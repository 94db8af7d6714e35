// libtoricenv: C-ABI over the HIP kernels (see include/toricenv.h for the contract and the
// reference interfaces each entry point replaces).  gfx950 only; no CPU path: every entry
// point needs a HIP device and reports TQ_E_HIP otherwise.
#include <stdlib.h>
#include <atomic>
#include <string.h>

#include <mutex>
#include <new>

#include "abi_util.hpp"
#include "stream_write.hpp"
#include "select_kernels.hpp"
#include "replay.hpp"

namespace {

// per-device caches shared by handles and the stateless entry points
struct DeviceCtx {
    std::mutex mu;
    uint16_t* lut[tq::N_SIZES] = {};
    int* err = nullptr;             // error latch of the stateless entry points (tq_states_check)
    void* ws = nullptr;             // scratch of the tq_states_persp_* entry points (tq_states_reserve)
    size_t ws_bytes = 0;
    int num_cus = 0;
};
constexpr int SPLIT_MAX = 256;       // persistent workgroups of the stack write: one per CU of an MI355X
constexpr int SPLIT_LG = 13;         // the scan's table cuts the stack into 1 << SPLIT_LG fine parts: 32 per workgroup
constexpr int N_SLOT_SETS = 8;       // sets of pair words of the stack write (stream_range.hpp: pair_claim), used in turn
constexpr int SLOT_SET_WORDS = tq::pair_set_words(SPLIT_MAX);
// Fine parts (of 32) that the workgroup of an odd XCD hands to its even neighbour (stream_write.hpp: the odd XCDs of an
// MI355X store ~20 % slower; sweep in profiles/r04_xcd_bias_sweep.txt).  tq_set_xcd_bias / TORICENV_XCD_BIAS = 0..16.
// Used for d >= 7 and 32- / 16-bit stacks: smaller lattices and the u8 stack are bound by the producers, where unequal
// shares only cost (u8, d=7, in the two-stream loop: 0.0931 ms with equal shares, 0.1000 ms with 37 : 27).
constexpr int XCD_BIAS_DEFAULT = 5;
static std::atomic<int> g_xcd_bias{-1};
static int xcd_bias() {
    int b = g_xcd_bias.load(std::memory_order_relaxed);
    if (b < 0) {
        b = XCD_BIAS_DEFAULT;
        if (const char* e = getenv("TORICENV_XCD_BIAS"); e && *e) { const int v = atoi(e); b = v < 0 ? 0 : (v > 16 ? 16 : v); }
        g_xcd_bias.store(b, std::memory_order_relaxed);
    }
    return b;
}
// tq_debug_force_xcc_parity: what the stack write's workgroups take for the parity of their XCD (-1 = what the hardware says)
static std::atomic<int> g_force_xcc_parity{-1};
DeviceCtx g_ctx[MAX_DEVICES];

int decode_latch(int flag) {
    if (flag & tq::ERR_ACTION) return fail(TQ_E_ACTION, "an action outside the lattice or with op not in 1..3 was applied");
    if (flag & tq::ERR_CAPACITY) return fail(TQ_E_CAPACITY, "perspective stack capacity exceeded");
    if (flag & tq::ERR_INTERNAL)
        return fail(TQ_E_INVALID, "stack write refused: the offsets are not the scan of these lattices' perspective counts "
                                  "(stale, shifted or from another batch), or a wave gave up waiting; or a planned selection "
                                  "whose plan was made with another eps or before a step");
    if (flag & tq::ERR_INDEX) return fail(TQ_E_INDEX, "tq_reset_idx: an index outside [0, n_envs) was given");
    if (flag & tq::ERR_RESET_DUP) return fail(TQ_E_INDEX, "tq_reset_idx: an index was listed more than once");
    if (flag & tq::ERR_RESET_ROUNDS)
        return fail(TQ_E_RESET, "a reset drew %d rounds without producing a defect (p_error too small)", tq::MAX_RESET_ROUNDS);
    return TQ_OK;
}

int get_lut(int dev, int d, hipStream_t stream, const uint16_t** out) {
    DeviceCtx& c = g_ctx[dev];
    std::lock_guard<std::mutex> lock(c.mu);
    const int slot = tq::size_slot(d);
    if (!c.lut[slot]) {
        const int nq = 2 * d * d;
        const size_t bytes = (2 * (size_t)nq * nq + 15) & ~(size_t)15;
        uint16_t* p = nullptr;
        HIPCHECK(hipMalloc(&p, bytes));
        HIPCHECK(hipMemsetAsync(p, 0, bytes, stream));
        if (int rc = by_size(d, [&](auto D) { return launch_1d(tq::k_build_lut<D()>, (int64_t)nq * nq, stream, p); })) return rc;
        HIPCHECK(hipStreamSynchronize(stream));     // once per (device, d)
        c.lut[slot] = p;
    }
    if (!c.err) {
        HIPCHECK(hipMalloc((void**)&c.err, sizeof(int)));
        HIPCHECK(hipMemset(c.err, 0, sizeof(int)));
    }
    if (!c.num_cus) {
        hipDeviceProp_t prop;
        HIPCHECK(hipGetDeviceProperties(&prop, dev));
        c.num_cus = prop.multiProcessorCount;
    }
    *out = c.lut[slot];
    return TQ_OK;
}

int launch_scan(const int32_t* counts, int64_t* partial, bool partial_valid, int64_t* offsets, int32_t* counts_out,
                int64_t n, hipStream_t stream, int32_t* split) {
    const unsigned blocks = (unsigned)((n + tq::SCAN_CHUNK - 1) / tq::SCAN_CHUNK);
    if (!partial_valid)
        hipLaunchKernelGGL(tq::k_scan_partials, grid1(n), dim3(BLOCK_1D), 0, stream, counts, partial, n);
    hipLaunchKernelGGL(tq::k_scan_final, dim3(blocks), dim3(256), 0, stream, counts, partial, offsets, counts_out, n, split,
                       SPLIT_LG);
    KCHECK();
    return TQ_OK;
}

// The stack write (stream_write.hpp): SPLIT_MAX persistent workgroups, one per CU, each with its own contiguous
// part of the stack.  Waves per workgroup by role, from the sweeps of tools/stream_tune.hip (profiles/r04_stream_tune_*):
//   * storers: 4 saturate a CU's store path (2-3 for d <= 5, whose short rows leave the producers more to do);
//   * positions waves: 1 for a 4-byte stack; 2 for 16- and 8-bit stacks, which carry 2-4 times the perspectives per
//     byte stored (u8, d=7: 5.3 -> 6.0-6.2 TB/s; d=9: 6.3 -> 6.5-6.6);
//   * producers: the rest.  d >= 7 is bound by the store path whatever the mix (d >= 13: 6.9-7.0 TB/s for f32, bf16
//     and u8 with 2 to 11 producers -- since Bits::get stopped pinning bitsets in scratch / LDS; before that fix 3
//     producers beat 7 there).  Small lattices are producer-bound (a d=3 lattice is 1.3 KB of output against ~3000
//     cycles of set-up), so d <= 5 gets every wave that is left.
template <int D, int ES>
struct StreamCfg {
    static constexpr int NS = D <= 5 ? (D == 5 && ES == 2 ? 3 : 2) : 4;
    static constexpr int NPW = (ES < 4 && D >= 5) ? 2 : 1;
    static constexpr int NP = D >= 17 ? 3 : (D >= 13 ? 8 - NPW : 16 - NS - NPW);   // d >= 17: 5-7 words per plane, 8 waves = 256 VGPRs each
    static constexpr int CPW = 8, RB = 14, RP = 12;          // 8 KiB windows, 64 KB bit ring, 16 KB position ring
};
// Tried and not adopted for the producer-bound small lattices: two workgroups per CU (512 workgroups, half-size rings):
// 39 -> 45 us at d=3, no gain at d=5 -- the producers are bound by the CU's instruction issue, not by latency
// (profiles/r04_stream_tune_small_two_wgs_per_cu.txt).
template <int D, typename OutT>
int launch_persp_write_t(const uint64_t* vp, int64_t n, const int64_t* offsets, void* out, int32_t* pos,
                         int64_t capacity, int* err, hipStream_t stream, int64_t first, int64_t count,
                         const int32_t* split, unsigned int* slots, int bias, hipEvent_t done) {
    using C = StreamCfg<D, (int)sizeof(OutT)>;
    // a workgroup's part of the stack is addressed with 32-bit element offsets
    if ((double)count * (2.0 * D * D) * (2.0 * D * D) / SPLIT_MAX * 1.5 > 2.0e9)    // (the largest share is 1.5 of the mean)
        return fail(TQ_E_INVALID, "lattice range too large for one stack write (%lld lattices of d=%d)", (long long)count, D);
    return launch_signal(tq::k_persp_stream<D, OutT, C::NS, C::NP, C::CPW, C::RB, C::RP, false, C::NPW>, dim3(SPLIT_MAX),
                         dim3(64 * (C::NS + C::NPW + C::NP)), stream, done, vp, n, offsets, out, pos, capacity, err, first,
                         first + count, split, SPLIT_LG, (D >= 7 && sizeof(OutT) >= 2) ? bias : 0, slots,
                         g_force_xcc_parity.load(std::memory_order_relaxed), nullptr);
}

// split == nullptr: the cut points did not come with the scan of these offsets (a lattice sub-range, or offsets from
// elsewhere): every workgroup of the write finds its own two (find_cut).  done (may be NULL): an event the launch signals
// when it has finished (launch_signal); with no lattice to write there is no launch, and the event is recorded plainly.
template <int D>
int launch_persp_write(const uint64_t* vp, int64_t n, const int64_t* offsets, void* out, int32_t* pos,
                       int64_t capacity, int dtype, int* err, hipStream_t stream, int64_t first, int64_t count,
                       const int32_t* split, unsigned int* slots = nullptr, int bias = 0, hipEvent_t done = nullptr) {
    if (count == 0) {
        if (done) HIPCHECK(hipEventRecord(done, stream));
        return TQ_OK;
    }
    switch (dtype) {
        case TQ_F32: return launch_persp_write_t<D, float>(vp, n, offsets, out, pos, capacity, err, stream, first, count, split, slots, bias, done);
        case TQ_F16: return launch_persp_write_t<D, __half>(vp, n, offsets, out, pos, capacity, err, stream, first, count, split, slots, bias, done);
        case TQ_BF16: return launch_persp_write_t<D, tq::bf16_t>(vp, n, offsets, out, pos, capacity, err, stream, first, count, split, slots, bias, done);
        case TQ_U8: return launch_persp_write_t<D, uint8_t>(vp, n, offsets, out, pos, capacity, err, stream, first, count, split, slots, bias, done);
        default: return fail(TQ_E_INVALID, "unknown dtype %d", dtype);
    }
}

}  // namespace

struct tq_env {            // made by `new tq_env()`: what has no initialiser here starts as zero
    int n, d, w, device;
    uint64_t seed;
    int64_t first_env;
    double terminal_reward = 100.0;
    int max_steps = 75;
    int min_err;           // config "min_qubit_errors": 0 = depolarizing sampler, n > 0 = exactly n errors per reset
    tq::PerrSchedule sched = {TQ_PERR_FIXED, 0.1, 0.1, 0.1, 0.0};
    uint64_t* planes;      // [6][W][N]: the lattices
    uint64_t* planes_alt;  // the second buffer: tq_actor_step reads `planes`, writes this one, then the two swap (so the
                           // stack write of the pre-step lattices can run beside the step on another stream)
    uint64_t* prev;        // [2][W][N]
    uint32_t* episodes;
    uint32_t* steps;
    int32_t* counts;
    int64_t* partial;      // level-1 sums of the scan: one per 256 counts
    bool partial_valid;    // left current by the last all-lattice kernel (false after tq_reset_idx)
    double* p_roof;
    int* err;              // device error latch
    uint32_t* mark;        // [N] epoch of the last indexed reset that touched the lattice (duplicate detection)
    uint32_t reset_epoch;
    void* tblock;          // packed block of N slots: scratch of tq_transition_write
    const uint16_t* lut;
    int num_cus;
    int32_t* split[2];     // cut points of the stack write, written by the scan (tq_persp_count); two tables take turns, so
    const int64_t* split_for[2];   // the scan of the next step does not overwrite what a running write reads; the offsets
    int split_last;        // array each belongs to, and which one was written last
    unsigned int* slots;   // N_SLOT_SETS sets of SLOT_SET_WORDS: one word per pair of workgroups of a stack write, which settle their shares
    unsigned write_seq;    // by XCD over it (stream_write.hpp) and leave it zero; write i uses set i % N, so N writes of one handle may be in flight
    int xcd_bias = -1;     // this handle's share setting (tq_env_set_xcd_bias), or -1: the process-wide one
    int32_t* sel_need;     // [N] scratch of tq_select_plan: rows of the Q-table each lattice's selection reads,
    int64_t* sel_partial;  // and the level-1 sums of their scan
    DeviceBuffers mem;     // owns every device pointer above but lut (the device's, get_lut)
};

extern "C" {

int tq_version(void) { return TQ_VERSION; }
int tq_set_xcd_bias(int bias) {
    if (bias < 0 || bias > 16) return fail(TQ_E_INVALID, "xcd bias %d outside 0..16", bias);
    g_xcd_bias.store(bias, std::memory_order_relaxed);
    return TQ_OK;
}
int tq_get_xcd_bias(void) { return xcd_bias(); }
int tq_env_set_xcd_bias(tq_env* h, int bias) {
    if (!h) return fail(TQ_E_INVALID, "NULL handle");
    if (bias < -1 || bias > 16) return fail(TQ_E_INVALID, "xcd bias %d outside -1..16", bias);
    h->xcd_bias = bias;
    return TQ_OK;
}
int tq_env_get_xcd_bias(const tq_env* h) { return !h ? TQ_E_INVALID : (h->xcd_bias >= 0 ? h->xcd_bias : xcd_bias()); }
int tq_debug_force_xcc_parity(int parity) {
    if (parity < -1 || parity > 2) return fail(TQ_E_INVALID, "xcc parity %d outside -1..2", parity);
    g_force_xcc_parity.store(parity, std::memory_order_relaxed);
    return TQ_OK;
}

}  // extern "C"

#include "abi_stack_alloc.hpp"

extern "C" {

const char* tq_last_error(void) { return g_err; }

int tq_create(tq_env** out, int n_envs, int d, int device, uint64_t seed, int64_t first_env_id) {
    if (!out) return fail(TQ_E_INVALID, "out is NULL");
    *out = nullptr;
    if (n_envs <= 0) return fail(TQ_E_INVALID, "n_envs must be > 0 (got %d)", n_envs);
    if (!tq::size_ok(d)) return bad_size(d);
    if (first_env_id < 0 || first_env_id + n_envs > 0xFFFFFFFFll)
        return fail(TQ_E_INVALID, "global env ids must fit in 32 bits");
    if (int rc = valid_device(device)) return rc;
    DeviceGuard guard;                                        // the caller's current device is restored on return
    if (int rc = guard.enter_device(device)) return rc;
    tq_env* h = new (std::nothrow) tq_env();
    if (!h) return fail(TQ_E_INVALID, "out of host memory");
    h->n = n_envs; h->d = d; h->w = (d * d + 63) / 64; h->device = device;
    h->seed = seed; h->first_env = first_env_id;
    const size_t N = (size_t)n_envs, W = (size_t)h->w;
    DeviceBuffers& m = h->mem;
    m.zeroed(&h->planes, 6 * W * N * 8);
    m.zeroed(&h->planes_alt, 6 * W * N * 8);
    m.zeroed(&h->prev, 2 * W * N * 8);
    m.zeroed(&h->episodes, N * 4);
    m.zeroed(&h->steps, N * 4);
    m.zeroed(&h->counts, N * 4 + 32);                           // +32: int4 tail loads of the scan stay in bounds
    m.zeroed(&h->partial, ((N + tq::PART_BLOCK - 1) / tq::PART_BLOCK) * 8);
    m.zeroed(&h->p_roof, N * 8);
    m.zeroed(&h->err, 4);
    m.zeroed(&h->mark, N * 4);
    m.zeroed(&h->tblock, (size_t)tq::block_bytes(h->w, n_envs));
    for (int32_t*& t : h->split) m.zeroed(&t, (size_t)tq::cut_table_words(SPLIT_LG) * sizeof(int32_t));
    m.zeroed(&h->slots, (size_t)N_SLOT_SETS * SLOT_SET_WORDS * sizeof(unsigned int));
    m.zeroed(&h->sel_need, N * 4 + 32);                         // +32: as for counts
    m.zeroed(&h->sel_partial, ((N + tq::PART_BLOCK - 1) / tq::PART_BLOCK) * 8);
    if (const hipError_t e = m.err; e != hipSuccess) { tq_destroy(h); return fail(TQ_E_HIP, "hipMalloc failed: %s", hipGetErrorString(e)); }
    if (int rc = get_lut(device, d, nullptr, &h->lut)) { tq_destroy(h); return rc; }
    h->num_cus = g_ctx[device].num_cus;
    // set-up calls allocate AND synchronise (toricenv.h): the memsets above ran on the null stream, and a
    // caller's non-blocking stream does not order itself behind that -- the first kernel of a fresh handle
    // (k_reset reads episodes / mark) must find them zero.
    if (hipError_t se = hipStreamSynchronize(nullptr); se != hipSuccess) {
        tq_destroy(h);
        return fail(TQ_E_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(se));
    }
    *out = h;
    return TQ_OK;
}

int tq_destroy(tq_env* h) {
    if (!h) return TQ_OK;
    DeviceGuard guard;
    (void)guard.enter_device(h->device);
    h->mem.release_all();
    delete h;
    return TQ_OK;
}

int tq_set_params(tq_env* h, double p_error_default, double terminal_reward, int max_steps_per_episode) {
    if (!h) return fail(TQ_E_INVALID, "NULL handle");
    // p_error = 0 can never produce a defect: every reset would spin through MAX_RESET_ROUNDS rounds.  With the
    // fixed-n sampler (min_qubit_errors > 0, set first) p_error is not used at all and 0 is accepted.
    const bool p_unused = h->min_err > 0;
    if (!((p_error_default > 0.0 || (p_unused && p_error_default == 0.0)) && p_error_default <= 1.0))
        return fail(TQ_E_INVALID, "p_error must be in (0,1] (0 is accepted only with min_qubit_errors > 0)");
    if (max_steps_per_episode < 1) return fail(TQ_E_INVALID, "max_steps_per_episode must be >= 1");
    h->sched.p_default = p_error_default;
    h->terminal_reward = terminal_reward;
    h->max_steps = max_steps_per_episode;
    return TQ_OK;
}

int tq_set_min_qubit_errors(tq_env* h, int n_errors) {
    if (!h) return fail(TQ_E_INVALID, "NULL handle");
    if (n_errors < 0 || n_errors > 2 * h->d * h->d) return fail(TQ_E_INVALID, "min_qubit_errors must be in [0, 2*d*d]");
    if (n_errors == 0 && !(h->sched.p_default > 0.0))
        return fail(TQ_E_INVALID, "min_qubit_errors = 0 selects the depolarizing sampler, which needs p_error in (0,1]");
    h->min_err = n_errors;
    return TQ_OK;
}

int tq_set_perror_schedule(tq_env* h, int strategy, double p_start, double p_final, double p_delta) {
    DeviceGuard guard;
    if (int rc = guard.enter(h)) return rc;
    if (strategy < TQ_PERR_FIXED || strategy > TQ_PERR_RANDOM) return fail(TQ_E_INVALID, "unknown p_error strategy %d", strategy);
    if (!(p_start > 0.0 && p_start <= 1.0 && p_final > 0.0 && p_final <= 1.0 && p_delta >= 0.0))
        return fail(TQ_E_INVALID, "p_error schedule needs 0 < p_start, p_final <= 1 and p_delta >= 0");
    h->sched.strategy = strategy; h->sched.p_start = p_start; h->sched.p_final = p_final; h->sched.p_delta = p_delta;
    // env_p_errors = ones * p_start (Actor_mp.py:46)
    double* host = new (std::nothrow) double[h->n];
    if (!host) return fail(TQ_E_INVALID, "out of host memory");
    for (int i = 0; i < h->n; ++i) host[i] = p_start;
    hipError_t e = hipMemcpy(h->p_roof, host, sizeof(double) * (size_t)h->n, hipMemcpyHostToDevice);
    delete[] host;
    HIPCHECK(e);
    return TQ_OK;
}

int tq_num_envs(const tq_env* h) { return h ? h->n : 0; }
int tq_size(const tq_env* h) { return h ? h->d : 0; }

int tq_reset_all(tq_env* h, const double* p_err, void* stream_) {
    ENTER(h, "handle");
    if (int rc = by_size(h->d, [&](auto D) {
            return launch_1d(tq::k_reset<D()>, h->n, stream, h->planes, h->episodes, h->steps, h->counts, nullptr, 0, p_err,
                             h->sched.p_default, h->seed, h->first_env, h->n, h->partial, h->mark, 0u, h->min_err, h->err);
        })) return rc;
    h->partial_valid = true;
    return TQ_OK;
}

int tq_reset_idx(tq_env* h, const int32_t* idx, int n_idx, const double* p_err, void* stream_) {
    ENTER(h, "handle");
    if (n_idx < 0 || (n_idx > 0 && !idx)) return fail(TQ_E_INVALID, "bad idx / n_idx");
    if (n_idx == 0) return TQ_OK;
    if (++h->reset_epoch == 0) {                             // epoch 0 is the mark array's initial value
        HIPCHECK(hipMemsetAsync(h->mark, 0, 4 * (size_t)h->n, stream));
        h->reset_epoch = 1;
    }
    if (int rc = by_size(h->d, [&](auto D) {
            return launch_1d(tq::k_reset<D()>, n_idx, stream, h->planes, h->episodes, h->steps, h->counts, idx, n_idx, p_err,
                             h->sched.p_default, h->seed, h->first_env, h->n, nullptr, h->mark, h->reset_epoch, h->min_err, h->err);
        })) return rc;
    h->partial_valid = false;
    return TQ_OK;
}

int tq_step(tq_env* h, const int32_t* actions, float* rewards, uint8_t* terminals, void* stream_) {
    ENTER(h, "handle");
    if (!actions) return fail(TQ_E_INVALID, "actions is NULL");
    REQUIRE_ALIGNED16(actions, "actions");
    if (int rc = by_size(h->d, [&](auto D) {
            return launch_1d(tq::k_step<D()>, h->n, stream, h->planes, h->prev, actions, rewards, terminals, h->steps, h->counts,
                             h->terminal_reward, h->n, h->err, h->partial);
        })) return rc;
    h->partial_valid = true;
    return TQ_OK;
}

int tq_get_state(tq_env* h, uint8_t* out, void* stream_) {
    ENTER(h, "handle");
    if (!out) return fail(TQ_E_INVALID, "out is NULL");
    const int64_t total = (int64_t)h->n * 2 * h->d * h->d;
    return by_size(h->d, [&](auto D) { return launch_1d(tq::k_get_state<D()>, total, stream, h->planes, h->n, nullptr, h->n, out); });
}

int tq_get_state_idx(tq_env* h, const int32_t* idx, int n_idx, uint8_t* out, void* stream_) {
    ENTER(h, "handle");
    if (n_idx < 0 || (n_idx > 0 && (!idx || !out))) return fail(TQ_E_INVALID, "bad idx / out");
    if (n_idx == 0) return TQ_OK;
    const int64_t total = (int64_t)n_idx * 2 * h->d * h->d;
    return by_size(h->d, [&](auto D) { return launch_1d(tq::k_get_state<D()>, total, stream, h->planes, h->n, idx, n_idx, out); });
}

int tq_get_qubits(tq_env* h, uint8_t* out, void* stream_) {
    ENTER(h, "handle");
    if (!out) return fail(TQ_E_INVALID, "out is NULL");
    const int64_t total = (int64_t)h->n * 2 * h->d * h->d;
    return by_size(h->d, [&](auto D) { return launch_1d(tq::k_get_qubits<D()>, total, stream, h->planes, h->n, out); });
}

int tq_set_qubits(tq_env* h, const uint8_t* qubits, void* stream_) {
    ENTER(h, "handle");
    if (!qubits) return fail(TQ_E_INVALID, "qubits is NULL");
    if (int rc = by_size(h->d, [&](auto D) {
            return launch_1d(tq::k_set_qubits<D()>, h->n, stream, h->planes, h->counts, qubits, h->n, h->partial);
        })) return rc;
    h->partial_valid = true;
    return TQ_OK;
}

int tq_get_counters(tq_env* h, uint32_t* episodes, uint32_t* steps, void* stream_) {
    ENTER(h, "handle");
    if (episodes) HIPCHECK(hipMemcpyAsync(episodes, h->episodes, 4 * (size_t)h->n, hipMemcpyDeviceToDevice, stream));
    if (steps) HIPCHECK(hipMemcpyAsync(steps, h->steps, 4 * (size_t)h->n, hipMemcpyDeviceToDevice, stream));
    return TQ_OK;
}

int tq_eval_ground_state(tq_env* h, uint8_t* out, void* stream_) {
    ENTER(h, "handle");
    if (!out) return fail(TQ_E_INVALID, "out is NULL");
    return by_size(h->d, [&](auto D) { return launch_1d(tq::k_flags<D()>, h->n, stream, h->planes, h->n, out, nullptr); });
}

int tq_is_terminal(tq_env* h, uint8_t* out, void* stream_) {
    ENTER(h, "handle");
    if (!out) return fail(TQ_E_INVALID, "out is NULL");
    return by_size(h->d, [&](auto D) { return launch_1d(tq::k_flags<D()>, h->n, stream, h->planes, h->n, nullptr, out); });
}

int tq_persp_count(tq_env* h, int32_t* counts, int64_t* offsets, void* stream_) {
    ENTER(h, "handle");
    if (!offsets) return fail(TQ_E_INVALID, "offsets is NULL");
    REQUIRE_ALIGNED16(offsets, "offsets");
    REQUIRE_ALIGNED16(counts, "counts");
    const int k = h->split_last ^ 1;                         // not the table the previous scan wrote: a stack write may still read it
    if (int rc = launch_scan(h->counts, h->partial, h->partial_valid, offsets, counts, h->n, stream, h->split[k])) return rc;
    h->partial_valid = true;
    h->split_for[k] = offsets;
    h->split_last = k;
    return TQ_OK;
}

struct tq_event {          // an event the library owns: signalled by a stack write's own dispatch (tq_persp_write_signal)
    int device;
    hipEvent_t ev;
};

int tq_event_create(tq_event** out, int device) {
    if (!out) return fail(TQ_E_INVALID, "out is NULL");
    *out = nullptr;
    if (int rc = valid_device(device)) return rc;
    DeviceGuard guard;
    if (int rc = guard.enter_device(device)) return rc;
    hipEvent_t ev;
    HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    tq_event* e = new (std::nothrow) tq_event{device, ev};
    if (!e) { (void)hipEventDestroy(ev); return fail(TQ_E_INVALID, "out of host memory"); }
    *out = e;
    return TQ_OK;
}

int tq_event_destroy(tq_event* ev) {
    if (!ev) return TQ_OK;
    DeviceGuard guard;
    (void)guard.enter_device(ev->device);
    (void)hipEventDestroy(ev->ev);
    delete ev;
    return TQ_OK;
}

int tq_stream_wait_event(tq_event* ev, void* stream_) {
    DeviceGuard guard;
    if (int rc = guard.enter(ev)) return rc;
    HIPCHECK(hipStreamWaitEvent((hipStream_t)stream_, ev->ev, 0));
    return TQ_OK;
}

int tq_persp_write_range_signal(tq_env* h, const int64_t* offsets, int first, int count, void* out, int32_t* positions,
                                int64_t capacity, int dtype, tq_event* done, void* stream_) {
    ENTER(h, "handle");
    if (!offsets || !out) return fail(TQ_E_INVALID, "offsets / out is NULL");
    if (capacity < 0) return fail(TQ_E_INVALID, "negative capacity");
    if (first < 0 || count < 0 || (int64_t)first + count > h->n) return fail(TQ_E_INVALID, "lattice range outside [0, n_envs)");
    REQUIRE_ALIGNED16(out, "out");
    REQUIRE_ALIGNED16(positions, "positions");
    if (done) {
        if (done->device != h->device) return fail(TQ_E_INVALID, "the event belongs to device %d, the handle to %d", done->device, h->device);
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        HIPCHECK(hipStreamIsCapturing(stream, &cap));
        if (cap != hipStreamCaptureStatusNone)
            return fail(TQ_E_INVALID, "tq_persp_write_signal on a capturing stream: capture the plain tq_persp_write");
    }
    const uint64_t* vp = h->planes + (size_t)tq::PL_V * h->w * h->n;
    // the cut points of the whole batch came with the scan of these very offsets; for a lattice sub-range, or offsets
    // from elsewhere, the workgroups find theirs themselves
    const int32_t* split = nullptr;
    if (first == 0 && count == h->n) {
        if (offsets == h->split_for[h->split_last]) split = h->split[h->split_last];
        else if (offsets == h->split_for[h->split_last ^ 1]) split = h->split[h->split_last ^ 1];
    }
    unsigned int* slots = h->slots + (size_t)SLOT_SET_WORDS * (h->write_seq++ % N_SLOT_SETS);
    return by_size(h->d, [&](auto D) {
        return launch_persp_write<D()>(vp, h->n, offsets, out, positions, capacity, dtype, h->err, stream, first, count, split,
                                       slots, h->xcd_bias >= 0 ? h->xcd_bias : xcd_bias(), done ? done->ev : nullptr);
    });
}

int tq_debug_slot_words_nonzero(tq_env* h) {
    void* stream_ = nullptr;
    ENTER(h, "handle");
    (void)stream;
    HIPCHECK(hipDeviceSynchronize());
    std::vector<unsigned int> w((size_t)N_SLOT_SETS * SLOT_SET_WORDS);
    HIPCHECK(hipMemcpy(w.data(), h->slots, w.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
    int n = 0;
    for (unsigned int x : w) n += x != 0u;
    return n;
}

int tq_persp_write_range(tq_env* h, const int64_t* offsets, int first, int count, void* out, int32_t* positions,
                         int64_t capacity, int dtype, void* stream_) {
    return tq_persp_write_range_signal(h, offsets, first, count, out, positions, capacity, dtype, nullptr, stream_);
}

int tq_persp_write_signal(tq_env* h, const int64_t* offsets, void* out, int32_t* positions, int64_t capacity,
                          int dtype, tq_event* done, void* stream_) {
    if (!h) return fail(TQ_E_INVALID, "NULL handle");
    return tq_persp_write_range_signal(h, offsets, 0, h->n, out, positions, capacity, dtype, done, stream_);
}

int tq_persp_write(tq_env* h, const int64_t* offsets, void* out, int32_t* positions, int64_t capacity,
                   int dtype, void* stream_) {
    if (!h) return fail(TQ_E_INVALID, "NULL handle");
    return tq_persp_write_range_signal(h, offsets, 0, h->n, out, positions, capacity, dtype, nullptr, stream_);
}

// ---- stateless variants (states outside a handle) -------------------------------------------
// What a stateless entry point needs once its arguments are checked (the checks come first, so that they answer on a
// machine without a device too): the current device, and its perspective LUT and error latch, made on first use.
static int stateless_enter(int d, hipStream_t stream, int* dev, const uint16_t** lut) {
    if (int rc = current_device(dev)) return rc;
    return get_lut(*dev, d, stream, lut);
}

// Layout of the device's scratch for n states of size d: the packed v and p planes, the counts (16-byte aligned; +32:
// int4 tail loads of the scan stay in bounds), the scan's partial sums.
struct StatesScratch {
    size_t counts_at, partial_at, bytes;
    StatesScratch(int d, int64_t n) {
        const size_t w = (size_t)(d * d + 63) / 64;
        counts_at = 2 * w * (size_t)n * 8;
        partial_at = counts_at + (((size_t)n * 4 + 32 + 15) & ~(size_t)15);
        bytes = partial_at + (((size_t)n + tq::PART_BLOCK - 1) / tq::PART_BLOCK) * 8;
    }
};

// set-up call: allocates (and synchronises); the tq_states_persp_* calls themselves never allocate
int tq_states_reserve(int d, int n_max) {
    if (!tq::size_ok(d)) return bad_size(d);
    if (n_max <= 0) return fail(TQ_E_INVALID, "n_max must be > 0");
    int dev;
    const uint16_t* lut;
    if (int rc = stateless_enter(d, nullptr, &dev, &lut)) return rc;
    DeviceCtx& c = g_ctx[dev];
    std::lock_guard<std::mutex> lock(c.mu);
    const size_t need = StatesScratch(d, n_max).bytes;
    if (c.ws_bytes < need) {
        HIPCHECK(hipDeviceSynchronize());                    // work queued on the old scratch must finish first
        if (c.ws) HIPCHECK(hipFree(c.ws));
        c.ws = nullptr; c.ws_bytes = 0;
        HIPCHECK(hipMalloc(&c.ws, need));
        HIPCHECK(hipMemset(c.ws, 0, need));
        c.ws_bytes = need;
    }
    return TQ_OK;
}

static int states_scratch(int dev, int d, int n, uint64_t** vp, int32_t** counts, int64_t** partial, int** err) {
    DeviceCtx& c = g_ctx[dev];
    std::lock_guard<std::mutex> lock(c.mu);
    const StatesScratch at(d, n);
    if (c.ws_bytes < at.bytes)
        return fail(TQ_E_CAPACITY, "stateless scratch too small for %d states of d=%d: call tq_states_reserve(d, n_max) first", n, d);
    *vp = (uint64_t*)c.ws;
    *counts = (int32_t*)((char*)c.ws + at.counts_at);
    *partial = (int64_t*)((char*)c.ws + at.partial_at);
    *err = c.err;
    return TQ_OK;
}

int tq_states_persp_count(int d, int n, const uint8_t* states, int32_t* counts, int64_t* offsets, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!tq::size_ok(d)) return bad_size(d);
    if (n <= 0 || !states || !offsets) return fail(TQ_E_INVALID, "bad n / states / offsets");
    REQUIRE_ALIGNED16(offsets, "offsets");
    REQUIRE_ALIGNED16(counts, "counts");
    int dev;
    const uint16_t* lut;
    if (int rc = stateless_enter(d, stream, &dev, &lut)) return rc;
    uint64_t* vp; int32_t* cnt; int64_t* part; int* err;
    if (int rc = states_scratch(dev, d, n, &vp, &cnt, &part, &err)) return rc;
    if (int rc = by_size(d, [&](auto D) { return launch_1d(tq::k_pack_states<D()>, n, stream, states, vp, cnt, n); })) return rc;
    // no cut-point table for the stateless path: a per-device table would be shared by every caller and stream of the
    // device; the workgroups of tq_states_persp_write find their cut points themselves (find_cut, a few microseconds)
    return launch_scan(cnt, part, false, offsets, counts, n, stream, nullptr);
}

int tq_states_persp_write(int d, int n, const uint8_t* states, const int64_t* offsets, void* out,
                          int32_t* positions, int64_t capacity, int dtype, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!tq::size_ok(d)) return bad_size(d);
    if (n <= 0 || !states || !offsets || !out || capacity < 0) return fail(TQ_E_INVALID, "bad arguments");
    REQUIRE_ALIGNED16(out, "out");
    REQUIRE_ALIGNED16(positions, "positions");
    int dev;
    const uint16_t* lut;
    if (int rc = stateless_enter(d, stream, &dev, &lut)) return rc;
    uint64_t* vp; int32_t* cnt; int64_t* part; int* err;
    if (int rc = states_scratch(dev, d, n, &vp, &cnt, &part, &err)) return rc;
    return by_size(d, [&](auto D) {
        if (int rc = launch_1d(tq::k_pack_states<D()>, n, stream, states, vp, nullptr, n)) return rc;
        return launch_persp_write<D()>(vp, n, offsets, out, positions, capacity, dtype, err, stream, 0, n, nullptr);
    });
}

int tq_states_transition(int d, int n, const uint8_t* states, const uint8_t* next_states, const int32_t* actions,
                         uint8_t* persp, uint8_t* next_persp, int32_t* actions_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!tq::size_ok(d)) return bad_size(d);
    if (n <= 0 || !actions || (persp && !states) || (next_persp && !next_states)) return fail(TQ_E_INVALID, "bad arguments");
    REQUIRE_ALIGNED16(actions, "actions");
    REQUIRE_ALIGNED16(actions_out, "actions_out");
    int dev;
    const uint16_t* lut;
    if (int rc = stateless_enter(d, stream, &dev, &lut)) return rc;
    int* err = g_ctx[dev].err;
    const int64_t total = (int64_t)n * 2 * d * d;
    return by_size(d, [&](auto D) {
        return launch_1d(tq::k_states_transition<D()>, total, stream, states, next_states, actions, persp, next_persp, actions_out,
                         lut, n, err);
    });
}

int tq_states_check(void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    int dev;
    if (int rc = current_device(&dev)) return rc;
    int* latch = g_ctx[dev].err;
    if (!latch) return TQ_OK;                                // no stateless call has run on this device yet
    int flag;
    if (int rc = read_latch(latch, stream, &flag)) return rc;
    return decode_latch(flag);
}

int tq_states_select_action(int n, const float* q_table, const int64_t* offsets, const int32_t* positions,
                            const double* eps, uint64_t seed, uint64_t call_counter, int64_t first_id,
                            int32_t* actions, float* q_values, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n <= 0 || !offsets || !positions || !actions) return fail(TQ_E_INVALID, "bad n / offsets / positions / actions");
    if (q_table && !eps) return fail(TQ_E_INVALID, "eps is NULL");
    if (first_id < 0 || first_id + n > 0xFFFFFFFFll) return fail(TQ_E_INVALID, "state ids must fit in 32 bits");
    // the kernel does not depend on the lattice size (positions carry the coordinates)
    return launch_1d(tq::k_select<3>, (int64_t)n * 64, stream, q_table, offsets, positions, eps, nullptr, nullptr, call_counter,
                     call_counter >> 32, tq::DOMAIN_SEL_CALL, actions, q_values, seed, first_id, n);
}

int tq_select_action(tq_env* h, const float* q_table, const int64_t* offsets, const int32_t* positions,
                     const double* eps, int32_t* actions, float* q_values, void* stream_) {
    ENTER(h, "handle");
    if (!offsets || !positions || !actions) return fail(TQ_E_INVALID, "offsets / positions / actions is NULL");
    if (q_table && !eps) return fail(TQ_E_INVALID, "eps is NULL");
    return by_size(h->d, [&](auto D) {
        return launch_1d(tq::k_select<D()>, (int64_t)h->n * 64, stream, q_table, offsets, positions, eps, h->episodes, h->steps,
                         0u, 0u, tq::DOMAIN_SEL, actions, q_values, h->seed, h->first_env, h->n);
    });
}

// select_plan.hpp: need -> scan -> rows.  The scratch is the handle's (tq_create); nothing is allocated here.
int tq_select_plan(tq_env* h, const int64_t* offsets, const double* eps, int64_t* plan_offsets, int32_t* rows, int64_t rows_cap,
                   void* stream_) {
    ENTER(h, "handle");
    if (!offsets || !eps || !plan_offsets) return fail(TQ_E_INVALID, "offsets / eps / plan_offsets is NULL");
    if (rows_cap < 0 || (rows_cap > 0 && !rows)) return fail(TQ_E_INVALID, "bad rows / rows_cap");
    REQUIRE_ALIGNED16(plan_offsets, "plan_offsets");
    return by_size(h->d, [&](auto D) {
        if (int rc = launch_1d(tq::k_select_need<D()>, h->n, stream, offsets, eps, h->episodes, h->steps, h->sel_need, h->seed,
                               h->first_env, h->n, h->sel_partial, h->err)) return rc;
        if (int rc = launch_scan(h->sel_need, h->sel_partial, true, plan_offsets, nullptr, h->n, stream, nullptr)) return rc;
        return launch_1d(tq::k_select_rows<D()>, (int64_t)h->n * 64, stream, offsets, plan_offsets, eps, h->episodes, h->steps, rows,
                         rows_cap, h->seed, h->first_env, h->n, h->err);
    });
}

int tq_select_action_planned(tq_env* h, const float* q_rows, const int64_t* offsets, const int64_t* plan_offsets,
                             const int32_t* positions, const double* eps, int32_t* actions, float* q_values, void* stream_) {
    ENTER(h, "handle");
    if (!q_rows || !offsets || !plan_offsets || !positions || !eps || !actions)
        return fail(TQ_E_INVALID, "q_rows / offsets / plan_offsets / positions / eps / actions is NULL");
    return by_size(h->d, [&](auto D) {
        return launch_1d(tq::k_select_planned<D()>, (int64_t)h->n * 64, stream, q_rows, offsets, plan_offsets, positions, eps,
                         h->episodes, h->steps, actions, q_values, h->seed, h->first_env, h->n, h->err);
    });
}

int tq_segment_max(const float* q_table, const int64_t* offsets, int n, const int32_t* largest, float* out,
                   void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n <= 0 || !offsets || !out) return fail(TQ_E_INVALID, "bad n / offsets / out");
    return launch_1d(tq::k_segment_max, (int64_t)n * 64, stream, q_table, offsets, largest, out, n);
}

int64_t tq_transition_block_bytes(int d, int64_t cap) {
    if (!tq::size_ok(d) || cap < 0) return -1;
    return tq::block_bytes((d * d + 63) / 64, cap);
}

// the packed block this goes through is the handle's own scratch (allocated by tq_create)
int tq_transition_write(tq_env* h, const int32_t* actions, uint8_t* persp, uint8_t* next_persp,
                        int32_t* actions_out, void* stream_) {
    ENTER(h, "handle");
    if (!actions) return fail(TQ_E_INVALID, "actions is NULL");
    REQUIRE_ALIGNED16(actions, "actions");
    REQUIRE_ALIGNED16(actions_out, "actions_out");
    tq::BlockView b = tq::block_view(h->tblock, h->w, h->n);
    if (int rc = by_size(h->d, [&](auto D) {
            return launch_1d(tq::k_transition<D()>, h->n, stream, h->planes, h->prev, actions, b, 0, h->n, h->err);
        })) return rc;
    return tq_transition_unpack(h->d, h->tblock, h->n, 0, h->n, persp, next_persp, actions_out, nullptr, nullptr, nullptr,
                                stream_);
}

int tq_block_priorities(int d, void* block, int64_t cap, int n_envs, int n_steps, const float* q_values,
                        double discount, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!tq::size_ok(d)) return bad_size(d);
    if (!block || n_envs <= 0 || n_steps <= 0 || (int64_t)n_envs * n_steps > cap)
        return fail(TQ_E_INVALID, "bad block / n_envs / n_steps (n_envs * n_steps must be <= cap)");
    tq::BlockView b = tq::block_view(block, (d * d + 63) / 64, cap);
    return launch_1d(tq::k_block_priorities, (int64_t)n_envs * n_steps, stream, b, n_envs, n_steps, q_values, discount);
}

int tq_transition_unpack(int d, const void* block, int64_t cap, int64_t first, int64_t count, uint8_t* persp,
                         uint8_t* next_persp, int32_t* actions, float* rewards, uint8_t* terminals, float* priorities,
                         void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!tq::size_ok(d)) return bad_size(d);
    if (!block || first < 0 || count < 0 || first + count > cap) return fail(TQ_E_INVALID, "bad block / slot range");
    if (count == 0) return TQ_OK;
    REQUIRE_ALIGNED16(actions, "actions");
    tq::BlockView b = tq::block_view(const_cast<void*>(block), (d * d + 63) / 64, cap);
    const int64_t total = count * 2 * d * d;
    return by_size(d, [&](auto D) {
        return launch_1d(tq::k_block_unpack<D()>, total, stream, b, first, count, persp, next_persp, actions, rewards, terminals,
                         priorities);
    });
}

int tq_actor_step(tq_env* h, const int32_t* actions, int32_t* actions_out, float* rewards, uint8_t* terminals,
                  void* block, int64_t block_cap, int64_t slot_base, void* stream_) {
    ENTER(h, "handle");
    REQUIRE_ALIGNED16(actions, "actions");
    REQUIRE_ALIGNED16(actions_out, "actions_out");
    if (block && (reinterpret_cast<uintptr_t>(block) & 7u)) return fail(TQ_E_INVALID, "block must be 8-byte aligned");
    tq::BlockView b;
    memset(&b, 0, sizeof(b));
    if (block) {
        if (slot_base < 0 || slot_base + h->n > block_cap) return fail(TQ_E_CAPACITY, "transition block too small");
        b = tq::block_view(block, h->w, block_cap);
    }
    if (int rc = by_size(h->d, [&](auto D) {
            return launch_1d(tq::k_actor_step<D()>, h->n, stream, h->planes, h->planes_alt, h->episodes, h->steps, h->counts,
                             h->p_roof, actions, actions_out, rewards, terminals, b, block ? 1 : 0, slot_base, h->sched,
                             h->terminal_reward, h->max_steps, h->min_err, h->seed, h->first_env, h->n, h->err, h->partial);
        })) return rc;
    { uint64_t* t = h->planes; h->planes = h->planes_alt; h->planes_alt = t; }   // the buffer just written holds the lattices now
    h->partial_valid = true;
    return TQ_OK;
}

int tq_check(tq_env* h, void* stream_) {
    ENTER(h, "handle");
    int flag;
    if (int rc = read_latch(h->err, stream, &flag)) return rc;
    return decode_latch(flag);
}

}  // extern "C"

#include "abi_replay.hpp"
#include "abi_nn11.hpp"
#include "abi_nn11_grad.hpp"
#include "abi_nn11_opt.hpp"
#include "abi_nnw.hpp"
#include "abi_nnw_grad.hpp"
#include "abi_resnet.hpp"
