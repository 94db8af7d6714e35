// The replay memory's entry points of include/toricenv.h (part of toricenv.hip's translation unit: included there
// after launch_scan, which the compaction of tq_replay_save_block shares with the environment).
#pragma once
#include <stddef.h>

#include <new>

#include "abi_util.hpp"
#include "replay.hpp"

// ---- prioritized replay memory (replay.hpp; contract in include/toricenv.h)
struct tq_replay {                         // made by `new tq_replay()`: every member starts as zero
    int d, w, device, faithful, L, clg;
    int64_t cap, nchunks;                  // nchunks: rebuild chunks of 2^clg leaves that hold ring positions
    double alpha;
    uint64_t seed, calls, serial;          // calls: samples that drew from the handle's stream; serial: update calls
    double* tree;                          // f64[2^L - 1]
    void* ring;                            // tq::ring_bytes(w, cap)
    tq::ReplayDev* st;
    unsigned long long* stamp;             // u64[cap], last-wins stamps of the scatter update
    int32_t* flags; int64_t* partial; int64_t* offsets; int64_t scratch_cap;   // compaction scratch of save_block
    uint64_t* nplanes;                     // u64[2][w][RP_MAX_BATCH]: next-state planes of a batch (tq_replay_next_persp_*)
    int32_t* ncounts; int64_t* npartial;   // their perspective counts and the level-1 sums of the scan
    DeviceBuffers mem;                     // owns every device pointer above
};

namespace {
double* leaves(const tq_replay* r) { return r->tree + tq::leaf_node(r->L, 0); }
int replay_latch(int flag) {
    if (flag & tq::RP_ERR_UNDERFILLED) return fail(TQ_E_CAPACITY, "replay sample: fewer records filled than the batch size");
    if (flag & tq::RP_ERR_LEAF) return fail(TQ_E_INDEX, "replay sample: a draw ended on a leaf that holds no record");
    if (flag & tq::RP_ERR_INDEX) return fail(TQ_E_INDEX, "replay: an index outside [0, filled) was given");
    return TQ_OK;
}
static_assert(offsetof(tq::ReplayDev, werr) == offsetof(tq::ReplayDev, err) + sizeof(int), "tq_replay_check reads the two latches as one");

// canonical rebuild of the whole tree: every chunk, then the top levels
int replay_rebuild_all(tq_replay* r, hipStream_t stream) {
    hipLaunchKernelGGL(tq::k_replay_chunks, dim3((unsigned)r->nchunks), dim3(256), 0, stream, r->tree, r->L, r->clg,
                       r->nchunks, r->st, 0);
    hipLaunchKernelGGL(tq::k_replay_top, dim3(1), dim3(1024), 0, stream, r->tree, tq::chunk_root_level(r->L, r->clg), r->st,
                       nullptr, r->cap);
    KCHECK();
    return TQ_OK;
}

// scatter update with last-wins + rebuild of the touched paths (or of the whole tree when that is less work)
int replay_update(tq_replay* r, const int64_t* idx, const double* p, int64_t n, hipStream_t stream) {
    const unsigned long long serial = ++r->serial;
    hipLaunchKernelGGL(tq::k_replay_stamp, grid1(n), dim3(BLOCK_1D), 0, stream, idx, n, r->stamp, serial, r->st);
    hipLaunchKernelGGL(tq::k_replay_scatter, grid1(n), dim3(BLOCK_1D), 0, stream, idx, p, n, r->stamp, serial, leaves(r),
                       r->alpha, r->st);
    KCHECK();
    if (n * 64 >= r->cap) return replay_rebuild_all(r, stream);
    return launch(tq::k_replay_paths, dim3(1), dim3(1024), stream, idx, n, r->tree, r->L, r->st);
}

// the next-state planes of the records at indices[0..n) into the handle's scratch; with_counts: their perspective
// counts and level-1 sums too
template <int D>
int replay_next_planes(tq_replay* r, const int64_t* indices, int n, bool with_counts, hipStream_t stream) {
    return launch(tq::k_replay_next_planes<D>, dim3(grid1(n).x, tq::Lat<D>::W), dim3(BLOCK_1D), stream,
                  tq::ring_view(r->ring, r->w, r->cap), indices, n, r->st, r->nplanes, with_counts ? r->ncounts : nullptr,
                  r->npartial);
}
int replay_batch_ok(const int64_t* indices, int n) {
    if (!indices) return fail(TQ_E_INVALID, "indices is NULL");
    if (n < 1 || n > tq::RP_MAX_BATCH) return fail(TQ_E_INVALID, "n must be in 1..%d (got %d)", tq::RP_MAX_BATCH, n);
    return TQ_OK;
}
}  // namespace

extern "C" {

int tq_replay_create(tq_replay** out, int d, int64_t capacity, double alpha, int device, uint64_t seed, int faithful) {
    if (!out) return fail(TQ_E_INVALID, "out is NULL");
    *out = nullptr;
    if (!tq::size_ok(d)) return bad_size(d);
    if (capacity < 1 || capacity > tq::RP_MAX_CAPACITY)
        return fail(TQ_E_INVALID, "replay capacity must be in 1..%lld (got %lld)", (long long)tq::RP_MAX_CAPACITY, (long long)capacity);
    if (!(alpha >= 0.0) || alpha > 1e300) return fail(TQ_E_INVALID, "alpha must be a finite number >= 0");
    if (faithful != 0 && faithful != 1) return fail(TQ_E_INVALID, "faithful must be 0 or 1");
    if (int rc = valid_device(device)) return rc;
    DeviceGuard guard;
    if (int rc = guard.enter_device(device)) return rc;
    tq_replay* r = new (std::nothrow) tq_replay();
    if (!r) return fail(TQ_E_INVALID, "out of host memory");
    r->d = d; r->w = (d * d + 63) / 64; r->device = device; r->faithful = faithful;
    r->cap = capacity; r->alpha = alpha; r->seed = seed;
    r->L = tq::tree_levels(capacity);
    r->clg = tq::chunk_lg(r->L);
    r->nchunks = tq::chunk_count(capacity, r->clg);
    r->mem.zeroed(&r->tree, (size_t)tq::tree_nodes(r->L) * sizeof(double));
    r->mem.zeroed(&r->ring, (size_t)tq::ring_bytes(r->w, capacity));
    r->mem.zeroed(&r->st, sizeof(tq::ReplayDev));
    r->mem.zeroed(&r->stamp, (size_t)capacity * sizeof(unsigned long long));
    r->mem.zeroed(&r->nplanes, 2 * (size_t)r->w * tq::RP_MAX_BATCH * sizeof(uint64_t));
    r->mem.zeroed(&r->ncounts, (size_t)tq::RP_MAX_BATCH * 4 + 32);          // +32: int4 tail loads of the scan stay in bounds
    r->mem.zeroed(&r->npartial, (size_t)(tq::RP_MAX_BATCH / tq::PART_BLOCK) * 8);
    hipError_t e = r->mem.err;
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { tq_replay_destroy(r); return fail(TQ_E_HIP, "replay allocation failed: %s", hipGetErrorString(e)); }
    *out = r;
    return TQ_OK;
}

int tq_replay_destroy(tq_replay* r) { return destroy_handle(r); }

int tq_replay_save_block(tq_replay* r, const void* block, int64_t cap, void* stream_) {
    ENTER(r, "replay handle");
    if (!block || cap < 0) return fail(TQ_E_INVALID, "bad block / cap");
    if (reinterpret_cast<uintptr_t>(block) & 7u) return fail(TQ_E_INVALID, "block must be 8-byte aligned");
    if (cap == 0) return TQ_OK;
    if (cap > r->scratch_cap) {            // grows once per larger block (allocates, synchronises)
        HIPCHECK(hipStreamSynchronize(stream));
        r->mem.release(r->flags); r->mem.release(r->partial); r->mem.release(r->offsets);
        r->flags = nullptr; r->partial = nullptr; r->offsets = nullptr; r->scratch_cap = 0;
        r->mem.err = hipSuccess;           // a growth that failed may be tried again
        r->mem.zeroed(&r->flags, (size_t)cap * 4 + 32);
        r->mem.zeroed(&r->partial, (size_t)((cap + tq::PART_BLOCK - 1) / tq::PART_BLOCK) * 8);
        r->mem.zeroed(&r->offsets, (size_t)(cap + 1) * 8);
        HIPCHECK(r->mem.err);
        HIPCHECK(hipStreamSynchronize(nullptr));   // the zeroing ran on the null stream: it must not land on what `stream` writes
        r->scratch_cap = cap;
    }
    tq::BlockView b = tq::block_view(const_cast<void*>(block), r->w, cap);
    tq::RingView ring = tq::ring_view(r->ring, r->w, r->cap);
    if (int rc = launch_1d(tq::k_replay_flags, cap, stream, b.action, cap, r->flags)) return rc;
    if (int rc = launch_scan(r->flags, r->partial, false, r->offsets, nullptr, cap, stream, nullptr)) return rc;
    hipLaunchKernelGGL(tq::k_replay_ingest, grid1(cap), dim3(BLOCK_1D), 0, stream, b, r->offsets, ring, r->w, leaves(r),
                       r->alpha, r->st);
    const int64_t nch = tq::chunks_to_rebuild(cap, r->cap, r->clg, r->nchunks);
    hipLaunchKernelGGL(tq::k_replay_chunks, dim3((unsigned)nch), dim3(256), 0, stream, r->tree, r->L, r->clg, r->nchunks,
                       r->st, 1);
    hipLaunchKernelGGL(tq::k_replay_top, dim3(1), dim3(1024), 0, stream, r->tree, tq::chunk_root_level(r->L, r->clg), r->st,
                       r->offsets + cap, r->cap);
    KCHECK();
    return TQ_OK;
}

int64_t tq_replay_filled(tq_replay* r, void* stream_) {
    ENTER(r, "replay handle");
    int64_t filled = 0;
    HIPCHECK(hipMemcpyAsync(&filled, &r->st->filled, sizeof(int64_t), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    return filled;
}

int tq_replay_get(tq_replay* r, const int64_t* indices, int n, float* state, float* next_state, int64_t* actions_idx,
                  float* rewards, uint8_t* terminals, int32_t* actions, void* stream_) {
    ENTER(r, "replay handle");
    if (n < 0 || (n > 0 && !indices)) return fail(TQ_E_INVALID, "bad indices / n");
    if (n == 0) return TQ_OK;
    tq::RingView ring = tq::ring_view(r->ring, r->w, r->cap);
    const int64_t total = (int64_t)n * 2 * r->d * r->d;
    return by_size(r->d, [&](auto D) {
        return launch_1d(tq::k_replay_gather<D()>, total, stream, ring, indices, n, r->st, state, next_state, actions_idx,
                         rewards, terminals, actions);
    });
}

int tq_replay_sample(tq_replay* r, int batch, double beta, const double* uniforms, int64_t* indices, double* priorities,
                     double* weights, float* state, float* next_state, int64_t* actions_idx, float* rewards,
                     uint8_t* terminals, int32_t* actions, void* stream_) {
    ENTER(r, "replay handle");
    if (batch < 1 || batch > tq::RP_MAX_BATCH) return fail(TQ_E_INVALID, "batch must be in 1..%d (got %d)", tq::RP_MAX_BATCH, batch);
    if (!indices || !priorities || !weights) return fail(TQ_E_INVALID, "indices / priorities / weights is NULL");
    if (!(beta == beta)) return fail(TQ_E_INVALID, "beta is NaN");
    const uint64_t call = uniforms ? 0 : r->calls++;
    if (int rc = launch(tq::k_replay_sample, dim3(1), dim3(256), stream, r->tree, r->L, r->cap, batch, beta, uniforms, r->seed,
                        call, indices, priorities, weights, r->st)) return rc;
    if (state || next_state || actions_idx || rewards || terminals || actions)
        if (int rc = tq_replay_get(r, indices, batch, state, next_state, actions_idx, rewards, terminals, actions, stream_)) return rc;
    if (r->faithful) return replay_update(r, indices, priorities, batch, stream);    // the reference's revert (:119)
    return TQ_OK;
}

int tq_replay_next_persp_count(tq_replay* r, const int64_t* indices, int n, int32_t* counts, int64_t* offsets, void* stream_) {
    ENTER(r, "replay handle");
    if (int rc = replay_batch_ok(indices, n)) return rc;
    if (!offsets) return fail(TQ_E_INVALID, "offsets is NULL");
    REQUIRE_ALIGNED16(offsets, "offsets");
    REQUIRE_ALIGNED16(counts, "counts");
    if (int rc = by_size(r->d, [&](auto D) { return replay_next_planes<D()>(r, indices, n, true, stream); })) return rc;
    // no cut-point table: the workgroups of the write find their cut points themselves, as for states outside a handle
    return launch_scan(r->ncounts, r->npartial, true, offsets, counts, n, stream, nullptr);
}

// The planes are gathered again (as tq_states_persp_write packs again): a count / write pair shares nothing but the
// scratch, and the writer checks the offsets against the planes it is given.
int tq_replay_next_persp_write(tq_replay* r, const int64_t* indices, int n, const int64_t* offsets, void* out,
                               int32_t* positions, int64_t capacity, int dtype, void* stream_) {
    ENTER(r, "replay handle");
    if (int rc = replay_batch_ok(indices, n)) return rc;
    if (!offsets || !out) return fail(TQ_E_INVALID, "offsets / out is NULL");
    if (capacity < 0) return fail(TQ_E_INVALID, "negative capacity");
    REQUIRE_ALIGNED16(out, "out");
    REQUIRE_ALIGNED16(positions, "positions");
    return by_size(r->d, [&](auto D) {
        if (int rc = replay_next_planes<D()>(r, indices, n, false, stream)) return rc;
        return launch_persp_write<D()>(r->nplanes, n, offsets, out, positions, capacity, dtype, &r->st->werr, stream, 0, n, nullptr);
    });
}

int tq_td_target(const float* q_table, const int64_t* offsets, int n, const float* rewards, const uint8_t* terminals,
                 float discount, float lo, float hi, float* y, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (n <= 0 || !offsets || !rewards || !terminals || !y) return fail(TQ_E_INVALID, "bad n / offsets / rewards / terminals / y");
    if (!(lo <= hi)) return fail(TQ_E_INVALID, "td target: lo must be <= hi");
    // one wavefront per state, at most one workgroup per CU of an MI355X: each finds the longest slice for itself
    const unsigned blocks = (unsigned)(((int64_t)n + 3) / 4);
    return launch(tq::k_td_target, dim3(blocks < 256u ? blocks : 256u), dim3(256), stream, q_table, offsets, rewards, terminals,
                  discount, lo, hi, y, n);
}

int tq_replay_update(tq_replay* r, const int64_t* indices, const double* priorities, int n, void* stream_) {
    ENTER(r, "replay handle");
    if (n < 0 || (n > 0 && (!indices || !priorities))) return fail(TQ_E_INVALID, "bad indices / priorities / n");
    if (n == 0) return TQ_OK;
    return replay_update(r, indices, priorities, n, stream);
}

int tq_replay_reset_alpha(tq_replay* r, double alpha, void* stream_) {
    ENTER(r, "replay handle");
    if (!(alpha >= 0.0) || alpha > 1e300) return fail(TQ_E_INVALID, "alpha must be a finite number >= 0");
    if (!r->faithful && r->alpha == 0.0) return fail(TQ_E_INVALID, "reset_alpha: alpha 0 cannot be inverted");
    if (int rc = launch_1d(tq::k_replay_realpha, r->cap, stream, leaves(r), r->st, r->alpha, alpha, r->faithful)) return rc;
    r->alpha = alpha;
    return replay_rebuild_all(r, stream);
}

int tq_replay_leaves(tq_replay* r, double* out, void* stream_) {
    ENTER(r, "replay handle");
    if (!out) return fail(TQ_E_INVALID, "out is NULL");
    HIPCHECK(hipMemcpyAsync(out, leaves(r), (size_t)r->cap * sizeof(double), hipMemcpyDeviceToDevice, stream));
    return TQ_OK;
}

int64_t tq_replay_tree_nodes(const tq_replay* r) {
    if (!r) return fail(TQ_E_INVALID, "NULL replay handle");
    return tq::tree_nodes(r->L);
}

int tq_replay_tree(tq_replay* r, double* out, void* stream_) {
    ENTER(r, "replay handle");
    if (!out) return fail(TQ_E_INVALID, "out is NULL");
    HIPCHECK(hipMemcpyAsync(out, r->tree, (size_t)tq_replay_tree_nodes(r) * sizeof(double), hipMemcpyDeviceToDevice, stream));
    return TQ_OK;
}

int tq_replay_check(tq_replay* r, void* stream_) {
    ENTER(r, "replay handle");
    int flags[2] = {0, 0};                                   // the replay kernels' latch, the stack writer's
    HIPCHECK(hipMemcpyAsync(flags, &r->st->err, sizeof(flags), hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    if (flags[0] | flags[1]) HIPCHECK(hipMemsetAsync(&r->st->err, 0, sizeof(flags), stream));
    if (int rc = replay_latch(flags[0])) return rc;
    return decode_latch(flags[1]);
}

}  // extern "C"
