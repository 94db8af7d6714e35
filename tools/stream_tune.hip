// Tuning harness for the stack-write kernel (stream_write.hpp), any lattice size and output type: synthetic syndromes
// at the steady-state hit density of eps = 1 play, a handful of candidate output buffers (the rate belongs to the buffer,
// profiles/r03_stack_write_ab.txt), and on the fastest of them a sweep over {storer, positions, producer} wave counts
// with every configuration's output compared byte for byte with the first one's, plus the per-role wait statistics
// (STATS instantiation) of chosen configurations.  Build here, run on the GPU box:
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Iinclude -Itoric-rl-decoder_amd/csrc tools/stream_tune.hip -o tools/stream_tune
//   tools/stream_tune <d> <dtype: f32|bf16|u8> [lattices=65536]
// TUNE_START=1: the start of a launch by the kernel's own clock (STATS instantiation, bias TUNE_START_BIAS or 5, the best buffer),
// three launches read.  Built with -DTUNE_OTHER_HPP='"file.hpp"' -- another version of stream_write.hpp whose namespace is tqo { using
// namespace tq; ... } and whose kernel takes the same arguments -- the two kernels run in turn and the table holds both.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "stream_write.hpp"
#include "stream_write_runs.hpp"
#ifdef TUNE_OTHER_HPP
#include TUNE_OTHER_HPP
#endif

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

template <int D>
__global__ __launch_bounds__(256) void k_counts(const uint64_t* __restrict__ vp, int32_t* __restrict__ counts, int64_t N,
                                                int64_t* __restrict__ part256) {
    using L = tq::Lat<D>;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int cnt = 0;
    if (e < N) {
        typename L::B v, p;
        for (int k = 0; k < L::W; ++k) { v.w[k] = vp[(int64_t)k * N + e]; p.w[k] = vp[((int64_t)L::W + k) * N + e]; }
        cnt = L::persp_count(v, p);
        counts[e] = cnt;
    }
    tq::block_count_partial(cnt, part256);
}

__global__ void k_diff(const uint32_t* a, const uint32_t* b, int64_t n, unsigned long long* bad) {
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) c += a[i] != b[i];
    if (c) atomicAdd(bad, c);
}

static void* alloc_vmm(size_t bytes) {
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = 0;
    const size_t chunk = (size_t)2 << 20;
    const size_t n = (bytes + chunk - 1) / chunk;
    void* va = nullptr;
    CK(hipMemAddressReserve(&va, n * chunk, 0, nullptr, 0));
    for (size_t i = 0; i < n; ++i) {
        hipMemGenericAllocationHandle_t hnd;
        CK(hipMemCreate(&hnd, chunk, &prop, 0));
        CK(hipMemMap((char*)va + i * chunk, chunk, 0, hnd, 0));
        CK(hipMemRelease(hnd));
    }
    hipMemAccessDesc acc = {};
    acc.location = prop.location;
    acc.flags = hipMemAccessFlagsProtReadWrite;
    CK(hipMemSetAccess(va, n * chunk, &acc, 1));
    CK(hipMemset(va, 0, n * chunk));
    return va;
}

struct Timer {
    hipEvent_t e0, e1;
    Timer() { CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1)); }
    template <class F> float run(F f) {
        CK(hipEventRecord(e0)); f(); CK(hipGetLastError()); CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1)); return ms;
    }
};

constexpr int SLOT_SET = tq::pair_set_words(512);            // the pair words of one launch of up to 512 workgroups

struct Ctx {
    const uint64_t* vp; int64_t N; const int64_t* off; void* out; int32_t* pos; int64_t P; int* err; const int32_t* split;
    void* ref; int32_t* pref; unsigned long long* bad; double bytes; size_t out_bytes; Timer* t;
    const int32_t* split_fine; unsigned int* ticket; unsigned launches;      // the scan's table of 1 << STREAM_DYN_LG fine parts; ticket counters, used in turn
    int bias;                                                                // fine parts (of 32) an odd workgroup hands to its even neighbour
};

// KIND: 2 = the library's kernel (fine parts from the scan's table, c.bias); 0 = the experiment of tools/stream_write_runs.hpp,
// runs behind the main runs taken by ticket (schedule SCHED); 1 = the same, one run per workgroup
template <int D, typename OutT, int NS, int NPW, int NP, int CPW, int RB, int RP, int KIND, int SCHED, bool STATS>
void launch_kind(Ctx& c, int grid, const int32_t* sp, unsigned long long* st) {
    constexpr int WV = NS + NPW + NP;
    if constexpr (KIND == 2) {
        hipLaunchKernelGGL((tq::k_persp_stream<D, OutT, NS, NP, CPW, RB, RP, STATS, NPW>), dim3(grid), dim3(64 * WV), 0, 0, c.vp, c.N, c.off,
                           (OutT*)c.out, c.pos, c.P, c.err, (int64_t)0, c.N, sp ? c.split_fine : nullptr, grid == 256 ? 13 : 14, c.bias,
                           c.ticket + 8 + SLOT_SET * (c.launches % 8), -1, st);
        ++c.launches;
    } else if constexpr (KIND == 1) {
        hipLaunchKernelGGL((tqr::k_persp_stream<D, OutT, NS, NP, CPW, RB, RP, STATS, NPW, SCHED>), dim3(grid), dim3(64 * WV), 0, 0, c.vp, c.N, c.off,
                           (OutT*)c.out, c.pos, c.P, c.err, (int64_t)0, c.N, sp, 8, (unsigned int*)nullptr, (unsigned int*)nullptr, st);
    } else {
        unsigned int* tk = c.ticket + c.launches % 8, *tc = c.ticket + (c.launches + 4) % 8;
        ++c.launches;
        hipLaunchKernelGGL((tqr::k_persp_stream<D, OutT, NS, NP, CPW, RB, RP, STATS, NPW, SCHED>), dim3(grid), dim3(64 * WV), 0, 0, c.vp, c.N, c.off,
                           (OutT*)c.out, c.pos, c.P, c.err, (int64_t)0, c.N, c.split_fine, tqr::STREAM_DYN_LG, tk, tc, st);
    }
}

// GRID: workgroups (a power of two; 256 = one per CU with the scan's cut points, 512 = two per CU -- needs <= 80 KB of LDS --
// which find their cut points themselves)
template <int D, typename OutT, int NS, int NPW, int NP, int CPW, int RB, int RP, int GRID = 256, int KIND = 0, int SCHED = 0>
void one(Ctx& c, bool stats, bool is_ref) {
    constexpr int WV = NS + NPW + NP;
    const int32_t* sp = GRID == 256 ? c.split : nullptr;
    auto k = [&] { launch_kind<D, OutT, NS, NPW, NP, CPW, RB, RP, KIND, SCHED, false>(c, GRID, sp, nullptr); };
    CK(hipMemset(c.out, 0x77, c.out_bytes)); CK(hipMemset(c.pos, 0x77, (size_t)c.P * 12));
    k(); CK(hipDeviceSynchronize());
    unsigned long long nb = 0;
    if (is_ref) {
        CK(hipMemcpy(c.ref, c.out, c.out_bytes, hipMemcpyDeviceToDevice)); CK(hipMemcpy(c.pref, c.pos, (size_t)c.P * 12, hipMemcpyDeviceToDevice));
    } else {
        CK(hipMemset(c.bad, 0, 8));
        hipLaunchKernelGGL(k_diff, dim3(2048), dim3(256), 0, 0, (const uint32_t*)c.ref, (const uint32_t*)c.out, (int64_t)(c.out_bytes / 4), c.bad);
        hipLaunchKernelGGL(k_diff, dim3(256), dim3(256), 0, 0, (const uint32_t*)c.pref, (const uint32_t*)c.pos, (int64_t)c.P * 3, c.bad);
        CK(hipMemcpy(&nb, c.bad, 8, hipMemcpyDeviceToHost));
    }
    int e; CK(hipMemcpy(&e, c.err, 4, hipMemcpyDeviceToHost));
    float a = 0, mn = 1e9;
    for (int r = 0; r < 9; ++r) { float x = c.t->run(k); if (r) { a += x; mn = std::min(mn, x); } }
    printf("  %s grid %d NS=%d NPW=%d NP=%2d CPW=%2d %s %d  %7.1f us  %6.0f GB/s (best %6.0f)   %s, latch %d\n",
           KIND == 0 ? "runs by ticket  " : (KIND == 1 ? "runs, one per wg" : "library kernel  "), GRID, NS, NPW, NP, CPW, KIND == 2 ? "bias" : "sched", KIND == 2 ? c.bias : SCHED, 1e3 * a / 8,
           c.bytes / (a / 8) / 1e6, c.bytes / mn / 1e6, is_ref ? "reference of this sweep" : (nb ? "DIFFERS" : "same bytes"), e);
    if (nb) printf("      %llu differing dwords\n", nb);
    if (!stats || GRID != 256) return;
    unsigned long long* st;
    CK(hipMalloc(&st, sizeof(unsigned long long) * 256 * WV * 4));
    CK(hipMemset(st, 0, sizeof(unsigned long long) * 256 * WV * 4));
    for (int r = 0; r < 4; ++r) {                            // warm code; the last launch is the one read
        CK(hipMemset(st, 0, sizeof(unsigned long long) * 256 * WV * 4));
        launch_kind<D, OutT, NS, NPW, NP, CPW, RB, RP, KIND, SCHED, true>(c, 256, c.split, st);
        CK(hipDeviceSynchronize());
    }
    std::vector<unsigned long long> h((size_t)256 * WV * 4);
    CK(hipMemcpy(h.data(), st, h.size() * 8, hipMemcpyDeviceToHost));
    auto agg = [&](int w0, int w1, const char* role, const char* a_name, const char* b_name) {
        double tot = 0, wa = 0, wb = 0, items = 0, mx = 0; int n = 0;
        for (int g = 0; g < 256; ++g) for (int w = w0; w < w1; ++w) {
            const unsigned long long* o = &h[((size_t)g * WV + w) * 4];
            if (!o[0]) continue;
            tot += o[0]; wa += o[1]; items += (double)(o[3] & 0xFFFFull); mx = std::max(mx, (double)o[0]); ++n;
        }
        if (n) printf("      %-10s waves %5d  alive %9.0f cyc (max %9.0f)  waiting for %s %5.1f %%  %s %5.1f %%  items/wave %7.1f  busy cyc/item %7.0f\n",
                      role, n, tot / n, mx, a_name, 100 * wa / tot, b_name, 100 * wb / tot, items / n, (tot - wa - wb) / std::max(1.0, items));
    };
    {   // when the workgroups' storers began and ended, on the constant 100 MHz clock: the launch lasts until the LAST one ends
        uint32_t b0 = 0xFFFFFFFFu; std::vector<double> en(256, 0), bg(256, 1e18);
        for (int g = 0; g < 256; ++g) for (int w = 0; w < NS; ++w) { const unsigned long long x = h[((size_t)g * WV + w) * 4 + 2]; if (x) b0 = std::min(b0, (uint32_t)(x >> 32)); }
        for (int g = 0; g < 256; ++g) for (int w = 0; w < NS; ++w) {
            const unsigned long long x = h[((size_t)g * WV + w) * 4 + 2]; if (!x) continue;
            bg[g] = std::min(bg[g], (double)((uint32_t)(x >> 32) - b0) / 100.0); en[g] = std::max(en[g], (double)((uint32_t)x - b0) / 100.0);
        }
        std::vector<double> se(en); std::sort(se.begin(), se.end());
        double mean = 0, bmax = 0; for (int g = 0; g < 256; ++g) { mean += en[g] / 256; bmax = std::max(bmax, bg[g]); }
        printf("      workgroups end (us after the first began): min %.1f  p10 %.1f  median %.1f  mean %.1f  p90 %.1f  max %.1f   last begin %.1f\n",
               se[0], se[25], se[128], mean, se[230], se[255], bmax);
        printf("      mean end by XCD (workgroup %% 8):");
        for (int x = 0; x < 8; ++x) { double m = 0; for (int g = x; g < 256; g += 8) m += en[g] / 32; printf(" %.1f", m); }
        printf("\n      shader clock by XCD (cycles alive / time alive of the storers, MHz):");
        for (int x = 0; x < 8; ++x) {
            double cyc = 0, us = 0;
            for (int g = x; g < 256; g += 8) for (int w = 0; w < NS; ++w) {
                const unsigned long long* o = &h[((size_t)g * WV + w) * 4];
                if (!o[2]) continue;
                cyc += (double)o[0]; us += (double)((uint32_t)o[2] - (uint32_t)(o[2] >> 32)) / 100.0;
            }
            printf(" %.0f", us > 0 ? cyc / us : 0.0);
        }
        {   // when a workgroup's storers began their first trip (the first bytes leave the CU), us after the workgroup began
            double mn = 1e9, mx = 0, sum = 0; int n = 0;
            for (int g = 0; g < 256; ++g) {
                double f = 1e9;
                for (int w = 0; w < NS; ++w) { const unsigned long long x = h[((size_t)g * WV + w) * 4 + 3] >> 16; if (x) f = std::min(f, (double)x / 100.0); }
                if (f < 1e9) { mn = std::min(mn, f); mx = std::max(mx, f); sum += f; ++n; }
            }
            if (n) printf("\n      first trip of a workgroup's storers begins after: min %.1f  mean %.1f  max %.1f us", mn, sum / n, mx);
        }
        {   // the start of a launch as producer 0 of every workgroup sees it (us after the workgroup began, means)
            double a = 0, b = 0, c2 = 0; int n = 0;
            for (int g = 0; g < 256; ++g) {
                const unsigned long long x = h[((size_t)g * WV + NS + NPW) * 4 + 3] >> 16;
                if (!(x >> 32)) continue;
                a += (double)(x & 0xFFFF) / 100.0; b += (double)((x >> 16) & 0xFFFF) / 100.0; c2 += (double)((x >> 32) & 0xFFFF) / 100.0; ++n;
            }
            if (n) printf("\n      producer 0: range known after %.1f us, first lattice loaded after %.1f us, in the ring after %.1f us", a / n, b / n, c2 / n);
        }
        printf("\n      mean end by position in the stack (32 consecutive workgroups each):");
        for (int x = 0; x < 8; ++x) { double m = 0; for (int g = 32 * x; g < 32 * x + 32; ++g) m += en[g] / 32; printf(" %.1f", m); }
        printf("\n");
    }
    agg(0, NS, "storer", "production", "-");
    agg(NS, NS + NPW, "positions", "production", "-");
    agg(NS + NPW, WV, "producer", "ring room", "commit turn");
    CK(hipFree(st));
}

// The start of a launch by the kernel's own clock: means over the 256 workgroups, us after the workgroup began, of producer
// 0's stamps (range known, first lattice loaded, first lattice in the ring) and of the storers' first trip (min / mean / max).
struct StartStamps { double known = 0, loaded = 0, ring = 0, trip_min = 1e9, trip_mean = 0, trip_max = 0; };
template <int NS, int NPW, int NP>
StartStamps start_stamps(const std::vector<unsigned long long>& h) {
    constexpr int WV = NS + NPW + NP;
    StartStamps s; int n = 0, nt = 0;
    for (int g = 0; g < 256; ++g) {
        const unsigned long long x = h[((size_t)g * WV + NS + NPW) * 4 + 3] >> 16;
        if (x >> 32) { s.known += (double)(x & 0xFFFF) / 100.0; s.loaded += (double)((x >> 16) & 0xFFFF) / 100.0; s.ring += (double)((x >> 32) & 0xFFFF) / 100.0; ++n; }
        double f = 1e9;
        for (int w = 0; w < NS; ++w) { const unsigned long long t = h[((size_t)g * WV + w) * 4 + 3] >> 16; if (t) f = std::min(f, (double)t / 100.0); }
        if (f < 1e9) { s.trip_min = std::min(s.trip_min, f); s.trip_max = std::max(s.trip_max, f); s.trip_mean += f; ++nt; }
    }
    if (n) { s.known /= n; s.loaded /= n; s.ring /= n; }
    if (nt) s.trip_mean /= nt;
    return s;
}
template <int D, typename OutT, int NS, int NPW, int NP>
void start_table(Ctx& c) {
    constexpr int WV = NS + NPW + NP;
    unsigned long long* st;
    CK(hipMalloc(&st, sizeof(unsigned long long) * 256 * WV * 4));
    std::vector<unsigned long long> h((size_t)256 * WV * 4);
    auto launch = [&](int which) {
        CK(hipMemset(st, 0, sizeof(unsigned long long) * 256 * WV * 4));
        unsigned int* words = c.ticket + 8 + SLOT_SET * (c.launches++ % 8);
        if (which == 0)
            hipLaunchKernelGGL((tq::k_persp_stream<D, OutT, NS, NP, 8, 14, 12, true, NPW>), dim3(256), dim3(64 * WV), 0, 0, c.vp, c.N, c.off, (OutT*)c.out, c.pos, c.P,
                               c.err, (int64_t)0, c.N, c.split_fine, 13, c.bias, words, -1, st);
#ifdef TUNE_OTHER_HPP
        else
            hipLaunchKernelGGL((tqo::k_persp_stream<D, OutT, NS, NP, 8, 14, 12, true, NPW>), dim3(256), dim3(64 * WV), 0, 0, c.vp, c.N, c.off, (OutT*)c.out, c.pos, c.P,
                               c.err, (int64_t)0, c.N, c.split_fine, 13, c.bias, words, -1, st);
#endif
        CK(hipGetLastError()); CK(hipDeviceSynchronize());
        CK(hipMemcpy(h.data(), st, h.size() * 8, hipMemcpyDeviceToHost));
    };
#ifdef TUNE_OTHER_HPP
    const int kernels = 2;
#else
    const int kernels = 1;
#endif
    const char* name[2] = {"this kernel ", "other kernel"};
    for (int r = 0; r < 3; ++r) for (int k = kernels - 1; k >= 0; --k) launch(k);     // warm code
    double trip[2][3];
    printf(" the start of a launch, bias %d: means over 256 workgroups, us after the workgroup began\n", c.bias);
    for (int r = 0; r < 3; ++r)
        for (int k = kernels - 1; k >= 0; --k) {
            launch(k);
            const StartStamps s = start_stamps<NS, NPW, NP>(h);
            trip[k][r] = s.trip_mean;
            printf("   %s reading %d: range known %5.2f  first lattice loaded %5.2f  in the ring %5.2f  first storer trip min %5.2f mean %5.2f max %5.2f\n",
                   name[k], r, s.known, s.loaded, s.ring, s.trip_min, s.trip_mean, s.trip_max);
        }
    int e; CK(hipMemcpy(&e, c.err, 4, hipMemcpyDeviceToHost));
    std::vector<unsigned int> words(8 * SLOT_SET);
    CK(hipMemcpy(words.data(), c.ticket + 8, words.size() * 4, hipMemcpyDeviceToHost));
    int nz = 0; for (unsigned int x : words) nz += x != 0u;
    for (int k = kernels - 1; k >= 0; --k) {
        const double mn = std::min({trip[k][0], trip[k][1], trip[k][2]}), mx = std::max({trip[k][0], trip[k][1], trip[k][2]});
        printf("   %s first trip, mean of the three readings %5.2f us, spread %4.2f us\n", name[k], (trip[k][0] + trip[k][1] + trip[k][2]) / 3, mx - mn);
    }
    printf("   latch %d, pair words not zero afterwards: %d\n", e, nz);
    CK(hipFree(st));
}

// Would a split of the stack that follows the workgroups' OBSERVED rates end the launch sooner?  Pass 0: the scan's equal
// split, the workgroups' end times from the STATS instantiation; pass k: cut points such that workgroup g gets a share
// proportional to share_g / end_g of the pass before.  (What a dynamic hand-out of parts would converge to.)
template <int D, typename OutT, int NS, int NPW, int NP>
void rebalance(Ctx& c, const std::vector<int64_t>& off_h) {
    constexpr int WV = NS + NPW + NP;
    const int64_t N = c.N, P = off_h[N];
    std::vector<double> share(256, 1.0 / 256);
    int32_t* sp; CK(hipMalloc(&sp, 4 * 264));
    unsigned long long* st; CK(hipMalloc(&st, sizeof(unsigned long long) * 256 * WV * 4));
    for (int pass = 0; pass < 4; ++pass) {
        std::vector<int32_t> cut(257);
        double acc = 0;
        for (int g = 0; g <= 256; ++g) {
            const int64_t target = g == 256 ? P : (int64_t)(acc * (double)P);
            cut[g] = (int32_t)(std::lower_bound(off_h.begin(), off_h.begin() + N + 1, target) - off_h.begin());
            if (g < 256) acc += share[g];
        }
        cut[0] = 0; cut[256] = (int32_t)N;
        CK(hipMemcpy(sp, cut.data(), 4 * 257, hipMemcpyHostToDevice));
        auto k = [&] { hipLaunchKernelGGL((tq::k_persp_stream<D, OutT, NS, NP, 8, 14, 12, false, NPW>), dim3(256), dim3(64 * WV), 0, 0, c.vp, c.N, c.off,
                                          (OutT*)c.out, c.pos, c.P, c.err, (int64_t)0, c.N, (const int32_t*)sp, 8, 0, (unsigned int*)nullptr, -1, (unsigned long long*)nullptr); };
        float a = 0, mn = 1e9;
        for (int r = 0; r < 9; ++r) { float x = c.t->run(k); if (r) { a += x; mn = std::min(mn, x); } }
        for (int r = 0; r < 3; ++r) {
            CK(hipMemset(st, 0, sizeof(unsigned long long) * 256 * WV * 4));
            hipLaunchKernelGGL((tq::k_persp_stream<D, OutT, NS, NP, 8, 14, 12, true, NPW>), dim3(256), dim3(64 * WV), 0, 0, c.vp, c.N, c.off, (OutT*)c.out, c.pos, c.P,
                               c.err, (int64_t)0, c.N, (const int32_t*)sp, 8, 0, (unsigned int*)nullptr, -1, st);
            CK(hipDeviceSynchronize());
        }
        std::vector<unsigned long long> h((size_t)256 * WV * 4);
        CK(hipMemcpy(h.data(), st, h.size() * 8, hipMemcpyDeviceToHost));
        uint32_t b0 = 0xFFFFFFFFu; std::vector<double> en(256, 0);
        for (int g = 0; g < 256; ++g) for (int w = 0; w < NS; ++w) { const unsigned long long x = h[((size_t)g * WV + w) * 4 + 2]; if (x) b0 = std::min(b0, (uint32_t)(x >> 32)); }
        for (int g = 0; g < 256; ++g) for (int w = 0; w < NS; ++w) {
            const unsigned long long x = h[((size_t)g * WV + w) * 4 + 2]; if (x) en[g] = std::max(en[g], (double)((uint32_t)x - b0) / 100.0);
        }
        std::vector<double> se(en); std::sort(se.begin(), se.end());
        double mean = 0, smin = 1, smax = 0; for (int g = 0; g < 256; ++g) { mean += en[g] / 256; smin = std::min(smin, share[g]); smax = std::max(smax, share[g]); }
        int e; CK(hipMemcpy(&e, c.err, 4, hipMemcpyDeviceToHost));
        printf("   pass %d  shares %.3f..%.3f of 1/256   %7.1f us  %6.0f GB/s (best %6.0f)   workgroups end: min %.1f median %.1f mean %.1f max %.1f   latch %d\n", pass,
               smin * 256, smax * 256, 1e3 * a / 8, c.bytes / (a / 8) / 1e6, c.bytes / mn / 1e6, se[0], se[128], mean, se[255], e);
        double tot = 0;
        for (int g = 0; g < 256; ++g) { share[g] = share[g] / std::max(1.0, en[g]); tot += share[g]; }
        for (int g = 0; g < 256; ++g) share[g] /= tot;
    }
    CK(hipFree(st)); CK(hipFree(sp));
}

template <int D, typename OutT>
int run(int64_t N, double q, const char* tname) {
    using L = tq::Lat<D>;
    constexpr int W = L::W, NQ = L::NQ, ES = (int)sizeof(OutT);
    std::mt19937_64 rng(7);
    std::vector<uint64_t> h((size_t)2 * W * N, 0);
    std::bernoulli_distribution bit(q);
    for (int64_t e = 0; e < N; ++e)
        for (int pl = 0; pl < 2; ++pl)
            for (int b = 0; b < L::DD; ++b)
                if (bit(rng)) h[((size_t)pl * W + b / 64) * N + e] |= 1ull << (b & 63);
    uint64_t* vp; CK(hipMalloc(&vp, h.size() * 8)); CK(hipMemcpy(vp, h.data(), h.size() * 8, hipMemcpyHostToDevice));
    int32_t* counts; CK(hipMalloc(&counts, 4 * N + 64));
    int64_t* part; CK(hipMalloc(&part, 8 * ((N + 255) / 256)));
    int64_t* off; CK(hipMalloc(&off, 8 * (N + 2)));
    int32_t* split; CK(hipMalloc(&split, 4 * 264));
    int* err; CK(hipMalloc(&err, 4)); CK(hipMemset(err, 0, 4));
    hipLaunchKernelGGL(k_counts<D>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, vp, counts, N, part);
    hipLaunchKernelGGL(tq::k_scan_final, dim3((unsigned)((N + tq::SCAN_CHUNK - 1) / tq::SCAN_CHUNK)), dim3(256), 0, 0, counts,
                       (const int64_t*)part, off, (int32_t*)nullptr, N, split, 8);
    CK(hipDeviceSynchronize());
    int64_t P; CK(hipMemcpy(&P, off + N, 8, hipMemcpyDeviceToHost));
    const double bytes = (double)P * (NQ * ES + 12) + (double)N * NQ;
    const size_t out_bytes = ((size_t)P * NQ * ES + 4095) & ~(size_t)4095;
    printf("d=%d %s  lattices %lld  perspectives %lld (%.1f per lattice)  algorithmic bytes %.4f GB\n", D, tname, (long long)N, (long long)P, (double)P / N, bytes / 1e9);
    Timer t;
    Ctx c{vp, N, off, nullptr, nullptr, P, err, split, nullptr, nullptr, nullptr, bytes, out_bytes, &t, nullptr, nullptr, 0u, 0};
    {   // the table the library's scan writes: 1 << STREAM_DYN_LG fine parts; eight ticket counters
        int32_t* sf; CK(hipMalloc(&sf, 4 * ((1 << tqr::STREAM_DYN_LG) + 4)));
        hipLaunchKernelGGL(tq::k_scan_final, dim3((unsigned)((N + tq::SCAN_CHUNK - 1) / tq::SCAN_CHUNK)), dim3(256), 0, 0, counts,
                           (const int64_t*)part, off, (int32_t*)nullptr, N, sf, tqr::STREAM_DYN_LG);
        CK(hipDeviceSynchronize());
        c.split_fine = sf;
        CK(hipMalloc(&c.ticket, 4 * (8 + 8 * SLOT_SET))); CK(hipMemset(c.ticket, 0, 4 * (8 + 8 * SLOT_SET)));   // 8 ticket counters (runs experiment) + 8 sets of pair words
    }
    CK(hipMalloc(&c.ref, out_bytes)); CK(hipMalloc(&c.pref, (size_t)P * 12 + 4096)); CK(hipMalloc(&c.pos, (size_t)P * 12 + 4096)); CK(hipMalloc(&c.bad, 8));
    // candidate buffers: the product configuration on each, the fastest is used for the sweep
    constexpr int NS0 = D <= 5 ? 2 : 4, NP0 = D <= 5 ? 13 : (D >= 13 ? 7 : 11);
    std::vector<void*> bufs;
    for (int b = 0; b < 8; ++b) {
        void* x;
        if (b < 2) CK(hipMalloc(&x, out_bytes + (size_t)b * (3u << 20)));
        else x = alloc_vmm(out_bytes + (size_t)b * (2u << 20));
        bufs.push_back(x);
    }
    int best = 0; float best_ms = 1e9;
    printf("candidate buffers (product configuration NS=%d NP=%d):", NS0, NP0);
    for (int b = 0; b < 8; ++b) {
        void* ob = bufs[b];
        auto k = [&] { hipLaunchKernelGGL((tq::k_persp_stream<D, OutT, NS0, NP0, 8, 14, 12>), dim3(256), dim3(64 * (NS0 + 1 + NP0)), 0, 0, vp, N, off, (OutT*)ob, c.pos, P, err,
                                          (int64_t)0, N, (const int32_t*)split, 8, 0, (unsigned int*)nullptr, -1, (unsigned long long*)nullptr); };
        float a = 0; for (int r = 0; r < 6; ++r) { float x = t.run(k); if (r) a += x; }
        printf(" %s %.0f", b < 2 ? "hipMalloc" : "vmm", bytes / (a / 5) / 1e6);
        if (a < best_ms) { best_ms = a; best = b; }
    }
    printf("  -> buffer %d\n", best);
    c.out = bufs[best];
    if (getenv("TUNE_START")) {
        constexpr int NPW0 = (ES < 4 && D >= 5) ? 2 : 1, NSP = D == 5 && ES == 2 ? 3 : NS0, NPP = D >= 17 ? 3 : (D >= 13 ? 8 - NPW0 : 16 - NSP - NPW0);
        c.bias = getenv("TUNE_START_BIAS") ? atoi(getenv("TUNE_START_BIAS")) : 5;     // (0: equal shares, no atomic)
        start_table<D, OutT, NSP, NPW0, NPP>(c);
        return 0;
    }
    if (getenv("TUNE_BIAS")) {                                // unequal fixed shares for even / odd XCDs, on every buffer
        constexpr int NPW0 = (ES < 4 && D >= 5) ? 2 : 1, NSP = D == 5 && ES == 2 ? 3 : NS0, NPP = D >= 17 ? 3 : (D >= 13 ? 8 - NPW0 : 16 - NSP - NPW0);
        const bool st = getenv("TUNE_STATS") != nullptr;
        for (int b = 0; b < 8; ++b) {
            printf(" buffer %d\n", b); c.out = bufs[b];
            const int biases[] = {0, 2, 3, 4, 5, 6, 0};
            for (int i = 0; i < 7; ++i) { c.bias = biases[i]; one<D, OutT, NSP, NPW0, NPP, 8, 14, 12, 256, 2, 0>(c, st && (i == 0 || i == 2 || i == 3), i == 0); }
            c.bias = 0;
        }
        return 0;
    }
    if (getenv("TUNE_RUNS")) {                                // the runs experiment against the library's kernel, on every buffer
        constexpr int NPW0 = (ES < 4 && D >= 5) ? 2 : 1, NSP = D == 5 && ES == 2 ? 3 : NS0, NPP = D >= 17 ? 3 : (D >= 13 ? 8 - NPW0 : 16 - NSP - NPW0);
        const bool st = getenv("TUNE_STATS") != nullptr;
        for (int b = 0; b < 8; ++b) {
            printf(" buffer %d\n", b); c.out = bufs[b];
            one<D, OutT, NSP, NPW0, NPP, 8, 14, 12, 256, 2, 0>(c, st, true);
            one<D, OutT, NSP, NPW0, NPP, 8, 14, 12, 256, 1, 0>(c, false, false);
            one<D, OutT, NSP, NPW0, NPP, 8, 14, 12, 256, 0, 0>(c, st, false);
            one<D, OutT, NSP, NPW0, NPP, 8, 14, 12, 256, 0, 1>(c, false, false);
            one<D, OutT, NSP, NPW0, NPP, 8, 14, 12, 256, 0, 4>(c, st, false);
            one<D, OutT, NSP, NPW0, NPP, 8, 14, 12, 256, 2, 0>(c, false, false);
        }
        return 0;
    }
    if (getenv("TUNE_REBALANCE")) {
        constexpr int NPW0 = (ES < 4 && D >= 5) ? 2 : 1, NSP = D == 5 && ES == 2 ? 3 : NS0, NPP = D >= 17 ? 3 : (D >= 13 ? 8 - NPW0 : 16 - NSP - NPW0);
        std::vector<int64_t> off_h((size_t)N + 1);
        CK(hipMemcpy(off_h.data(), off, 8 * (N + 1), hipMemcpyDeviceToHost));
        for (int b = 0; b < 8; ++b) { printf(" buffer %d\n", b); c.out = bufs[b]; rebalance<D, OutT, NSP, NPW0, NPP>(c, off_h); }
        return 0;
    }
    if (getenv("TUNE_SPREAD")) {                              // the product configuration on EVERY candidate buffer, with the workgroups' end times
        constexpr int NPW0 = (ES < 4 && D >= 5) ? 2 : 1, NSP = D == 5 && ES == 2 ? 3 : NS0, NPP = D >= 17 ? 3 : (D >= 13 ? 8 - NPW0 : 16 - NSP - NPW0);
        for (int b = 0; b < 8; ++b) { printf(" buffer %d\n", b); c.out = bufs[b]; one<D, OutT, NSP, NPW0, NPP, 8, 14, 12, 256, 2, 0>(c, true, b == 0); }
        return 0;
    }
    // (KIND: see launch_kind.  A sweep of the library's kernel ends with its first configuration once more, without the
    // statistics: the drift of the box over the sweep)
#define CFG(NS, NPW, NP, CPW, KIND, STATS, REF) one<D, OutT, NS, NPW, NP, CPW, 14, 12, 256, KIND, 0>(c, STATS, REF);
    if constexpr (D == 3) {
        CFG(2, 1, 13, 8, 2, true, true)
        CFG(3, 1, 12, 8, 2, false, false)
        CFG(4, 1, 11, 8, 2, false, false)
        CFG(2, 2, 12, 8, 2, false, false)
        CFG(2, 1, 13, 8, 2, false, false)
    } else if constexpr (D == 5) {
        CFG(2, 1, 13, 8, 2, true, true)
        CFG(2, 2, 12, 8, 2, true, false)
        CFG(3, 2, 11, 8, 2, false, false)
        CFG(4, 2, 10, 8, 2, false, false)
        CFG(4, 1, 11, 8, 2, false, false)
        CFG(2, 1, 13, 8, 2, false, false)
    } else if constexpr (D >= 13) {
        CFG(4, 1, 7, 8, 0, true, true)
        CFG(4, 1, 3, 8, 0, true, false)
        CFG(4, 2, 6, 8, 0, ES < 4, false)
        CFG(4, 1, 7, 8, 0, false, false)
    } else if constexpr (D == 7) {
        CFG(4, 1, 11, 8, 2, true, true)
        CFG(4, 2, 10, 8, 2, true, false)
        CFG(3, 2, 11, 8, 2, false, false)
        CFG(4, 1, 7, 8, 2, false, false)
        CFG(4, 1, 11, 8, 2, false, false)
    } else {
        CFG(4, 1, 11, 8, 0, true, true)
        CFG(4, 2, 10, 8, 0, true, false)
        CFG(4, 3, 9, 8, 0, false, false)
        CFG(4, 1, 11, 8, 0, false, false)
    }
    return 0;
}

// f32, bf16 and u8 stacks of the same lattices written into the SAME buffers, one after the other: is a narrow stack
// slower per byte than the f32 stack on one and the same memory?
template <int D>
int run_all(int64_t N, double q) {
    using L = tq::Lat<D>;
    constexpr int W = L::W, NQ = L::NQ;
    std::mt19937_64 rng(7);
    std::vector<uint64_t> h((size_t)2 * W * N, 0);
    std::bernoulli_distribution bit(q);
    for (int64_t e = 0; e < N; ++e)
        for (int pl = 0; pl < 2; ++pl)
            for (int b = 0; b < L::DD; ++b)
                if (bit(rng)) h[((size_t)pl * W + b / 64) * N + e] |= 1ull << (b & 63);
    uint64_t* vp; CK(hipMalloc(&vp, h.size() * 8)); CK(hipMemcpy(vp, h.data(), h.size() * 8, hipMemcpyHostToDevice));
    int32_t* counts; CK(hipMalloc(&counts, 4 * N + 64));
    int64_t* part; CK(hipMalloc(&part, 8 * ((N + 255) / 256)));
    int64_t* off; CK(hipMalloc(&off, 8 * (N + 2)));
    int32_t* split; CK(hipMalloc(&split, 4 * 264));
    int* err; CK(hipMalloc(&err, 4)); CK(hipMemset(err, 0, 4));
    hipLaunchKernelGGL(k_counts<D>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, vp, counts, N, part);
    hipLaunchKernelGGL(tq::k_scan_final, dim3((unsigned)((N + tq::SCAN_CHUNK - 1) / tq::SCAN_CHUNK)), dim3(256), 0, 0, counts,
                       (const int64_t*)part, off, (int32_t*)nullptr, N, split, 8);
    CK(hipDeviceSynchronize());
    int64_t P; CK(hipMemcpy(&P, off + N, 8, hipMemcpyDeviceToHost));
    int32_t* pos; CK(hipMalloc(&pos, (size_t)P * 12 + 4096));
    const size_t out_bytes = (size_t)P * NQ * 4 + 4096;
    printf("d=%d  lattices %lld  perspectives %lld: f32 / bf16 / u8 stacks into the same buffer, GB/s of algorithmic bytes (us)\n", D, (long long)N, (long long)P);
    Timer t;
    constexpr int NS0 = 4, NP1 = D >= 13 ? 3 : 11, NP2 = D >= 13 ? 3 : 10;
    for (int b = 0; b < 8; ++b) {
        void* ob;
        if (b < 2) CK(hipMalloc(&ob, out_bytes + (size_t)b * (3u << 20)));
        else ob = alloc_vmm(out_bytes + (size_t)b * (2u << 20));
        auto kf = [&] { hipLaunchKernelGGL((tq::k_persp_stream<D, float, NS0, NP1, 8, 14, 12, false, 1>), dim3(256), dim3(64 * (NS0 + 1 + NP1)), 0, 0, vp, N, off, (float*)ob, pos, P, err, (int64_t)0, N, (const int32_t*)split, 8, 0, (unsigned int*)nullptr, -1, (unsigned long long*)nullptr); };
        auto kb = [&] { hipLaunchKernelGGL((tq::k_persp_stream<D, tq::bf16_t, NS0, NP2, 8, 14, 12, false, 2>), dim3(256), dim3(64 * (NS0 + 2 + NP2)), 0, 0, vp, N, off, (tq::bf16_t*)ob, pos, P, err, (int64_t)0, N, (const int32_t*)split, 8, 0, (unsigned int*)nullptr, -1, (unsigned long long*)nullptr); };
        auto ku = [&] { hipLaunchKernelGGL((tq::k_persp_stream<D, uint8_t, NS0, NP2, 8, 14, 12, false, 2>), dim3(256), dim3(64 * (NS0 + 2 + NP2)), 0, 0, vp, N, off, (uint8_t*)ob, pos, P, err, (int64_t)0, N, (const int32_t*)split, 8, 0, (unsigned int*)nullptr, -1, (unsigned long long*)nullptr); };
        auto km4 = [&] { (void)hipMemsetAsync(ob, 1, (size_t)P * NQ * 4, 0); };
        auto km2 = [&] { (void)hipMemsetAsync(ob, 1, (size_t)P * NQ * 2, 0); };
        auto km1 = [&] { (void)hipMemsetAsync(ob, 1, (size_t)P * NQ, 0); };
        auto tm = [&](auto k) { float a = 0; for (int r = 0; r < 7; ++r) { float x = t.run(k); if (r) a += x; } return a / 6; };
        const double by4 = (double)P * (NQ * 4 + 12) + (double)N * NQ, by2 = (double)P * (NQ * 2 + 12) + (double)N * NQ, by1 = (double)P * (NQ + 12) + (double)N * NQ;
        const float f = tm(kf), bb = tm(kb), u = tm(ku), m4 = tm(km4), m2 = tm(km2), m1 = tm(km1);
        printf("  buffer %d %-9s: f32 %5.0f (%6.1f)  bf16 %5.0f (%6.1f)  u8 %5.0f (%6.1f)   hipMemset of the stack bytes alone: %5.0f %5.0f %5.0f\n", b, b < 2 ? "hipMalloc" : "vmm 2 MiB",
               by4 / f / 1e6, 1e3 * f, by2 / bb / 1e6, 1e3 * bb, by1 / u / 1e6, 1e3 * u, (double)P * NQ * 4 / m4 / 1e6, (double)P * NQ * 2 / m2 / 1e6, (double)P * NQ / m1 / 1e6);
    }
    return 0;
}

template <int D>
int run_t(const char* ty, int64_t N, double q) {
    if (!strcmp(ty, "all")) return run_all<D>(N, q);
    if (!strcmp(ty, "f32")) return run<D, float>(N, q, ty);
    if (!strcmp(ty, "bf16")) return run<D, tq::bf16_t>(N, q, ty);
    if (!strcmp(ty, "u8")) return run<D, uint8_t>(N, q, ty);
    printf("dtype must be f32, bf16 or u8\n");
    return 1;
}

int main(int argc, char** argv) {
    const int d = argc > 1 ? atoi(argv[1]) : 7;
    const char* ty = argc > 2 ? argv[2] : "f32";
    const int64_t N = argc > 3 ? atoll(argv[3]) : 65536;
    // defect probability per check that reproduces the steady-state perspectives per lattice of eps = 1 play
    const double q = argc > 4 ? atof(argv[4]) : (d == 3 ? 0.42 : d == 5 ? 0.349 : d == 7 ? 0.29 : d == 9 ? 0.311 : d == 11 ? 0.26 : d == 13 ? 0.217 : 0.175);
#ifdef TUNE_D
    return run_t<TUNE_D>(ty, N, q);
#else
    if (d == 5) return run_t<5>(ty, N, q);
    if (d == 7) return run_t<7>(ty, N, q);
    printf("built for d = 5, 7 (or -DTUNE_D=<d>)\n");
    return 1;
#endif
}
