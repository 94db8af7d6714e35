// READ THIS FIRST: every experiment below RE-MAPS a virtual range (hipMemUnmap + hipMemMap of other chunks at the same
// addresses), and on this stack (ROCm 7.2, MI355X) that leaves stale address translations behind -- the kernels keep
// reaching the pages of an EARLIER mapping, several addresses can reach one page, and writes through such aliased
// translations look fast (7 TB/s and more).  Every rate this program prints after its first mapping is an artifact of that;
// it is kept as the reproducer of the effect (profiles/r03_stack_write_ab.txt section 15, profiles/r03_void_va_*).
//
// Stand-alone experiment: what about a stack buffer's physical make-up decides the rate of the stack write?
// One pool of 2 MiB physical chunks (HIP virtual memory API), ONE virtual range that is re-mapped from chunk lists,
// the product's stream kernel (stream_write.hpp) on synthetic syndromes timed on every mapping:
//   same chunks in creation order / shuffled / back in order; other chunk sets; sets interleaved; and a greedy search
//   that replaces segments of the buffer by spare chunks while the real kernel gets faster.
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 -Iinclude -Itoric-rl-decoder_amd/csrc -Itools tools/placement_bench.hip -o tools/placement_bench
//   tools/placement_bench [sets=4] [segments=16] [rounds=2]
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <random>
#include <vector>

#include "stream_write.hpp"   // (the kernel is called with its 257-entry table: equal shares (lg = 8, bias 0, no pair words), as when this harness was written)

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

constexpr int D = 7;
using L = tq::Lat<D>;
constexpr int W = L::W, NQ = L::NQ;
constexpr size_t CHUNK = 2u << 20;

__global__ __launch_bounds__(256) void k_counts(const uint64_t* __restrict__ vp, int32_t* __restrict__ counts, int64_t N,
                                                int64_t* __restrict__ part256) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int cnt = 0;
    if (e < N) {
        typename L::B v, p;
        for (int k = 0; k < W; ++k) { v.w[k] = vp[(int64_t)k * N + e]; p.w[k] = vp[((int64_t)W + k) * N + e]; }
        cnt = L::persp_count(v, p);
        counts[e] = cnt;
    }
    tq::block_count_partial(cnt, part256);
}

struct Pool {
    std::vector<hipMemGenericAllocationHandle_t> h;
    hipMemAllocationProp prop = {};
    char* va = nullptr;
    size_t n = 0;                                             // chunks of the buffer
    std::vector<int> mapped;                                  // chunk id at every position (-1: none)
    void init(size_t chunks_total, size_t n_buf) {
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = 0;
        h.resize(chunks_total);
        for (auto& x : h) CK(hipMemCreate(&x, CHUNK, &prop, 0));
        n = n_buf;
        CK(hipMemAddressReserve((void**)&va, n * CHUNK, 0, nullptr, 0));
        mapped.assign(n, -1);
    }
    void unmap_all() {
        CK(hipDeviceSynchronize());
        for (size_t i = 0; i < n; ++i) if (mapped[i] >= 0) { CK(hipMemUnmap(va + i * CHUNK, CHUNK)); mapped[i] = -1; }
    }
    void map(const std::vector<int>& ids) {                   // ids.size() == n
        CK(hipDeviceSynchronize());
        bool any = false;
        for (size_t i = 0; i < n; ++i) {
            if (mapped[i] == ids[i]) continue;
            if (mapped[i] >= 0) CK(hipMemUnmap(va + i * CHUNK, CHUNK));
            CK(hipMemMap(va + i * CHUNK, CHUNK, 0, h[ids[i]], 0));
            mapped[i] = ids[i];
            any = true;
        }
        if (any) {
            hipMemAccessDesc acc = {};
            acc.location = prop.location;
            acc.flags = hipMemAccessFlagsProtReadWrite;
            CK(hipMemSetAccess(va, n * CHUNK, &acc, 1));
        }
    }
};

int main(int argc, char** argv) {
    const int sets = argc > 1 ? atoi(argv[1]) : 4;
    const int segs = argc > 2 ? atoi(argv[2]) : 16;
    const int rounds = argc > 3 ? atoi(argv[3]) : 2;
    const int64_t N = 65536;
    const double q = 0.29;
    std::mt19937_64 rng(7);
    std::vector<uint64_t> hv((size_t)2 * W * N, 0);
    std::bernoulli_distribution bit(q);
    for (int64_t e = 0; e < N; ++e)
        for (int pl = 0; pl < 2; ++pl)
            for (int b = 0; b < L::DD; ++b)
                if (bit(rng)) hv[((size_t)pl * W + b / 64) * N + e] |= 1ull << (b & 63);
    uint64_t* vp; CK(hipMalloc(&vp, hv.size() * 8)); CK(hipMemcpy(vp, hv.data(), hv.size() * 8, hipMemcpyHostToDevice));
    int32_t* counts; CK(hipMalloc(&counts, 4 * N + 64));
    int64_t* part; CK(hipMalloc(&part, 8 * ((N + 255) / 256)));
    int64_t* off; CK(hipMalloc(&off, 8 * (N + 2)));
    int32_t* split; CK(hipMalloc(&split, 4 * 264));
    int* err; CK(hipMalloc(&err, 4)); CK(hipMemset(err, 0, 4));
    hipLaunchKernelGGL(k_counts, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, vp, counts, N, part);
    hipLaunchKernelGGL(tq::k_scan_final, dim3((unsigned)((N + tq::SCAN_CHUNK - 1) / tq::SCAN_CHUNK)), dim3(256), 0, 0, counts,
                       (const int64_t*)part, off, (int32_t*)nullptr, N, split, 8);
    CK(hipDeviceSynchronize());
    int64_t P; CK(hipMemcpy(&P, off + N, 8, hipMemcpyDeviceToHost));
    const double bytes = (double)P * (NQ * 4 + 12) + (double)N * NQ;
    int32_t* pos; CK(hipMalloc(&pos, (size_t)P * 12 + 4096));
    const size_t n = ((size_t)P * NQ * 4 + CHUNK - 1) / CHUNK;
    printf("d=%d lattices %lld perspectives %lld, %.3f GB algorithmic, buffer = %zu chunks of 2 MiB, pool = %d sets\n", D, (long long)N,
           (long long)P, bytes / 1e9, n, sets);
    Pool pool;
    pool.init(n * sets, n);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    float* out = (float*)pool.va;
    auto rate = [&](int reps = 5) {
        float a = 0;
        for (int r = 0; r <= reps; ++r) {
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL((tq::k_persp_stream<D, float, 4, 11, 8, 14, 12>), dim3(256), dim3(1024), 0, 0, vp, N, (const int64_t*)off, out, pos, P, err,
                               (int64_t)0, N, (const int32_t*)split, 8, 0, (unsigned int*)nullptr, -1, (unsigned long long*)nullptr);
            CK(hipGetLastError());
            CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if (r) a += ms;
        }
        return bytes / (a / reps) / 1e6;
    };
    auto iota = [&](int set) { std::vector<int> v(n); for (size_t i = 0; i < n; ++i) v[i] = (int)(set * n + i); return v; };
    std::mt19937 sh(5);
    // ---- 1. order vs set
    for (int s = 0; s < sets; ++s) {
        std::vector<int> ids = iota(s);
        pool.map(ids);
        const double r0 = rate();
        std::vector<double> rs;
        for (int k = 0; k < 3; ++k) { std::vector<int> p = ids; std::shuffle(p.begin(), p.end(), sh); pool.map(p); rs.push_back(rate()); }
        pool.map(ids);
        const double r1 = rate();
        std::vector<int> rev = ids; std::reverse(rev.begin(), rev.end()); pool.map(rev);
        const double r2 = rate();
        printf("set %d: creation order %6.0f   shuffled %6.0f %6.0f %6.0f   creation order again %6.0f   reversed %6.0f GB/s\n", s, r0, rs[0], rs[1], rs[2], r1, r2);
        fflush(stdout);
    }
    // ---- 2. two sets interleaved chunk by chunk, and in halves
    if (sets >= 2) {
        std::vector<int> a = iota(0), b = iota(1), m(n);
        for (size_t i = 0; i < n; ++i) m[i] = (i & 1) ? b[i] : a[i];
        pool.map(m); const double ri = rate();
        for (size_t i = 0; i < n; ++i) m[i] = i < n / 2 ? a[i] : b[i];
        pool.map(m); const double rh = rate();
        for (size_t i = 0; i < n; ++i) m[i] = i < n / 2 ? b[i] : a[i];
        pool.map(m); const double rh2 = rate();
        printf("sets 0 and 1: alternating chunks %6.0f   first half of 0 + second half of 1 %6.0f   the other halves %6.0f GB/s\n", ri, rh, rh2);
    }
    // ---- 3. greedy: replace a segment by spare chunks while the real kernel gets faster
    {
        std::vector<int> cur = iota(0);
        pool.map(cur);
        double best = rate();
        printf("greedy search from set 0 (%.0f GB/s), %d segments, spares = sets 1..%d:\n", best, segs, sets - 1);
        std::vector<int> spare;
        for (int s = 1; s < sets; ++s) { auto v = iota(s); spare.insert(spare.end(), v.begin(), v.end()); }
        size_t sp = 0;
        for (int round = 0; round < rounds; ++round) {
            for (int g = 0; g < segs; ++g) {
                const size_t a = n * g / segs, b = n * (g + 1) / segs;
                if (sp + (b - a) > spare.size()) break;
                std::vector<int> tr = cur;
                for (size_t i = a; i < b; ++i) tr[i] = spare[sp + (i - a)];
                pool.map(tr);
                const double r = rate(4);
                const bool keep = r > best * 1.003;
                printf("  round %d segment %2d: %6.0f %s\n", round, g, r, keep ? "kept" : "");
                if (keep) {
                    for (size_t i = a; i < b; ++i) std::swap(cur[i], spare[sp + (i - a)]);     // the replaced chunks become spares again
                    best = r;
                }
                sp += b - a;
                if (sp + n / segs + 1 > spare.size()) sp = 0;
            }
            pool.map(cur);
            printf("  after round %d: %6.0f GB/s (re-measured)\n", round, rate());
            fflush(stdout);
        }
    }
    // ---- 4. the same chunks (set 0, creation order) behind DIFFERENT virtual addresses
    {
        pool.unmap_all();
        char* va0 = pool.va;
        std::vector<int> ids = iota(0);
        const size_t GiB = 1ull << 30;
        char* big = nullptr;
        size_t big_gib = 2048;
        while (hipMemAddressReserve((void**)&big, big_gib * GiB, 0, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); big_gib /= 2; if (big_gib < 64) { printf("cannot reserve\n"); return 1; } }
        printf("reserved %zu GiB of virtual addresses\n", big_gib);
        printf("set 0 in creation order behind different virtual addresses (window at %p, the first range was %p):\n", (void*)big, (void*)va0);
        // ---- what makes a fresh region fast?  recipes, each in a region of the window nothing was ever mapped in
        printf("  other buffers of the launch: vp %p  offsets %p  split %p  positions %p\n", (void*)vp, (void*)off, (void*)split, (void*)pos);
        const size_t M128 = GiB / 8;
        auto at = [&](size_t o) { pool.unmap_all(); pool.va = big + o; out = (float*)pool.va; pool.map(ids); };
        auto touch = [&](int how) {                            // 0: nothing, 1: hipMemset of the buffer, 2: one stack write
            if (how == 1) { CK(hipMemsetAsync(out, 1, (size_t)P * NQ * 4, 0)); CK(hipDeviceSynchronize()); }
            if (how == 2) (void)rate(0 + 1);
        };
        struct Recipe { const char* name; int steps; long long shift_mib; int how; int pattern; };
        const Recipe rec[] = {
            {"map once", 0, 0, 0, 0},
            {"9 maps at the same address, nothing written", 8, 0, 0, 0},
            {"9 maps at the same address, a stack write after each", 8, 0, 2, 0},
            {"walk in: 8 shifts of 128 MiB, nothing written", 8, 128, 0, 0},
            {"walk in: 8 shifts of 128 MiB, hipMemset after each map", 8, 128, 1, 0},
            {"walk in: 8 shifts of 128 MiB, a stack write after each map", 8, 128, 2, 0},
            {"walk in: 8 shifts of 2 MiB, a stack write after each", 8, 2, 2, 0},
            {"walk in: 8 shifts of 16 MiB, a stack write after each", 8, 16, 2, 0},
            {"back and forth: +128 MiB, back, ... 8 times, a stack write after each", 8, 128, 2, 1},
            {"walk in: 16 shifts of 128 MiB, a stack write after each", 16, 128, 2, 0},
            {"walk in: 4 shifts of 256 MiB, a stack write after each", 4, 256, 2, 0},
            {"walk in: 2 shifts of 512 MiB, a stack write after each", 2, 512, 2, 0},
            {"walk DOWN: 8 shifts of -128 MiB, a stack write after each", 8, -128, 2, 0},
        };
        std::vector<size_t> finals;
        size_t region = 32 * GiB;
        for (const Recipe& r : rec) {
            size_t o = region + 8 * GiB;
            region += 24 * GiB;
            at(o); touch(r.how);
            for (int k = 1; k <= r.steps; ++k) {
                if (r.pattern == 1) o = (k & 1) ? o + (size_t)r.shift_mib * (1 << 20) : o - (size_t)r.shift_mib * (1 << 20);
                else o = (size_t)((long long)o + r.shift_mib * (1ll << 20));
                at(o); touch(r.how);
            }
            const double rr = rate();
            finals.push_back(o);
            printf("  %-72s -> %6.0f GB/s   (+%.3f GiB)\n", r.name, rr, (double)o / GiB);
            fflush(stdout);
        }
        printf("  the same final addresses again, in order:");
        for (size_t o : finals) { at(o); printf(" %5.0f", rate()); }
        printf("\n");
        pool.unmap_all();
        for (int k = 0; k < 4; ++k) {                        // fresh reservations of the buffer's own size
            char* v = nullptr;
            CK(hipMemAddressReserve((void**)&v, n * CHUNK + (size_t)k * 37 * CHUNK, 0, nullptr, 0));
            pool.va = v; out = (float*)v;
            pool.map(ids);
            printf("  own reservation %d (%p): %6.0f GB/s\n", k, (void*)v, rate());
            pool.unmap_all();
        }
        pool.va = va0; out = (float*)va0;
        pool.map(ids);
        printf("  the first range again (%p): %6.0f GB/s\n", (void*)va0, rate());
        float* hm = nullptr;
        CK(hipMalloc(&hm, n * CHUNK));
        out = hm;
        printf("  a hipMalloc buffer (%p): %6.0f GB/s\n", (void*)hm, rate());
        out = (float*)va0;
    }
    int e; CK(hipMemcpy(&e, err, 4, hipMemcpyDeviceToHost));
    printf("error latch %d\n", e);
    return 0;
}
