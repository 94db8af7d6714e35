// Perspective stack write, producer / storer form (gfx950 / CDNA4).
//
// One persistent workgroup per CU owns a CONTIGUOUS range of the output (lattices [e_lo, e_hi), cut by perspective
// count, k_scan_final / find_cut: one fixed share per workgroup, larger for the workgroups on the faster XCDs).  Inside the workgroup
// the two jobs of the stack write are done by different waves:
//   * NP producer waves build lattice bitstreams (lattice.hpp, PStream: rotated planes by ballot, table of
//     row-rolled planes, one lane per hit, ds_or_b32) -- not into a per-wave buffer but into ONE ring in LDS
//     that is the workgroup's output range as a bit string (bit x = element org + x of the stack);
//   * NS storer waves do nothing but  ds_read_b32 -> shift -> bit->element expansion -> global_store_dwordx4
//     along that range, in aligned windows of CPW KiB, and hand the ring words back zeroed;
//   * NPW positions waves write the positions (P,3) from a second ring (one packed dword per perspective).
// Hand-off: `pq[p]` (producer p: how far it is -- the first perspective of its lattice that is not in the rings yet,
// published per lattice and after every pass of 64 hits inside a lattice; its earlier lattices are complete; the
// minimum over the producers is the produced PREFIX of the range, no producer ever waits for another),
// `cons[s]` (low-water mark of storer s), `pcons[w]` (of positions wave w): plain LDS words, polled with s_sleep.
// Every poll loop is the one bounded wait (wait_until); a wave that gives up raises `abort` for its workgroup and
// latches ERR_INTERNAL, so the grid always drains.
//
// Output lines: the stack is cut into 128-byte lines and a workgroup stores the lines whose FIRST element lies
// in its range, whole.  The trailing elements of its last line belong to the first lattice(s) of the next
// range: its producers simply go on for the few perspectives that line needs (`need_extra`).  That arithmetic, the
// slot -> fine parts mapping is stream_range.hpp, the cut points are cut_points.hpp: host + device, tested without a GPU.
//
// The kernel, in the order of this file: stream_setup (workgroup-uniform: the pair's slot, cut points, capacity, range), one function
// per role -- storer_wave, positions_wave, producer_wave -- and the entry k_persp_stream, which runs the set-up and
// dispatches on the wave number.  The roles share StreamShape, StreamCtx, wait_until and StreamStats.
#pragma once
#include "kernels.hpp"
#include "stream_range.hpp"

namespace tq {

constexpr int ERR_INTERNAL = 32;
constexpr int STREAM_SPIN_LIMIT = 1 << 21;

// Hand-off words live in LDS, which one workgroup's waves see coherently, and a wave's LDS operations execute in
// issue order: publishing needs no memory fence, only the COMPILER must keep the order (a workgroup-scope release
// would also drain vmcnt, i.e. stall a storer on its own global stores); reading needs only the s_waitcnt that the
// use of the value implies.
__device__ __forceinline__ uint32_t lds_peek(const uint32_t& w) {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}
__device__ __forceinline__ void lds_after_peek() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }
__device__ __forceinline__ void lds_publish(uint32_t& w, uint32_t v, int lane) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    if (lane == 0) __hip_atomic_store(&w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ uint64_t readlane64(uint64_t x, int l) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}
// minimum of the first CNT lanes' words (LDS hand-off marks; the other lanes count as 0xFFFFFFFF); wave-uniform.  The
// producers' form, a butterfly in vector registers; the consumers' `produced` takes the same minimum on the scalar unit.
// Two helpers on purpose: in a producer the scalar form crowds more wave-uniform values out of the SGPRs into vector lanes
// (profiles/stream_roles_resource_usage.txt), a storer has no use for the butterfly's cross-lane traffic.
template <int CNT>
__device__ __forceinline__ uint32_t lds_min(const uint32_t* w, int lane) {
    uint32_t c = 0xFFFFFFFFu;
    if (lane < CNT) c = __hip_atomic_load(&w[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
    for (int o = 1; o < CNT; o <<= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)c, o, 64); c = t < c ? t : c; }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
}

// OR the NQ-bit string of one perspective into the ring at bit position `pos` (the caller's orfn reduces the dword
// index mod the ring)
template <int D, class OrFn>
__device__ __forceinline__ void emit_at(uint32_t pos, const typename Lat<D>::B& ov, const typename Lat<D>::B& op, OrFn&& orfn) {
    using S = PStream<D>;
    const uint32_t base = pos >> 5;
    const int sh = (int)(pos & 31);
    uint32_t prev = 0;
#pragma unroll
    for (int j = 0; j <= S::ND; ++j) {
        const uint32_t cur = j < S::ND ? S::string_dword(ov, op, j) : 0u;
        const uint32_t val = (cur << sh) | ((prev >> 1) >> (31 - sh));
        if (j < S::ND || val) orfn(base + j, val);
        prev = cur;
    }
}

template <int D>
struct LatTables {                                             // of ONE lattice
    static constexpr int NQP = (Lat<D>::NQ + 7) & ~7;
    uint64_t rr[4][D][Lat<D>::W];                              // V, P, rot V, rot P rolled by every row amount
    uint32_t hpos[NQP];                                        // k-th hit -> layer | row << 8 | col << 16
};
// private to one producer wave: one lattice at a time, its hits done in passes of 64 lanes (a lattice of 73 hits pays
// for two passes)
template <int D>
struct ProdTables {
    LatTables<D> t;
    uint64_t low[D][Lat<D>::W];                                // lowcols(k): the same for every lattice
};

template <int D, int NS, int NP, int RB_LOG, int RP_LOG, int NPW = 1>
struct StreamLds {
    __attribute__((aligned(16))) uint32_t bits[1u << RB_LOG];  // the output range as a bit string, ring
    uint32_t posr[1u << RP_LOG];                               // packed position of perspective q at [q & mask]
    ProdTables<D> tab[NP];
    uint32_t pq[NP];                                           // producer p: first perspective (range-relative) of the lattice it is
                                                               // working on; everything of ITS lattices below that is in the rings;
                                                               // 0xFFFFFFFF = it has no lattice left
    uint32_t cons[NS];                                         // storer s: first element (from org) it has not taken yet
    uint32_t pcons[NPW];                                       // positions wave w: first perspective whose position it has not written yet
    uint32_t abort;
};

// A cut point of a lattice range into G = 1 << LG parts of equal perspective count: the first lattice e in
// [e_begin, e_end] with offsets[e] - offsets[e_begin] >= cut_target(total, k, LG).  One wavefront, 64-ary search (three
// rounds of vector loads for 65 536 lattices); the result is wave-uniform.  k_scan_final writes the same numbers for
// the whole batch as a by-product; this serves lattice sub-ranges and offsets that did not come from the scan.
__device__ __forceinline__ int64_t find_cut(const int64_t* __restrict__ offsets, int64_t e_begin, int64_t e_end, int k, int LG, int lane) {
    const int64_t off0 = offsets[e_begin], total = offsets[e_end] - off0;
    const int64_t target = off0 + cut_target(total, k, LG);
    int64_t lo = e_begin, hi = e_end;                         // answer in [lo, hi]; offsets[hi] >= target always
    while (lo < hi) {
        const int64_t span = hi - lo;
        const int64_t stepw = (span + 62) / 63;               // probes lo + i*stepw, i = 0..63: lane 63 reaches hi (63*stepw >= span)
        int64_t e = lo + (int64_t)lane * stepw;
        e = e < hi ? e : hi;
        const bool ge = offsets[e] >= target;
        const uint64_t m = __ballot(ge);                      // never empty: lane 63 probes hi
        if (!m) { lo = hi; break; }
        const int f = (int)__ffsll((long long)m) - 1;
        int64_t ef = lo + (int64_t)f * stepw;
        ef = ef < hi ? ef : hi;
        const int64_t new_lo = f == 0 ? lo : (lo + (int64_t)(f - 1) * stepw + 1);
        if (ef == lo) { hi = lo; break; }
        lo = new_lo < ef ? new_lo : ef;
        hi = ef;
    }
    return lo;
}
// The compile-time shape of one instantiation of the kernel.  NPW: positions waves (chunks of 1 KiB dealt round-robin among them)
template <int D_, typename OutT, int NS_, int NP_, int CPW_, int RB_LOG, int RP_LOG, int NPW_>
struct StreamShape {
    using L = Lat<D_>;
    using Out = OutT;
    using Lds = StreamLds<D_, NS_, NP_, RB_LOG, RP_LOG, NPW_>;
    static constexpr int D = D_, NS = NS_, NP = NP_, CPW = CPW_, NPW = NPW_, NQ = L::NQ;
    static constexpr int VEC = 16 / (int)sizeof(OutT);       // elements per 16-byte lane store
    static constexpr int EPC = 64 * VEC;                     // elements per chunk (one wave store instruction = 1 KiB)
    static constexpr int LPD = 32 / VEC;                     // lanes that share one ring dword
    static constexpr uint32_t RING_BITS = 32u << RB_LOG, BMASK = (1u << RB_LOG) - 1u, RP = 1u << RP_LOG, PMASK = RP - 1u;
    // WHOLE: a lattice's whole stack (2d^2 hits of 2d^2 bits each at most) fits into the ring beside what the storers may lag
    // behind: the producer asks for room once per lattice.  Otherwise (d >= 19) it asks pass by pass (64 hits) and publishes its
    // progress after every pass -- the consumers must be able to take the first passes of a lattice for the last ones to find room.
    // Per-pass publishing costs a producer ~14 % (5290 against 4640 cycles per d=7 lattice, profiles/r04_stream_tune_ab_passes.txt).
    static constexpr bool WHOLE = (uint32_t)NQ * NQ + 2u * NS * CPW * EPC + 4096u < RING_BITS;
    static_assert(64u * (uint32_t)NQ + 2u * NS * CPW * EPC + 4096u < RING_BITS, "bit ring too small for this lattice size");
    static_assert((uint32_t)NQ + 512u < RP, "position ring too small");
};
// What a workgroup knows once its range is set up (stream_setup); the same in every wave
template <typename OutT>
struct StreamCtx {
    const uint64_t* vp; int64_t N; const int64_t* offsets; OutT* out; int32_t* pos; int* err;   // the kernel's arguments
    int64_t off0, e_lo, e_stop;       // offsets[e_begin]; first lattice of the range; lattices from e_stop on are not written
    int64_t Q0, QT;                   // first perspective of the range; lattices are produced while they start in front of QT
    StreamRange r;
};
// Diagnostic builds only (STATS = true, tools/stream_tune.hip): every wave leaves {cycles alive, cycles waiting, begin << 32 |
// end on the 100 MHz clock, items | stamps << 16} in stats[(block * waves + wave) * 4 ..]; waiting = storers and positions
// waves: for production, producers: for ring room.  Stamps, in 10 ns units since the wave began -- storers: when the first
// trip began; producers: 16 bits each for range known, first lattice loaded, first lattice in the ring.
template <bool STATS>
struct StreamStats {                                           // the library's form: empty
    __device__ __forceinline__ unsigned long long now() const { return 0; }
    __device__ __forceinline__ void waited(unsigned long long) {}
    __device__ __forceinline__ void item() {}
    __device__ __forceinline__ void trip() {}
    __device__ __forceinline__ void range_known() {}
    __device__ __forceinline__ void lattice_loaded() {}
    __device__ __forceinline__ void lattice_in_ring() {}
    __device__ __forceinline__ void out(unsigned long long*, int, int) const {}
};
template <>
struct StreamStats<true> {
    unsigned long long t_begin, t_rt, t_wait = 0, n_items = 0, t_first = 0;
    __device__ __forceinline__ unsigned long long since() const { return __builtin_amdgcn_s_memrealtime() - t_rt; }
    __device__ __forceinline__ StreamStats() { t_begin = __builtin_readcyclecounter(); t_rt = __builtin_amdgcn_s_memrealtime(); }
    __device__ __forceinline__ unsigned long long now() const { return __builtin_readcyclecounter(); }
    __device__ __forceinline__ void waited(unsigned long long t0) { t_wait += now() - t0; }
    __device__ __forceinline__ void item() { ++n_items; }
    __device__ __forceinline__ void trip() { if (!n_items) t_first = since(); ++n_items; }
    __device__ __forceinline__ void range_known() { t_first = since() & 0xFFFFull; }
    __device__ __forceinline__ void lattice_loaded() { if (!n_items) t_first |= (since() & 0xFFFFull) << 16; ++n_items; }
    __device__ __forceinline__ void lattice_in_ring() { if (n_items == 1 && !(t_first >> 32)) t_first |= (since() & 0xFFFFull) << 32; }
    __device__ __forceinline__ void out(unsigned long long* stats, int waves, int wave) const {    // (lane 0 only)
        unsigned long long* o = stats + ((size_t)blockIdx.x * waves + wave) * 4;
        o[0] = now() - t_begin; o[1] = t_wait;
        o[2] = (t_rt << 32) | (__builtin_amdgcn_s_memrealtime() & 0xFFFFFFFFull); o[3] = (n_items & 0xFFFFull) | (t_first << 16);
    }
};
// A wave gives up: its workgroup's other waves see `abort` in their own waits and leave, the host sees the latch
__device__ __forceinline__ void give_up(uint32_t& abort, int* err, int lane) {
    if (lane == 0) { __hip_atomic_store(&abort, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); atomicOr(err, ERR_INTERNAL); }
}
// The bounded wait of every role: poll pred() (wave-uniform; it reads the other waves' hand-off words), s_sleep SLEEP
// between two looks.  False = the workgroup gave up -- another wave did, or this one after STREAM_SPIN_LIMIT looks -- and
// the caller returns.  The time spent here is what StreamStats reports as waiting.
template <int SLEEP, class Stats, class Pred>
__device__ __forceinline__ bool wait_until(uint32_t& abort, int* err, int lane, Stats& st, Pred&& pred) {
    const unsigned long long t0 = st.now();
    for (int spin = 0; spin < STREAM_SPIN_LIMIT; ++spin) {
        if (pred()) { lds_after_peek(); st.waited(t0); return true; }
        if (lds_peek(abort)) return false;
        __builtin_amdgcn_s_sleep(SLEEP);
    }
    give_up(abort, err, lane);
    return false;
}
// Perspectives [0, produced()) of the range are complete in the rings: lattices are dealt to the producers round-robin
// and every producer works through its own in order, so every lattice that starts below the smallest `pq` is done (one
// LDS read by NP lanes, the minimum on the scalar unit; wave-uniform).  0xFFFFFFFF = everything.
template <int NP>
__device__ __forceinline__ uint32_t produced(const uint32_t* pq, int lane) {
    uint32_t v = 0xFFFFFFFFu;
    if (lane < NP) v = __hip_atomic_load(&pq[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    uint32_t m = 0xFFFFFFFFu;
#pragma unroll
    for (int l = 0; l < NP; ++l) { const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)v, l); m = x < m ? x : m; }
    return m;
}

// ---- the workgroup's range (uniform over the workgroup; false = nothing to do, or refused and latched: every wave
// returns).  Also clears the rings and the hand-off words.  The stack is cut into 1 << lg FINE parts of equal perspective
// count, RR of them per workgroup on average (a power of two): cut points from the scan's table `split` (k_scan_final),
// or -- no table of these offsets: a lattice sub-range, or offsets that did not come with the scan -- found here by waves 1-3.
// The shares are NOT equal ("unequal shares"): the CUs of the odd XCDs of an MI355X store this stream ~20 %
// slower than those of the even ones, so every pair of shares is cut into a LARGE and a SMALL slot (slot_fine_parts).
// Workgroups b and b ^ 1 own the two slots of pair b >> 1 and settle between themselves who takes which: the one on an even
// XCD (HW_REG_XCC_ID; blockIdx.x says nothing about the XCD) prefers the large slot, the first of the two to arrive at the
// pair's word gets what it prefers, the second takes the other (pair_claim, stream_range.hpp).  One returning atomic per
// workgroup on a word that only its partner shares: nothing is contended, gridDim.x workgroups take gridDim.x different
// slots whatever the dispatcher does, and under round-robin dispatch b and b + 1 sit on XCDs of opposite parity, so the even
// XCD always gets the large slot.  The second arriver stores 0: a launch leaves the words as it found them (graph replay).
// Equal shares (slot = blockIdx.x, which is the same pair) where the launch is not bound by the stores: small stacks, and
// the host passes bias = 0 for d <= 5.
//
// The start of a launch is a chain of dependent loads on an idle chip, so it is kept to two rounds:
//   1. with the atomic in flight: offsets[e_begin], offsets[e_end], the table's header and the pair's cut points -- both ends
//      and the middle for either bias; they serve whichever kind the atomic's answer names.  No table: three find_cut
//      searches side by side (waves 1-3), which need nothing of the atomic either;
//   2. offsets[e_lo], offsets[e_hi] -- and, issued right behind them (`prefetch`), the producers' first planes and offsets.
// slots: one zeroed word per pair, PAIR_WORD_STRIDE dwords apart, that no other launch in flight uses.
// force_parity (tq_debug_force_xcc_parity): -1 = the XCD's own parity, 0 / 1 = every workgroup claims that one, 2 = inverted
template <class K, class Prefetch>
__device__ __forceinline__ bool stream_setup(StreamCtx<typename K::Out>& c, typename K::Lds& S, int64_t capacity,
                                             int64_t e_begin, int64_t e_end, const int32_t* __restrict__ split, int lg, int bias,
                                             unsigned int* __restrict__ slots, int force_parity, int wave, int lane, Prefetch&& prefetch) {
    using L = typename K::L;
    static_assert(K::NS + K::NPW + K::NP >= 4, "waves 1-3 find the pair's cut points");
    const int RR = (1 << lg) / (int)gridDim.x;
    const int pair = (int)(blockIdx.x >> 1);
    // the claim: the kernel's first memory instruction, before anything is known about the stack.  A small stack ignores the
    // answer (below), but both arrivals happen, so the word returns to 0 all the same.
    const bool claim = slots && bias > 0 && !(gridDim.x & 1u);
    int prefers_large = !(blockIdx.x & 1);
    unsigned old = 0u;
    if (threadIdx.x == 0 && claim) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        if (force_parity >= 0) xcc = force_parity < 2 ? (unsigned)force_parity : (xcc ^ 1u);
        prefers_large = !(xcc & 1u);
        // (an index the compiler cannot prove uniform: with a uniform address it folds the wave's adds into one and
        // broadcasts the answer, which waits for the atomic on the spot)
        unsigned word = (unsigned)(pair * PAIR_WORD_STRIDE);
        asm volatile("" : "+v"(word));
        old = atomicAdd(&slots[word], pair_claim(0u, prefers_large).add);
    }
    if (!claim || bias >= RR) bias = 0;
    // round 1, with the atomic in flight: one vector load each, one lane per word (scalar loads would be waited for one by
    // one) -- the two offsets; the pair's cut points -- [f_lo, f_mid) is its large slot, [f_mid, f_hi) its small one, f_mid
    // for equal shares and for this bias -- and the table's header.  (Wave 0 has the atomic's answer when it has these:
    // a wave's loads and returning atomics come back in issue order.  It has nothing else to do until then.)
    int f_lo, f_eq, f_bias, f_hi;
    slot_fine_parts(1, pair, RR, 0, f_lo, f_eq);
    slot_fine_parts(0, pair, RR, bias, f_bias, f_hi);
    const int64_t ow = c.offsets[lane == 1 ? e_end : e_begin];
    int32_t tw = 0;
    if (split) {
        int fi = cut_header_at(lg) + (lane >= 4 && lane < 4 + CUT_HEADER_WORDS ? lane - 4 : 0);
        fi = lane == 0 ? f_lo : fi;  fi = lane == 1 ? f_eq : fi;  fi = lane == 2 ? f_bias : fi;  fi = lane == 3 ? f_hi : fi;
        tw = split[fi];
    }
    // A table is followed only if it is the table of THESE offsets over THIS lattice range: its header (cut_points.hpp)
    // holds the stack's perspective count and the last lattice, and a scan covers [0, N].  The handle matches tables to
    // offsets POINTERS; a caller who refilled a scanned array hands in a table of another stack -- all zero, say, which
    // would leave the stack unwritten with nothing latched.  Such a table is not followed: the workgroups find their cut
    // points themselves.
    const int64_t off0 = (int64_t)readlane64((uint64_t)ow, 0);
    int64_t p_all = (int64_t)readlane64((uint64_t)ow, 1) - off0;    // perspectives of the whole stack
    int64_t cut_lo = __builtin_amdgcn_readlane(tw, 0), cut_eq = __builtin_amdgcn_readlane(tw, 1), cut_bias = __builtin_amdgcn_readlane(tw, 2),
            cut_hi = __builtin_amdgcn_readlane(tw, 3);
    const bool by_tab = split && cut_header_words_match(__builtin_amdgcn_readlane(tw, 4), __builtin_amdgcn_readlane(tw, 5),
                                                        __builtin_amdgcn_readlane(tw, 6), p_all, e_begin, e_end);
    // a small stack is not bound by the stores: equal shares
    if (p_all * (int64_t)(K::NQ * sizeof(typename K::Out)) < (int64_t)(64 << 20)) bias = 0;
    int64_t cut_mid = bias ? cut_bias : cut_eq;
    __shared__ int64_t cut_s[3];
    __shared__ int kind_s;
    if (!by_tab && wave >= 1 && wave <= 3) {                 // (not wave 0: its loads come back behind the atomic)
        const int64_t e = find_cut(c.offsets, e_begin, e_end, wave == 1 ? f_lo : (wave == 2 ? (bias ? f_bias : f_eq) : f_hi), lg, lane);
        if (lane == 0) cut_s[wave - 1] = e;
    }
    // (the rings and hand-off words meanwhile: they do not depend on the range)
    constexpr uint32_t THREADS = 64u * (K::NS + K::NPW + K::NP);    // (blockDim.x would be one more load to wait for)
    for (uint32_t i = threadIdx.x; i < (K::BMASK + 1u) / 4; i += THREADS) reinterpret_cast<uint4*>(S.bits)[i] = make_uint4(0u, 0u, 0u, 0u);
    if (threadIdx.x == 0) S.abort = 0u;
    if (threadIdx.x < K::NP) S.pq[threadIdx.x] = 0u;
    if (threadIdx.x < K::NPW) S.pcons[threadIdx.x] = 0u;
    if (threadIdx.x < K::NS) S.cons[threadIdx.x] = 0u;       // (a lower bound of "the first element storer s has not taken yet")
    if (threadIdx.x == 0) {                                  // the atomic's answer
        const PairClaim pc = pair_claim(old, prefers_large);
        if (claim && pc.second) __hip_atomic_store(&slots[pair * PAIR_WORD_STRIDE], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        kind_s = claim ? pc.kind : prefers_large;
    }
    __syncthreads();
    int kind = kind_s;
    if (kind < 0) {                                          // the pair's word was not zero when the launch began
        if (threadIdx.x == 0) atomicOr(c.err, ERR_INTERNAL);
        return false;
    }
    if (!bias) kind = !(blockIdx.x & 1);                     // equal shares: slot = blockIdx.x
    if (!by_tab) { cut_lo = cut_s[0]; cut_mid = cut_s[1]; cut_hi = cut_s[2]; }
    int64_t e_lo = kind ? cut_lo : cut_mid, e_hi = kind ? cut_mid : cut_hi;
    e_lo = e_lo < e_begin ? e_begin : (e_lo > e_end ? e_end : e_lo);       // whatever the table holds, stay inside the range
    e_hi = e_hi < e_lo ? e_lo : (e_hi > e_end ? e_end : e_hi);
    int64_t e_stop = e_end;
    if (p_all > capacity) {                                  // stack does not fit: only the lattices that fit whole are written
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(c.err, ERR_CAPACITY);
        int64_t lo = e_begin, hi = e_end;                    // largest e with offsets[e] - off0 <= capacity
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) >> 1;
            if (c.offsets[mid] - off0 <= capacity) lo = mid; else hi = mid - 1;
        }
        e_stop = lo;
        p_all = c.offsets[e_stop] - off0;
        e_lo = e_lo < e_stop ? e_lo : e_stop;
        e_hi = e_hi < e_stop ? e_hi : e_stop;
    }
    // round 2: one vector load again, and behind it the producers' first planes and offsets
    const int64_t qw = c.offsets[lane == 1 ? e_hi : e_lo];
    prefetch(e_lo, e_stop);
    const int64_t Q0 = (int64_t)readlane64((uint64_t)qw, 0) - off0, Q1 = (int64_t)readlane64((uint64_t)qw, 1) - off0;    // perspective range [Q0, Q1)
    // The offsets come from the caller: whatever they hold, nothing is stored outside [0, p_all) perspectives.  Offsets
    // that are not monotone over this workgroup's cut points are refused here; offsets that do not match the lattices'
    // own hit counts are refused by the producer that meets the first such lattice.
    if (Q0 < 0 || Q1 < Q0 || Q1 > p_all) {
        if (threadIdx.x == 0) atomicOr(c.err, ERR_INTERNAL);
        return false;
    }
    if (p_all == 0 && e_stop == e_end) {                     // "the stack is empty": true only if no lattice of the range has a hit
        for (int64_t e = e_begin + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < e_end; e += (int64_t)gridDim.x * blockDim.x) {
            typename L::B v, pl;
#pragma unroll
            for (int k = 0; k < L::W; ++k) { v.w[k] = c.vp[(int64_t)k * c.N + e]; pl.w[k] = c.vp[((int64_t)L::W + k) * c.N + e]; }
            if (L::persp_count(v, pl) != 0) atomicOr(c.err, ERR_INTERNAL);
        }
        return false;
    }
    c.r = stream_range(Q0, Q1, p_all, K::NQ, (int)sizeof(typename K::Out), c.pos != nullptr);
    c.off0 = off0; c.e_lo = e_lo; c.e_stop = e_stop; c.Q0 = Q0; c.QT = Q1 + c.r.need_extra;
    return c.r.has_stack || c.r.has_pos;
}

// =========================================================== stack storer s
template <class K, class Stats>
__device__ __forceinline__ bool storer_wave(const StreamCtx<typename K::Out>& c, typename K::Lds& S, int s, int lane, Stats& st) {
    using OutT = typename K::Out;  using Enc = OutEnc<OutT>;
    constexpr int NS = K::NS, CPW = K::CPW, VEC = K::VEC, EPC = K::EPC;
    const uint32_t head = c.r.head, a0 = c.r.a0, a1 = c.r.a1;
    if (!c.r.has_stack) return false;
    __builtin_amdgcn_s_setprio(3);                           // store issue goes before the producers' arithmetic
    constexpr int U = CPW < 4 ? CPW : 4;                     // chunks per trip: one LDS round trip and one hand-back per U KiB
    static_assert(CPW % U == 0, "window must be a whole number of trips");
    const uint32_t nchunks = (a1 - a0 + EPC - 1) / EPC;
    const uint32_t lane_el = (uint32_t)lane * VEC;
    const int sh = (int)((a0 + lane_el) & 31u);              // a0 is a multiple of the line, EPC of 32: loop-invariant
    const bool zero_lane = (lane % K::LPD) == 0;
    char* __restrict__ obase = reinterpret_cast<char*>(c.out + c.r.org);
    uint32_t prod_c = 0;                                     // cached produced()
    // stream bit position (from org) up to which the stack is produced, saturating
    auto produced_bits = [&]() -> uint32_t { return prod_c == 0xFFFFFFFFu ? 0xFFFFFFFFu : head + prod_c * (uint32_t)K::NQ; };
    bool first = true;
    for (uint32_t w = (uint32_t)s; w * CPW < nchunks; w += NS) {
        for (uint32_t cb = w * CPW; cb < (w + 1) * CPW && cb < nchunks; cb += U) {
            const uint32_t el0 = a0 + cb * EPC;
            uint32_t end = el0 + U * EPC;
            end = end < a1 ? end : a1;
            if (produced_bits() < end &&                     // wait until the trip's last element is produced
                !wait_until<4>(S.abort, c.err, lane, st, [&] { prod_c = produced<K::NP>(S.pq, lane); return produced_bits() >= end; })) return false;
            st.trip();
            if (first) {
                first = false;
                if (s == 0 && a0 && lane < (int)(a0 / 32u)) S.bits[lane] = 0u;   // ring words in front of a0 (stored by the previous range)
            }
            uint32_t wv[U], idx[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                idx[u] = ((el0 + (uint32_t)u * EPC + lane_el) >> 5) & K::BMASK;
                wv[u] = S.bits[idx[u]];
            }
            if (zero_lane) {                                 // hand the words back zeroed
#pragma unroll
                for (int u = 0; u < U; ++u) S.bits[idx[u]] = 0u;
            }
            if (el0 + U * EPC <= a1) {                       // whole trip inside the range: U x 1 KiB
#pragma unroll
                for (int u = 0; u < U; ++u)
                    *reinterpret_cast<u32x4*>(obase + (size_t)(el0 + (uint32_t)u * EPC + lane_el) * sizeof(OutT)) = expand_bits<OutT>(wv[u] >> sh);
            } else {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const uint32_t el = el0 + (uint32_t)u * EPC + lane_el;
                    const u32x4 val = expand_bits<OutT>(wv[u] >> sh);
                    if (el + VEC <= a1) {
                        *reinterpret_cast<u32x4*>(obase + (size_t)el * sizeof(OutT)) = val;
                    } else if (el < a1) {                    // the stack ends inside this lane's 16 bytes (last range only)
                        const int nel = (int)(a1 - el);
                        if (Enc::BITS == 32) {
                            for (int j = 0; j < nel; ++j) reinterpret_cast<uint32_t*>(obase)[el + j] = val[j];
                        } else if (Enc::BITS == 16) {
                            for (int j = 0; j < nel; ++j) reinterpret_cast<uint16_t*>(obase)[el + j] = (uint16_t)(val[j >> 1] >> (16 * (j & 1)));
                        } else {
                            for (int j = 0; j < nel; ++j) reinterpret_cast<uint8_t*>(obase)[el + j] = (uint8_t)(val[j >> 2] >> (8 * (j & 3)));
                        }
                    }
                }
            }
            // first element this storer has not taken yet: the next trip of this window, or the next window of its own
            uint32_t nb = cb + U;
            if (nb % CPW == 0) nb += (uint32_t)(NS - 1) * CPW;
            lds_publish(S.cons[s], nb < nchunks ? a0 + nb * EPC : 0xFFFFFFFFu, lane);
        }
    }
    lds_publish(S.cons[s], 0xFFFFFFFFu, lane);
    return true;
}

// =========================================================== positions storer pw (1 KiB chunks, round-robin over NPW waves)
template <class K, class Stats>
__device__ __forceinline__ bool positions_wave(const StreamCtx<typename K::Out>& c, typename K::Lds& S, int pw, int lane, Stats& st) {
    constexpr int NPW = K::NPW;
    const uint32_t phead = c.r.phead, pa0 = c.r.pa0, pa1 = c.r.pa1;
    if (!c.r.has_pos) return false;
    int32_t* __restrict__ pbase = c.pos + c.r.porg;
    const uint32_t nchunks = (pa1 - pa0 + 255u) / 256u;
    for (uint32_t ch = (uint32_t)pw; ch < nchunks; ch += NPW) {
        const uint32_t x0 = pa0 + ch * 256u;
        const uint32_t x_end = x0 + 256u < pa1 ? x0 + 256u : pa1;
        const uint32_t need = (x_end - phead + 2u) / 3u;
        st.item();
        if (!wait_until<(NPW > 1 ? 8 : 16)>(S.abort, c.err, lane, st, [&] { return produced<K::NP>(S.pq, lane) >= need; })) return false;
        const uint32_t x = x0 + 4u * (uint32_t)lane;
        if (x < x_end) {
            int o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t t = x + j - phead, q = t / 3u;
                o[j] = (int)((S.posr[q & K::PMASK] >> (8u * (t - 3u * q))) & 255u);
            }
            if (x + 4u <= x_end) *reinterpret_cast<int4*>(pbase + x) = make_int4(o[0], o[1], o[2], o[3]);
            else for (uint32_t j = 0; x + j < x_end; ++j) pbase[x + j] = o[j];
        }
        // low-water mark: the first perspective of this wave's NEXT chunk (everything below it, of this wave's, is written)
        const uint32_t nc = ch + NPW;
        lds_publish(S.pcons[pw], nc < nchunks ? (pa0 + nc * 256u - phead) / 3u : 0xFFFFFFFFu, lane);
    }
    lds_publish(S.pcons[pw], 0xFFFFFFFFu, lane);
    return true;
}

// =========================================================== producer
// tables of one lattice: rotated planes (ballot), row-rolled planes, hit list (+ has_pos: its positions, into ring `posr` from q0 on)
template <class K>
__device__ __forceinline__ void build_tables(LatTables<K::D>& T, uint32_t* posr, bool has_pos, const typename K::L::B& v, const typename K::L::B& pl,
                                             const typename K::L::B& e0, const typename K::L::B& e1, int n0, uint32_t q0, int lane) {
    using L = typename K::L;  using PS = PStream<K::D>;  using B = typename L::B;
    constexpr int D = K::D, DD = L::DD, W = L::W;
    B rv, rp;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const int o = 64 * k + lane;
        const bool inb = o < DD;
        const int oc = inb ? o : 0;
        rv.w[k] = __ballot(inb && v.get(PS::rot_src_v(oc)));
        rp.w[k] = __ballot(inb && pl.get(PS::rot_src_p(oc)));
    }
    for (int t = lane; t < 4 * D; t += 64) {                 // one lane per (plane, row amount): 4 d entries (more than 64 from d = 17 on)
        const int sel = t / D, k = t - sel * D;
        B src;
#pragma unroll
        for (int w = 0; w < W; ++w) src.w[w] = sel == 0 ? v.w[w] : (sel == 1 ? pl.w[w] : (sel == 2 ? rv.w[w] : rp.w[w]));
        const B r = (src.shl(k * D) | src.shr(DD - k * D)) & L::full();
#pragma unroll
        for (int w = 0; w < W; ++w) T.rr[sel][k][w] = r.w[w];
    }
    for (int c = lane; c < K::NQ; c += 64) {
        const int l = c >= DD, bit = c - l * DD;
        if (l ? e1.get(bit) : e0.get(bit)) {
            const int row = bit / D, col = bit - row * D;
            const int k = l ? n0 + e1.rank(bit) : e0.rank(bit);
            const uint32_t hp = (uint32_t)l | ((uint32_t)row << 8) | ((uint32_t)col << 16);
            T.hpos[k] = hp;
            if (has_pos) posr[(q0 + (uint32_t)k) & K::PMASK] = hp;
        }
    }
}
// hit k of the lattice: its perspective as two bit-planes (two row-rolled planes of the lattice's table, two masked
// column rolls), OR-ed (has_stack) into the ring at bit position `pos`
template <class K>
__device__ __forceinline__ void emit_hit(const ProdTables<K::D>& PT, uint32_t* bits, bool has_stack, int k, uint32_t pos) {
    using PS = PStream<K::D>;
    typename K::L::B a, c, low;
    const uint32_t hp = PT.t.hpos[k];
    const int layer = (int)(hp & 255u), i = (int)((hp >> 8) & 255u), jj = (int)(hp >> 16);
    int rs, cs;
    PS::hit_shifts(layer, i, jj, rs, cs);                    // (moving this to the hit-list stage, per qubit lane, was measured: no gain)
#pragma unroll
    for (int w = 0; w < K::L::W; ++w) { a.w[w] = PT.t.rr[2 * layer][rs][w]; c.w[w] = PT.t.rr[2 * layer + 1][rs][w]; low.w[w] = PT.low[cs][w]; }
    const auto ov = PS::roll_cols_masked(a, cs, low), op = PS::roll_cols_masked(c, cs, low);
    if (has_stack) emit_at<K::D>(pos, ov, op, [&](uint32_t idx, uint32_t val) { atomicOr(&bits[idx & K::BMASK], val); });
}
// The planes and offsets of a producer wave's next 64 lattices, one lattice per lane (e_lo + Lb + lane * NP + p), in one
// round of vector loads.  The first round is issued by the set-up, in front of its own last loads: the addresses need the
// range's first lattice only, the values are used when the range is known.
template <class K>
struct ProducerLoads {
    uint64_t vv[K::L::W], pp[K::L::W];
    int64_t oo, oo1;                                           // offsets[e], offsets[e + 1]
    bool in;                                                   // the lane has a lattice in front of e_stop
    __device__ __forceinline__ void load(const uint64_t* __restrict__ vp, int64_t N, const int64_t* __restrict__ offsets, int64_t e_lo,
                                         int64_t e_stop, int64_t Lb, int p, int lane) {
        constexpr int W = K::L::W;
        const int64_t e_l = e_lo + Lb + (int64_t)lane * K::NP + p;
        in = e_l < e_stop;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            vv[k] = in ? vp[(int64_t)k * N + e_l] : 0ull;
            pp[k] = in ? vp[((int64_t)W + k) * N + e_l] : 0ull;
        }
        oo = in ? offsets[e_l] : 0;
        oo1 = in ? offsets[e_l + 1] : 0;
    }
};
// Producer p takes the lattices e_lo + p, e_lo + p + NP, ... of the range, one at a time, 64 hits per pass.  ld: its first
// 64 lattices, loaded by the set-up
template <class K, class Stats>
__device__ __forceinline__ bool producer_wave(const StreamCtx<typename K::Out>& c, typename K::Lds& S, int p, int lane, Stats& st,
                                              ProducerLoads<K>& ld) {
    using L = typename K::L;  using B = typename L::B;
    constexpr int W = L::W, NP = K::NP, NQ = K::NQ;
    const bool has_stack = c.r.has_stack, has_pos = c.r.has_pos;
    const uint32_t head = c.r.head;
    st.range_known();
    ProdTables<K::D>& PT = S.tab[p];
    if (lane < K::D) {                                       // column masks: the same for every lattice
        const B m = L::lowcols(lane);
#pragma unroll
        for (int w = 0; w < W; ++w) PT.low[lane][w] = m.w[w];
    }
    // Room in the rings for the stream bits below `bits_end` and the positions below `q_end`: everything below the storers'
    // low-water marks has been handed back.  The marks are cached: while the storers keep up the ring is nearly empty and one
    // look lasts for dozens of lattices.  Wave-uniform; false = the workgroup gave up (the caller returns)
    uint32_t lw_c = c.r.a0, pc_c = 0u;
    auto wait_room = [&](uint32_t bits_end, uint32_t q_end) __attribute__((always_inline)) -> bool {
        auto fits = [&]() {
            return (lw_c == 0xFFFFFFFFu || bits_end + 64u <= lw_c + K::RING_BITS) && (!has_pos || pc_c == 0xFFFFFFFFu || q_end <= pc_c + K::RP);
        };
        return fits() || wait_until<8>(S.abort, c.err, lane, st, [&] {
            lw_c = has_stack ? lds_min<K::NS>(S.cons, lane) : 0xFFFFFFFFu;
            if (has_pos) pc_c = lds_min<K::NPW>(S.pcons, lane);
            return fits();
        });
    };
    for (int64_t Lb = 0;; Lb += 64 * NP) {
        if (Lb) ld.load(c.vp, c.N, c.offsets, c.e_lo, c.e_stop, Lb, p, lane);
        const bool in = ld.in;
        const uint64_t (&vv)[W] = ld.vv, (&pp)[W] = ld.pp;
        const int64_t oo = in ? ld.oo - c.off0 : (int64_t)0x7fffffffffffffffll;
        const int64_t oo1 = in ? ld.oo1 - c.off0 : (int64_t)0x7fffffffffffffffll;
        const uint64_t inmask = __ballot(in && oo < c.QT);   // offsets are monotone: a prefix of the lanes
        if (!inmask) break;
        const int cnt = __popcll(inmask);
        for (int j = 0; j < cnt; ++j) {
            B v, pl, e0, e1;
#pragma unroll
            for (int k = 0; k < W; ++k) { v.w[k] = readlane64(vv[k], j); pl.w[k] = readlane64(pp[k], j); }
            L::hit_masks(v, pl, e0, e1);
            const int n0 = e0.popc();
            const int n = n0 + e1.popc();
            // the offsets must be the scan of THESE lattices' hit counts; a table that is not (stale, shifted, from another
            // batch) is refused at the first lattice that disagrees, before anything of it reaches the rings
            if (readlane64((uint64_t)oo1, j) - readlane64((uint64_t)oo, j) != (uint64_t)n) { give_up(S.abort, c.err, lane); return false; }
            if (n == 0) continue;
            const uint32_t q0 = (uint32_t)((int64_t)readlane64((uint64_t)oo, j) - c.Q0);
            const uint32_t bit0 = head + q0 * (uint32_t)NQ;
            st.lattice_loaded();
            // this wave's earlier lattices are in the rings (its LDS operations execute in issue order): say so
            lds_publish(S.pq[p], q0, lane);
            // room.  Positions: the whole lattice (n <= 2d^2 < ring - 512); bits: the whole lattice, or (d >= 19) its first 64 hits
            const uint32_t pass1 = (uint32_t)((K::WHOLE || n < 64) ? n : 64);
            if (!wait_room(bit0 + pass1 * (uint32_t)NQ, q0 + (uint32_t)n)) return false;
            build_tables<K>(PT.t, S.posr, has_pos, v, pl, e0, e1, n0, q0, lane);
            wave_lds_sync();
            // one lane per hit, 64 hits per pass.  d >= 19 (!WHOLE): after every pass the wave says how far the lattice is (the
            // consumers may take it) and asks for the next pass's room -- 2d^2 hits x 2d^2 bits are more than the ring holds
            for (int kb = 0; kb < n; kb += 64) {
                if (!K::WHOLE && kb) {
                    lds_publish(S.pq[p], q0 + (uint32_t)kb, lane);
                    const uint32_t upto = (uint32_t)(n < kb + 64 ? n : kb + 64);
                    if (!wait_room(bit0 + upto * (uint32_t)NQ, q0 + (uint32_t)n)) return false;
                }
                const int k = kb + lane;
                if (k >= n) continue;
                emit_hit<K>(PT, S.bits, has_stack, k, head + (q0 + (uint32_t)k) * (uint32_t)NQ);
            }
            wave_lds_sync();                                 // the tables are rewritten by the next lattice
            st.lattice_in_ring();
        }
        if (cnt < 64) break;
    }
    lds_publish(S.pq[p], 0xFFFFFFFFu, lane);                 // no lattice left: everything of this wave is in the rings
    return true;
}

// split / lg / bias / slots / force_parity: see stream_setup.  stats: see StreamStats
template <int D, typename OutT, int NS, int NP, int CPW, int RB_LOG, int RP_LOG, bool STATS = false, int NPW = 1>
__global__ __launch_bounds__(64 * (NS + NPW + NP)) void k_persp_stream(
        const uint64_t* __restrict__ vp, int64_t N, const int64_t* __restrict__ offsets, OutT* __restrict__ out, int32_t* __restrict__ pos,
        int64_t capacity, int* __restrict__ err, int64_t e_begin, int64_t e_end, const int32_t* __restrict__ split, int lg, int bias,
        unsigned int* __restrict__ slots, int force_parity, unsigned long long* __restrict__ stats = nullptr) {
    using K = StreamShape<D, OutT, NS, NP, CPW, RB_LOG, RP_LOG, NPW>;
    StreamStats<STATS> st;
    __shared__ typename K::Lds S;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    StreamCtx<OutT> c{vp, N, offsets, out, pos, err};
    ProducerLoads<K> ld;
    if (!stream_setup<K>(c, S, capacity, e_begin, e_end, split, lg, bias, slots, force_parity, wave, lane, [&](int64_t e_lo, int64_t e_stop) {
            if (wave >= NS + NPW) ld.load(vp, N, offsets, e_lo, e_stop, 0, wave - NS - NPW, lane);
        })) return;
    // (false: nothing to do for this role, or the workgroup gave up.  The producer stands first: the kernel is at its SGPR limit,
    // and with the storer first the producer's wave-uniform bitset words are parked in vector lanes: +7 % cycles per lattice, d = 19)
    const bool done = wave >= NS + NPW ? producer_wave<K>(c, S, wave - NS - NPW, lane, st, ld)
                    : wave < NS        ? storer_wave<K>(c, S, wave, lane, st)
                                       : positions_wave<K>(c, S, wave - NS, lane, st);
    if (done && lane == 0) st.out(stats, NS + NPW + NP, wave);
}

}  // namespace tq
