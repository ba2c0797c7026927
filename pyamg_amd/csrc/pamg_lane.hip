// pamg_lane.hip -- the LANE-PARALLEL ("fast order") Gauss-Seidel / SOR sweep: layout in pamg_lane_plan.h.
//
// Same rows in the same order as amg_core::gauss_seidel (relaxation.h:48-76) / sor_gauss_seidel (:116-145) /
// bsr_gauss_seidel with 1x1 blocks (:185-266) -- the dependency DAG of the sequential sweep is kept, so the iterates
// are the reference's up to rounding -- but nothing of the row sum's order is: L lanes of a wave share a row, each adds
// its K products, the lanes are added across the wave ("wavefront-wide segmented reduction per row"), and the row is
// finished with (b - sum) * (1 / a_ii) instead of the IEEE division.  What that buys: the order-exact sweeps spend
// ~0.9 us per dependency level BEHIND the last hand-off (LDS staging, barrier, 31..70-term in-order add chain, divide).
//
// ONE persistent launch per sweep; a group of 64 / L rows of one dependency level is the work of ONE wave, waves never
// meet (no LDS, no barrier).  The hand-off is the one of the granular exact sweep: the published 8-byte value is the
// flag (sentinel-filled buffer xs, write-through store -> polled L1-bypassing load).
//   static form : wave w takes groups w, w + W, w + 2W, ... (all W waves co-resident; a group only waits for groups
//                 with smaller numbers -> deadlock-free);
//   one-XCD form: small operators (vectors fit one XCD's L2).  The first workgroup to arrive claims its XCD, workgroups
//                 elsewhere leave, the rest draw groups from a ticket counter (two tickets ahead, taken in increasing
//                 order by running waves: complete for any placement) and publish with ordinary L2-resident stores.
// In the ticket form the static operands of a wave's NEXT group are requested before it starts to wait for the current one (the static form stopped
// doing that in round 5: - 1.4 % on level 1 of the 256^3 hierarchy; the ticket form WITHOUT it: level 2 0.705 -> 0.745 ms -- inside one XCD a poll
// costs little and the operands of the next group are the longer wait; profiles/r05_microbench_lane_prefetch_ab.txt).
//
// Round 5: the slab form (one slab of the visit order per XCD, hand-off through the XCD's L2 for operands of the own slab) is gone -- it never
// beat the plain static form (profiles/r04_microbench_lane_exp_{g,h}.json) --, rid / gate / 1 / a_ii of a slot row travel as ONE 16-byte record,
// and three forms of a shorter tail behind the last hand-off were built, measured and removed again (early products added one by one by
// v_readlane in a producer-level slot order; the last two / three early slots polled by every lane at one address each): the butterfly is not
// what a dependency level costs -- profiles/r05_microbench_lane_tail_*_not_kept.json, DESIGN 3.
#include "pamg_common.h"
#include "pamg_lane_plan.h"
#include "pamg_lanem_plan.h"
#include "pamg_tile_plan.h"
#include "pamg_wave.h"
#include "pamg_sweep_host.h"

namespace pamg {

// per slot row (group g, row r of the group): original row | NODIAG, the group's gate operand, 1 / a_ii -- ONE 16-byte request
struct alignas(16) LaneRec { int rid; int gate; int rd_lo; int rd_hi; };

struct LaneSched {
    int L = 0, K = 0, RPW = 0;
    int64_t ngroups = 0;
    int *d_cols = nullptr;
    LaneRec *d_rec = nullptr;
    void *d_vals = nullptr;
    long long *d_prof = nullptr;
    int64_t n_early = 0, n_old = 0, n_slots = 0;
    int64_t max_level_groups = 0;
    int last_grid = 0;              // workgroups of the last launch (diagnostics)
    int cap = 0;                    // co-resident workgroups per CU of this schedule's kernel (queried once)
    const void *cap_kernel = nullptr;
    size_t bytes = 0;
};

template <typename T>
struct LaneArgs {
    const int *cols;
    const T *vals;
    const LaneRec *rec;
    const T *x;            // OLD values (x itself, or its snapshot for structurally non-symmetric patterns)
    T *y;                  // destination (the live x)
    T *xs;                 // hand-off buffer, sentinel-filled
    const T *b;
    unsigned *err;         // spin bound hit
    unsigned *ticket;      // one-XCD form: [0] ticket counter, [1] home XCD + 1
    long long *prof;       // nullptr or [ngroups][4] time stamps
    int ngroups, nidle;
    int use_gate;          // != 0: a wave that runs ahead polls its gate operand first
    T omega;
};

template <typename T, int K>
struct LaneSet {
    int c[K];
    T v[K];
    int rid;
    T rd;
    int gate;
};

template <typename T> __device__ __forceinline__ T rec_rd(const int4 &q);
template <> __device__ __forceinline__ double rec_rd<double>(const int4 &q) { return __hiloint2double(q.w, q.z); }
template <> __device__ __forceinline__ float rec_rd<float>(const int4 &q) { return __int_as_float(q.z); }

template <typename T, int L, int K>
__device__ __forceinline__ void lane_load(const LaneArgs<T> &a, int g, LaneSet<T, K> &S)
{
    const int lane = threadIdx.x & 63;
    const size_t e0 = (size_t)g * (size_t)(K * 64) + (size_t)lane;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        S.c[k] = a.cols[e0 + (size_t)k * 64];
        S.v[k] = a.vals[e0 + (size_t)k * 64];
    }
    const size_t slot = (size_t)g * (size_t)(64 / L) + (size_t)(lane / L);
    const int4 q = reinterpret_cast<const int4 *>(a.rec)[slot];
    S.rid = q.x;
    S.gate = a.use_gate ? q.y : -1;
    S.rd = rec_rd<T>(q);
}

// one group, first half: request everything that depends on the group's static operands -- b, the row's own old value,
// and the first round of operand loads (early entries from the hand-off buffer, the others from x; both bypass the L1,
// other CUs write these lines during the launch; padding reads a per-wave idle element).  The caller requests the
// NEXT group's static operands right after this, so that waiting for these loads (the memory counter is in-order)
// never waits for those.
template <typename T, int K>
struct LaneDyn {
    T bv, xo;
    T xv[K];
    long long t0;
};

template <typename T, int EPI, int K>
__device__ __forceinline__ void lane_issue(const LaneArgs<T> &a, const LaneSet<T, K> &S, LaneDyn<T, K> &D, int idle)
{
    D.t0 = 0;
    if (a.prof && (threadIdx.x & 63) == 0) D.t0 = wall_clock64();
    const int row = S.rid < 0 ? 0 : (S.rid & LANE_MASK);
    D.bv = a.b[row];
    D.xo = T(0);
    if constexpr (EPI == EPI_SOR) D.xo = a.x[row];
    else if (S.rid & LANE_NODIAG) D.xo = a.x[row];             // (dummy rows have the bit set too: harmless)
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = S.c[k];
        const int col = c & LANE_MASK;
        const T *p = (c & LANE_NONE) ? a.x + idle : ((c & LANE_EARLY) ? a.xs + col : a.x + col);
        D.xv[k] = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// a wave that runs ahead: the sweep is still two or more dependency levels away while the gate operand is missing -- the
// whole wave polls that ONE value (one request per round) instead of all its operands
template <typename T>
__device__ __forceinline__ unsigned lane_gate_wait(const LaneArgs<T> &a, int gate)
{
    unsigned spins = 0;
    const T *gp = a.xs + gate;
    while (true) {
        const T gv = __hip_atomic_load(gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (Sentinel<T>::bits(gv) != Sentinel<T>::value) break;
        __builtin_amdgcn_s_sleep(2);
        if ((++spins & 1023u) == 0 && (spins > (1u << 21) || __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) break;
    }
    return spins;
}

template <typename T, int EPI, int MODE>
__device__ __forceinline__ void lane_publish(const LaneArgs<T> &a, int rid, T s, T bv, T rd, T xo)
{
    const int row = rid & LANE_MASK;
    const bool upd = !(rid & LANE_NODIAG);
    T v = (bv - s) * rd;
    if constexpr (EPI == EPI_SOR) v = a.omega * v + (T(1) - a.omega) * xo;
    if (!upd) v = xo;
    if constexpr (MODE == 1) __hip_atomic_store(a.xs + row, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_store(a.xs + row, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (upd) a.y[row] = v;
}

// second half, butterfly form: wait for the early operands, row sums across the lanes, publish
template <typename T, int EPI, int L, int K, int MODE>
__device__ __forceinline__ void lane_finish(const LaneArgs<T> &a, const LaneSet<T, K> &S, LaneDyn<T, K> &D, int g, int idle)
{
    const int lane = threadIdx.x & 63;
    const bool head = (lane & (L - 1)) == 0;
    long long t1 = 0;
    unsigned pend = 0;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if ((S.c[k] & LANE_EARLY) && !(S.c[k] & LANE_NONE) && Sentinel<T>::bits(D.xv[k]) == Sentinel<T>::value) pend |= 1u << k;
    unsigned spins = 0;
    if (S.gate >= 0 && __builtin_amdgcn_ballot_w64(pend != 0)) spins = lane_gate_wait<T>(a, S.gate);
    while (pend) {
        if (spins) __builtin_amdgcn_s_sleep(1);
        T t[K];
#pragma unroll
        for (int k = 0; k < K; ++k)
            t[k] = __hip_atomic_load(((pend >> k) & 1u) ? a.xs + (S.c[k] & LANE_MASK) : a.xs + idle, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int k = 0; k < K; ++k)
            if ((pend >> k) & 1u) {
                D.xv[k] = t[k];
                if (Sentinel<T>::bits(t[k]) != Sentinel<T>::value) pend &= ~(1u << k);
            }
        if ((++spins & 1023u) == 0) {
            // a producer that never comes (not resident / an earlier time-out): give up together, quickly
            if (spins > (1u << 21) || __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                __hip_atomic_store(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
    if (a.prof && lane == 0) t1 = wall_clock64();
    T s = T(0);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const T pr = S.v[k] * D.xv[k];
        s = s + ((S.c[k] & LANE_NONE) ? T(0) : pr);
    }
    s = seg_allreduce<L, T>(s);
    if (head && S.rid >= 0) lane_publish<T, EPI, MODE>(a, S.rid, s, D.bv, S.rd, D.xo);
    if (a.prof && lane == 0) profile_stamp(a.prof + (size_t)g * 4, D.t0, t1);
}

constexpr int LANE_WPB = BLK / 64;            // waves per workgroup (they never meet)

template <typename T, int EPI, int L, int K, int MODE>
__global__ __launch_bounds__(BLK) void gs_lane_kernel(const LaneArgs<T> a)
{
    const int wib = threadIdx.x >> 6;
    const int idle = (int)((((unsigned)blockIdx.x * LANE_WPB + (unsigned)wib) * 16u) % (unsigned)a.nidle);
    LaneSet<T, K> P, Q;
    LaneDyn<T, K> D;
    if constexpr (MODE != 1) {
        const int W = (int)gridDim.x * LANE_WPB;
        int g = (int)blockIdx.x * LANE_WPB + wib;
        const int gend = a.ngroups;
        if (g >= gend) return;
        // a group's static operands are requested when the wave arrives at it (round 5; until then the NEXT group's were requested before the wave
        // started to wait for the current one: the in-order memory counter puts every poll behind that prefetch -- level 1 of the 256^3 hierarchy
        // 2.282 -> 2.249 ms in one session, profiles/r05_microbench_lane_prefetch_ab.txt)
        for (; g < gend; g += W) {
            lane_load<T, L, K>(a, g, P);
            lane_issue<T, EPI, K>(a, P, D, idle);
            lane_finish<T, EPI, L, K, MODE>(a, P, D, g, idle);
        }
    } else {
        if (!claim_home_xcd(a.ticket + 1)) return;
        // two tickets are always ahead of the running group
        unsigned tk = 0;
        draw_ticket(a.ticket, tk);
        int g = ticket_number(tk);
        if (g >= a.ngroups) return;
        lane_load<T, L, K>(a, g, P);
        draw_ticket(a.ticket, tk);
        int g2 = ticket_number(tk);
        while (true) {
            unsigned tk3 = 0;
            lane_issue<T, EPI, K>(a, P, D, idle);
            if (g2 < a.ngroups) {
                lane_load<T, L, K>(a, g2, Q);
                draw_ticket(a.ticket, tk3);
            }
            lane_finish<T, EPI, L, K, MODE>(a, P, D, g, idle);
            if (g2 >= a.ngroups) break;
            g = ticket_number(tk3);
            unsigned tk4 = 0;
            lane_issue<T, EPI, K>(a, Q, D, idle);
            if (g < a.ngroups) {
                lane_load<T, L, K>(a, g, P);
                draw_ticket(a.ticket, tk4);
            }
            lane_finish<T, EPI, L, K, MODE>(a, Q, D, g2, idle);
            if (g >= a.ngroups) break;
            g2 = ticket_number(tk4);
        }
    }
}


// =================================================================== the MERGED form (round 6; layout and algebra: pamg_lanem_plan.h)
// s consecutive dependency levels of the sweep are eliminated into ONE super-level at plan time: the sweep pays one hand-off per
// super-level instead of one per level.  One row per wave (64 lanes share it), K = 1..8 operand slots per lane chosen PER ROW (the
// record of a group carries the first 64-slot unit and K), three kinds of operands: NEW values of earlier super-levels (polled in xs),
// OLD values (the snapshot of x taken by lanem_prepare_kernel) and entries of b.  f64, Gauss-Seidel only (SOR's merged coefficients
// would depend on the relaxation parameter of the call).
struct alignas(32) LaneMRec { int rid_a; int rid_b; int gate; int unitK; int rda_lo; int rda_hi; int rdb_lo; int rdb_hi; };     // unitK = first unit * 16 + units

struct LaneMSched {
    int64_t ngroups = 0, n_units = 0, nrows = 0;
    int rpw = 1;
    int nsuper = 0, nlevels = 0, s_max = 0, max_len = 0;
    int closed_by_length = 0, closed_by_growth = 0;
    double max_growth = 0.0;
    int64_t n_early = 0, n_old = 0, n_b = 0, max_super_groups = 0;
    int *d_cols = nullptr;
    double *d_vals = nullptr;
    LaneMRec *d_rec = nullptr;
    long long *d_prof = nullptr;
    // cluster layout (cluster > 0: d_cols = unique operands, d_vals = slot values, d_rec stays empty)
    int cluster = 0;
    int4 *d_crec = nullptr;           // [ngroups] {gate, first unique unit, first slot unit, KU | KS << 8 | rows << 16}
    unsigned short *d_sidx = nullptr; // [n_units * 64] slot codes
    int *d_crid = nullptr;            // [ngroups * cluster] row | NODIAG, -1 = none
    double *d_crd = nullptr;          // [ngroups * cluster] 1 / a_ii
    int64_t n_uunits = 0, n_uearly = 0, n_uold = 0, n_ub = 0, n_early_lines = 0;
    std::vector<int64_t> super_grp;   // [nsuper + 1] first row (group) of every super-level
    int last_grid = 0;
    int cap = 0;
    const void *cap_kernel = nullptr;
    size_t bytes = 0;
};

struct LaneMArgs {
    const int *cols;
    const double *vals;
    const LaneMRec *rec;
    const double *xold;    // snapshot of x from before the sweep
    double *y;             // the live x
    double *xs;            // hand-off buffer, sentinel-filled
    const double *b;
    unsigned *err;
    unsigned *ticket;
    int ngroups, nidle, use_gate;
    long long *prof;       // nullptr or [ngroups][4] time stamps (PAMG_TUNE_GS_PROF; the unpipelined kernel, static form)
    const unsigned short *sidx;   // cluster layout only: slot codes, rows of the groups, 1 / a_ii, rows per group at most (rec: one int4 per group)
    const int *crid;
    const double *crd;
    int crows;
    double *w;             // zero-iterate forward plan (the kernels' template argument Z): every updated row also stores its numerator b_r - s_r here
};

// x -> snapshot, sentinels -> hand-off buffer: the two passes every merged sweep starts with, in one launch
__global__ __launch_bounds__(BLK) void lanem_prepare_kernel(const double *__restrict__ x, double *__restrict__ xold, double *__restrict__ xs, int64_t n)
{
    unsigned long long *p = reinterpret_cast<unsigned long long *>(xs);
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLK) {
        xold[i] = x[i];
        p[i] = Sentinel<double>::value;
    }
}

// ---- the kernel.  One row at a time per wave: the record of the NEXT row travels while this one waits; the first two 64-slot units of a row are
// held in registers (46 VGPRs: eight waves per SIMD), rows of three and more units (a few per cent) fetch the rest in the tail.
// What round 6 measured on level 1 of the 256^3 hierarchy (2.03 M rows; profiles/r06_microbench_lanem_*, r06_lanem_row_phase_stamps_level1.txt,
// r06_pmc_lane_probe_level1_merged_vs_unmerged.json): the forward sweep goes 2.27 -> 1.80 - 1.85 ms at s = 2 AND at s = 3 and stays there -- it is no
// longer bound by the hand-off: 95 - 98 % of the rows find every early operand in their FIRST poll round (stamps), a row costs its wave 2.2 - 2.9 us
// (slots from HBM 0.6 - 0.7 us, operands 0.6 - 2.0 us growing with the number of waves, tail 0.16 us), and the sweep delivers 1.1 G rows/s from 768
// workgroups on, more waves only slow each other down.  The counters: 45 - 52 L1 -> L2 requests per row (35 unmerged), 24 % of them from memory, average
// latency 390 - 430 cycles.  Built, parity-tested, measured and REMOVED again (git history of this file; numbers in profiles/): every unit of a row in
// registers (92 VGPRs, five waves per SIMD: same floor); a pipelined kernel with three row contexts in flight (slower: 2.0 - 2.3 ms -- every re-poll
// waits for the prefetches, the first poll round is stale); the same with a PUBLISHER wave per workgroup taking the stores out of the compute waves'
// in-order memory queue through an LDS mailbox (2.2 - 2.5 ms); ordinary loads for the static operands (+ 3 - 5 %); the next row's slots requested behind
// the current row's operands (1.86 - 1.99 ms).  An ablation of the first kernel (wrong results by construction): 1.21 ms without waiting for early
// operands, 0.94 without the publishing store as well, 0.73 for slots + early operands alone.  What that ablation priced -- the loads past the L1 and the
// publishing stores per row -- is what the CLUSTER layout (round 8, c_group below; RPW = 0 in the kernels' template arguments) shares between
// neighbouring rows.
// RPW rows of one super-level per wave (64 / RPW lanes each), NREG units of 64 slots in registers (the rest of a long group is fetched in the tail)
template <int NREG>
struct MCtx {
    int c[NREG];
    double v[NREG], xv[NREG];
    double bv, xo, rd;         // per lane: its row's b, old value, 1 / a_ii
    double num;                // per lane: b - sum of its row (m_finish; what a zero-iterate forward plan stores in w)
    int rid;                   // per lane: its row | NODIAG, -1 = dummy slot
    int gate, unit, K, g;      // uniform
};

__device__ __forceinline__ void m_rec(const int4 *rp, int g, int gend, int4 &q0, int4 &q1)
{
    const size_t gg = (size_t)(g < gend ? g : gend - 1);
    q0 = rp[2 * gg];
    q1 = rp[2 * gg + 1];
}

template <int RPW, int NREG>
__device__ __forceinline__ void m_slots(const LaneMArgs &a, MCtx<NREG> &C, const int4 &q0, const int4 &q1, int g, int lane)
{
    // record: {row a | NODIAG, row b (RPW = 2; else -1), gate, unit * 16 + K, 1 / a_ii of a (2 words), of b (2 words)}
    C.g = g;
    const int rid_a = __builtin_amdgcn_readfirstlane(q0.x), rid_b = __builtin_amdgcn_readfirstlane(q0.y);
    C.gate = a.use_gate ? __builtin_amdgcn_readfirstlane(q0.z) : -1;
    const int uk = __builtin_amdgcn_readfirstlane(q0.w);
    C.unit = uk >> 4;
    C.K = uk & 15;
    const double rd_a = __hiloint2double(__builtin_amdgcn_readfirstlane(q1.y), __builtin_amdgcn_readfirstlane(q1.x));
    const double rd_b = __hiloint2double(__builtin_amdgcn_readfirstlane(q1.w), __builtin_amdgcn_readfirstlane(q1.z));
    const bool second = RPW == 2 && lane >= 32;
    C.rid = second ? rid_b : rid_a;
    C.rd = second ? rd_b : rd_a;
    const size_t e0 = (size_t)C.unit * 64 + (size_t)lane;
#pragma unroll
    for (int k = 0; k < NREG; ++k) {
        // a group of fewer units reads its last unit again (no load under a branch); the copies are masked in m_gather
        const size_t e = e0 + (size_t)64 * (size_t)(k < C.K ? k : C.K - 1);
        C.c[k] = a.cols[e];
        C.v[k] = a.vals[e];
    }
}

// xz: the old iterate is known to be all zeros -- every OLD operand (neither an early one nor an entry of b) becomes an idle slot, its product + 0
// as the padding's is: the same bits for finite data without the gathers.  coh: a.xold was written by other workgroups of THIS launch (the second
// phase of the fused symmetric sweep), so the row's own old value is read past the L1 as the operands are
// BCOH: a.b was written by other workgroups of THIS launch too (the backward phase on a zero-iterate plan, whose right-hand side is the vector of
// numerators the forward phase stored): the row's own entry is read past the L1; the operands that come from b already are
// XOZ: the sweep runs on a virtual zero iterate (the correction form, Z = 2 of the kernels): a row without a diagonal carries 0, not what a.xold holds
template <int NREG, bool BCOH = false, bool XOZ = false>
__device__ __forceinline__ void m_gather(const LaneMArgs &a, MCtx<NREG> &C, int idle, const bool xz = false, const bool coh = false)
{
#pragma unroll
    for (int k = 1; k < NREG; ++k)
        if (k >= C.K) C.c[k] = LANE_NONE;
    if (xz) {
#pragma unroll
        for (int k = 0; k < NREG; ++k)
            if (!(C.c[k] & (LANE_EARLY | LANEM_BSRC))) C.c[k] |= LANE_NONE;
    }
    const int row = C.rid < 0 ? 0 : (C.rid & LANE_MASK);
    if constexpr (BCOH) C.bv = __hip_atomic_load(a.b + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else C.bv = a.b[row];
    if constexpr (XOZ) C.xo = 0.0;
    else C.xo = coh ? __hip_atomic_load(a.xold + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : a.xold[row];      // used by rows without a diagonal only
    // every operand by an L1-bypassing load: early ones poll the hand-off buffer, static ones read the snapshot of x and b (ordinary loads for
    // the static operands were measured 3 - 5 % slower, profiles/r06_microbench_lanem_plain_loads_for_static_operands_not_kept.json)
#pragma unroll
    for (int k = 0; k < NREG; ++k) {
        const int col = C.c[k] & LANEM_MASK;
        const double *p = (C.c[k] & LANE_NONE) ? a.xold + idle : ((C.c[k] & LANE_EARLY) ? a.xs + col : ((C.c[k] & LANEM_BSRC) ? a.b + col : a.xold + col));
        C.xv[k] = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// wait for the group's operands and form x_i of its rows; returns the value a row's head lane publishes
template <int RPW, int NREG>
__device__ __forceinline__ double m_finish(const LaneMArgs &a, MCtx<NREG> &C, int idle, long long *t_ready = nullptr, unsigned *n_spins = nullptr, const bool xz = false)
{
    using T = double;
    const int lane = threadIdx.x & 63;
    unsigned pend = 0;
#pragma unroll
    for (int k = 0; k < NREG; ++k)
        if ((C.c[k] & LANE_EARLY) && !(C.c[k] & LANE_NONE) && Sentinel<T>::bits(C.xv[k]) == Sentinel<T>::value) pend |= 1u << k;
    unsigned spins = 0;
    if (C.gate >= 0 && __builtin_amdgcn_ballot_w64(pend != 0)) {
        const T *gp = a.xs + C.gate;
        while (true) {
            const T gv = __hip_atomic_load(gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (Sentinel<T>::bits(gv) != Sentinel<T>::value) break;
            __builtin_amdgcn_s_sleep(2);
            if ((++spins & 1023u) == 0 && (spins > (1u << 21) || __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) break;
        }
    }
    while (pend) {
        if (spins) __builtin_amdgcn_s_sleep(1);
        T t[NREG];
#pragma unroll
        for (int k = 0; k < NREG; ++k)
            t[k] = __hip_atomic_load(((pend >> k) & 1u) ? a.xs + (C.c[k] & LANEM_MASK) : a.xs + idle, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int k = 0; k < NREG; ++k)
            if ((pend >> k) & 1u) {
                C.xv[k] = t[k];
                if (Sentinel<T>::bits(t[k]) != Sentinel<T>::value) pend &= ~(1u << k);
            }
        if ((++spins & 1023u) == 0) {
            if (spins > (1u << 21) || __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                __hip_atomic_store(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
    if (t_ready) { *t_ready = wall_clock64(); *n_spins = spins; }
    T s = T(0);
#pragma unroll
    for (int k = 0; k < NREG; ++k) {
        const T pr = C.v[k] * C.xv[k];
        s = s + ((C.c[k] & LANE_NONE) ? T(0) : pr);
    }
    if (C.K > NREG) {
        // the units beyond the registers: fetched now, one after the other (groups this long are a few per cent)
        for (int k = NREG; k < C.K; ++k) {
            const size_t e = (size_t)(C.unit + k) * 64 + (size_t)lane;
            int c = a.cols[e];
            if (xz && !(c & (LANE_EARLY | LANEM_BSRC))) c |= LANE_NONE;
            const T v = a.vals[e];
            const int col = c & LANEM_MASK;
            const bool early = (c & LANE_EARLY) && !(c & LANE_NONE);
            const T *p = (c & LANE_NONE) ? a.xold + idle : ((c & LANE_EARLY) ? a.xs + col : ((c & LANEM_BSRC) ? a.b + col : a.xold + col));
            T x = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            unsigned sp2 = 0;
            while (__builtin_amdgcn_ballot_w64(early && Sentinel<T>::bits(x) == Sentinel<T>::value)) {
                __builtin_amdgcn_s_sleep(1);
                const T t = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (early && Sentinel<T>::bits(x) == Sentinel<T>::value) x = t;
                if ((++sp2 & 1023u) == 0 && (sp2 > (1u << 21) || __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                    __hip_atomic_store(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
            }
            const T pr = v * x;
            s = s + ((c & LANE_NONE) ? T(0) : pr);
        }
    }
    s = seg_allreduce<64 / RPW, T>(s);
    const bool upd = C.rid >= 0 && !(C.rid & LANE_NODIAG);
    C.num = C.bv - s;
    T val = C.num * C.rd;
    if (!upd) val = C.xo;
    return val;
}

// PH = 1: the first phase of the fused symmetric sweep -- the hand-off buffer is also where the second phase reads its OLD operands (every row
// publishes, a row without a diagonal its old value), x is not written
// WST: a zero-iterate forward plan -- the row's numerator goes to a.w
// ACC: the correction form -- the row's value is ADDED to a.y (y is read by nobody else in a zero-iterate launch, and the row has one owning lane:
// a plain load, add, store)
template <int RPW, int MODE, int NREG, int PH = 0, bool WST = false, bool ACC = false>
__device__ __forceinline__ void m_publish(const LaneMArgs &a, const MCtx<NREG> &C, double val)
{
    if (((threadIdx.x & 63) & (64 / RPW - 1)) == 0 && C.rid >= 0) {
        const int row = C.rid & LANE_MASK;
        if constexpr (MODE == 1) __hip_atomic_store(a.xs + row, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else __hip_atomic_store(a.xs + row, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (PH != 1) {
            if (!(C.rid & LANE_NODIAG)) {
                if constexpr (ACC) a.y[row] = a.y[row] + val;
                else a.y[row] = val;
            }
        }
        if constexpr (WST) {                                  // the numerator crosses XCDs inside the fused launch: the flavour of the publishing store
            if (!(C.rid & LANE_NODIAG)) __hip_atomic_store(a.w + row, C.num, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- the CLUSTER layout (pamg_lanem_plan.h): one wave takes up to R rows of one super-level that are consecutive in row-index order, loads the
// UNION of their operands ONCE -- one lane per unique operand, the same L1-bypassing loads, sentinel polling, gate wait, bounded spin and error
// word as m_gather / m_finish -- puts the values in its own 4 KB of LDS (wave-synchronous: the waves of a workgroup never meet), forms the products
// of its slots from there, sums them per row (a lane serves one row, a row owns consecutive lanes: segmented inclusive scan, the row's LAST lane
// holds the sum) and publishes every row of the group in one store instruction.  Static chip-wide assignment only.
constexpr int LANEC_K = 8;                    // units of unique operands / of slots per group at most (LANEC_UMAX = 64 * this)

__device__ __forceinline__ int4 c_rec(const int4 *rp, int g, int gend) { return rp[(size_t)(g < gend ? g : gend - 1)]; }

// one group.  PH / WST / ACC as in m_publish; xz / coh / BCOH as in m_gather (ACC in phase 1: XOZ)
template <int PH, bool WST = false, bool BCOH = false, bool ACC = false>
__device__ __forceinline__ void c_group(const LaneMArgs &a, double *lds, const int4 &q, int g, int lane, int idle, const bool xz, const bool coh)
{
    using T = double;
    const int gate = a.use_gate ? __builtin_amdgcn_readfirstlane(q.x) : -1;
    const int uunit = __builtin_amdgcn_readfirstlane(q.y), sunit = __builtin_amdgcn_readfirstlane(q.z), kk = __builtin_amdgcn_readfirstlane(q.w);
    const int KU = kk & 15, KS = (kk >> 8) & 15;
    int c[LANEC_K];
    unsigned si[LANEC_K];
    T sv[LANEC_K], xv[LANEC_K];
    const size_t u0 = (size_t)uunit * 64 + (size_t)lane, s0 = (size_t)sunit * 64 + (size_t)lane;
#pragma unroll
    for (int k = 0; k < LANEC_K; ++k) {
        c[k] = LANE_NONE;
        if (k < KU) c[k] = a.cols[u0 + (size_t)64 * k];
    }
#pragma unroll
    for (int k = 0; k < LANEC_K; ++k) {
        si[k] = LANEC_PAD | LANEC_UNUSED; sv[k] = T(0);
        if (k < KS) { si[k] = a.sidx[s0 + (size_t)64 * k]; sv[k] = a.vals[s0 + (size_t)64 * k]; }
    }
    if (xz) {
#pragma unroll
        for (int k = 0; k < LANEC_K; ++k)
            if (!(c[k] & (LANE_EARLY | LANEM_BSRC))) c[k] |= LANE_NONE;
    }
    // the unique operands: early ones poll the hand-off buffer, static ones read the snapshot of x and b
#pragma unroll
    for (int k = 0; k < LANEC_K; ++k) {
        xv[k] = T(0);
        if (k < KU) {
            const int col = c[k] & LANEM_MASK;
            const T *p = (c[k] & LANE_NONE) ? a.xold + idle : ((c[k] & LANE_EARLY) ? a.xs + col : ((c[k] & LANEM_BSRC) ? a.b + col : a.xold + col));
            xv[k] = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // the lane's row (every slot of a lane carries it)
    const bool unused = (si[0] & LANEC_UNUSED) != 0;
    const int tag = (int)((si[0] >> LANEC_ROWSHIFT) & 7u);
    const size_t ri = (size_t)g * (size_t)a.crows + (size_t)(tag < a.crows ? tag : 0);
    const int rid = unused ? -1 : a.crid[ri];
    const T rd = a.crd[ri];
    const int row = rid < 0 ? 0 : (rid & LANE_MASK);
    T bv;
    if constexpr (BCOH) bv = __hip_atomic_load(a.b + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else bv = a.b[row];
    T xo = T(0);                                                // used by rows without a diagonal only
    if constexpr (!(ACC && PH == 1)) xo = coh ? __hip_atomic_load(a.xold + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : a.xold[row];
    // the rows' first lanes (static plan data): exchanged here, in front of the waits, so that no lane exchange but the sums' stands between the
    // last operand and the publishing store.  The empty asm keeps the compiler from sinking the exchange behind the poll loop; the mask lives
    // through the loop in scalar registers (the kernels are at their 128 vector registers)
    unsigned long long heads = seg_scan_heads(si[0] & ((7u << LANEC_ROWSHIFT) | LANEC_UNUSED), lane);
    asm volatile("" : "+s"(heads));
    unsigned pend = 0;
#pragma unroll
    for (int k = 0; k < LANEC_K; ++k)
        if ((c[k] & LANE_EARLY) && !(c[k] & LANE_NONE) && Sentinel<T>::bits(xv[k]) == Sentinel<T>::value) pend |= 1u << k;
    unsigned spins = 0;
    if (gate >= 0 && __builtin_amdgcn_ballot_w64(pend != 0)) {
        const T *gp = a.xs + gate;
        while (true) {
            const T gv = __hip_atomic_load(gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (Sentinel<T>::bits(gv) != Sentinel<T>::value) break;
            __builtin_amdgcn_s_sleep(2);
            if ((++spins & 1023u) == 0 && (spins > (1u << 21) || __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) break;
        }
    }
    while (pend) {
        if (spins) __builtin_amdgcn_s_sleep(1);
        T t[LANEC_K];
#pragma unroll
        for (int k = 0; k < LANEC_K; ++k) {
            t[k] = T(0);
            if (k < KU) t[k] = __hip_atomic_load(((pend >> k) & 1u) ? a.xs + (c[k] & LANEM_MASK) : a.xs + idle, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int k = 0; k < LANEC_K; ++k)
            if ((pend >> k) & 1u) {
                xv[k] = t[k];
                if (Sentinel<T>::bits(t[k]) != Sentinel<T>::value) pend &= ~(1u << k);
            }
        if ((++spins & 1023u) == 0) {
            if (spins > (1u << 21) || __hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                __hip_atomic_store(a.err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
    asm volatile("" : "+s"(heads));                              // (the lanes' part of the bookkeeping: in the shadow of the LDS round trip)
    const int seglo = seg_scan_first(heads, lane);
    // values -> LDS (an idle operand is a zero: padding, and every OLD operand where x is known to be zero), slots <- LDS
#pragma unroll
    for (int k = 0; k < LANEC_K; ++k)
        if (k < KU) lds[k * 64 + lane] = (c[k] & LANE_NONE) ? T(0) : xv[k];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    T s = T(0);
#pragma unroll
    for (int k = 0; k < LANEC_K; ++k) {
        const T pr = sv[k] * lds[si[k] & LANEC_IDX];
        s = s + ((si[k] & LANEC_PAD) ? T(0) : pr);
    }
    // segmented inclusive scan over the lanes of a row, in registers (pamg_wave.h)
    s = seg_scan_incl(s, seglo, lane);
    const bool tail = ((((heads >> 1) | (1ull << 63)) >> lane) & 1ull) != 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // the next group's values overwrite what was read here
    __builtin_amdgcn_wave_barrier();
    const bool upd = rid >= 0 && !(rid & LANE_NODIAG);
    const T num = bv - s;
    T val = num * rd;
    if (!upd) val = xo;
    if (tail && rid >= 0) {
        __hip_atomic_store(a.xs + row, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if constexpr (PH != 1) {
            if (upd) {
                if constexpr (ACC) a.y[row] = a.y[row] + val;
                else a.y[row] = val;
            }
        }
        if constexpr (WST) {
            if (upd) __hip_atomic_store(a.w + row, num, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// NREG = units of a group held in registers: 2 (one row per wave) / 4 (two rows per wave) on the large levels, where eight waves per SIMD matter;
// 8 on the small levels, whose sweeps are bound by their hand-offs -- there the sequential tail of a long row sits on the critical path (level 2 of the
// 256^3 hierarchy at s = 6: 56 % of the rows hold three and more units)
// Z = 1: the forward plan of a zero-iterate pair run as a launch of its own (the numerators go to a.w; the backward plan then runs as Z = 0 with
// b = that vector: the kernel boundary orders the two)
// Z = 2: the backward plan of a zero-iterate pair in the correction form: its values are added to a.y
template <int MODE, int RPW, int NREG, int Z = 0>
__global__ __launch_bounds__(BLK) void gs_lanem_kernel(const LaneMArgs a)
{
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;
    const int idle = (int)((((unsigned)blockIdx.x * LANE_WPB + (unsigned)wib) * 16u) % (unsigned)a.nidle);
    const int4 *rp = reinterpret_cast<const int4 *>(a.rec);
    const int gend = a.ngroups;
    __shared__ double c_lds[RPW == 0 ? LANE_WPB * LANEC_UMAX : 1];
    if constexpr (RPW == 0) {                                    // the cluster layout (static assignment)
        static_assert(RPW != 0 || MODE != 1, "the cluster layout has no ticket form");
        const int W = (int)gridDim.x * LANE_WPB;
        int g = __builtin_amdgcn_readfirstlane((int)blockIdx.x * LANE_WPB + wib);
        if (g >= gend) return;
        int4 q = c_rec(rp, g, gend);
        for (; g < gend; g += W) {
            const int4 nq = c_rec(rp, g + W, gend);
            c_group<0, Z == 1, false, Z == 2>(a, c_lds + wib * LANEC_UMAX, q, g, lane, idle, false, false);
            q = nq;
        }
    } else {
    MCtx<NREG> X;
    if constexpr (MODE != 1) {
        const int W = (int)gridDim.x * LANE_WPB;
        int g = __builtin_amdgcn_readfirstlane((int)blockIdx.x * LANE_WPB + wib);
        if (g >= gend) return;
        int4 q0, q1;
        m_rec(rp, g, gend, q0, q1);
        for (; g < gend; g += W) {
            int4 n0, n1;
            m_rec(rp, g + W, gend, n0, n1);
            if (a.prof) {
                // diagnostics: where a group's time goes (forced waits between the phases: the stamps change the timing a little)
                const long long t0 = wall_clock64();
                m_slots<RPW, NREG>(a, X, q0, q1, g, lane);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const long long t1 = wall_clock64();
                m_gather<NREG>(a, X, idle);
                long long t2 = 0;
                unsigned sp = 0;
                const double val = m_finish<RPW, NREG>(a, X, idle, &t2, &sp);
                m_publish<RPW, MODE, NREG, 0, Z == 1, Z == 2>(a, X, val);
                if (lane == 0) {
                    long long *o = a.prof + (size_t)g * 4;
                    o[0] = t0 | ((long long)(sp > 4095u ? 4095u : sp) << 52);
                    o[1] = t1; o[2] = t2; o[3] = wall_clock64();
                }
            } else {
                m_slots<RPW, NREG>(a, X, q0, q1, g, lane);
                m_gather<NREG>(a, X, idle);
                const double val = m_finish<RPW, NREG>(a, X, idle);
                m_publish<RPW, MODE, NREG, 0, Z == 1, Z == 2>(a, X, val);
            }
            q0 = n0; q1 = n1;
        }
    } else {
        if (!claim_home_xcd(a.ticket + 1)) return;
        unsigned tk = 0;
        draw_ticket(a.ticket, tk);
        int g = ticket_number(tk);
        if (g >= gend) return;
        draw_ticket(a.ticket, tk);
        int g2 = ticket_number(tk);
        int4 q0, q1;
        m_rec(rp, g, gend, q0, q1);
        while (true) {
            int4 n0, n1;
            m_rec(rp, g2, gend, n0, n1);
            unsigned tk3 = 0;
            draw_ticket(a.ticket, tk3, g2 < gend);
            m_slots<RPW, NREG>(a, X, q0, q1, g, lane);
            m_gather<NREG>(a, X, idle);
            const double val = m_finish<RPW, NREG>(a, X, idle);
            m_publish<RPW, MODE, NREG, 0, Z == 1, Z == 2>(a, X, val);
            if (g2 >= gend) break;
            g = g2; q0 = n0; q1 = n1;
            g2 = ticket_number(tk3);
        }
    }
    }
}

// =================================================================== the FUSED SYMMETRIC sweep of the merged form: forward + backward in ONE launch
// Phase 1 walks the forward schedule's groups exactly as gs_lanem_kernel does, a completion barrier follows, phase 2 walks the backward schedule's.
// What the two directional launches paid around the sweeps is gone: no sentinel fill and no snapshot of x (lanem_prepare_kernel), one kernel
// drain / ramp-up instead of two, and phase 1 stores every value ONCE.
//   vectors : phase 1 reads its OLD operands from x, which it never writes, and publishes every row's value in its hand-off buffer H_f (a row
//             without a diagonal its old value): H_f then IS the iterate after the forward sweep.  Phase 2 reads its OLD operands from H_f, polls
//             H_b and writes x.  No vector is read and written in the same phase, so no snapshot is needed.
//   buffers : the operator owns H_f[0], H_f[1] and H_b; a parity word says which H_f this launch publishes in and is flipped by the last workgroup
//             to leave.  Between launches H_f[parity] is all sentinels, the other two hold anything.  Wipes ride on the sweep: phase 1 wipes H_b
//             (the previous sweep's backward values, read by nobody in phase 1), phase 2 wipes H_f[parity ^ 1] (the previous launch's forward
//             values, dead since that launch ended) -- the buffer the NEXT launch publishes in.  The wipe is partitioned by GROUP, not by wave, so
//             that it holds for the static and the ticket assignment alike: with n = q G + r entries and G groups, group g owns
//             [g q + min(g, r), + q + (g < r)); the first group of every block of B consecutive groups (B = wipe_blk, chosen so that a block owns
//             >= 64 entries) wipes its block's entries in one coalesced wave store (tests/test_symsweep_plan.py replays the partition).  Wipes are
//             stores of the flavour of the publishing store and complete with the wave's vmcnt(0) wait in front of the barrier / at its exit.
//   barrier : counts FINISHED GROUPS (in the ticket form nobody knows how many workgroups stayed).  Every wave waits for its stores
//             (s_waitcnt vmcnt(0)) and adds its groups to a word in LDS; behind a workgroup barrier ONE lane adds the workgroup's total to the counter
//             (agent-scope atomic) and polls it past the L1 with the bounded spin of the hand-offs (same error word, same time-out); the other
//             waves wait for that lane at a second workgroup barrier.  No phase-2 group starts before the counter is full; phase 1 is the forward
//             sweep, which completes on its own, and phase 2 is the backward sweep: deadlock-free where the two sweeps are.
//   counters: the last workgroup to leave (a second counter, one add per workgroup after its waves have met) zeroes barrier, tickets and the home
//             XCD word and flips the parity: no helper launch, no memset node.
struct LaneMSymArgs {
    LaneMArgs ph[2];       // [0] forward: xold = x, xs = H_f[parity] (set by the kernel); [1] backward: xold = H_f[parity] (likewise), y = x, xs = H_b
    double *hf[2];
    unsigned *sync;        // [0] finished groups of phase 1, [1] workgroups that left, [2] / [3] tickets of phase 1 / 2, [4] home XCD + 1, [5] parity
    int wq[2], wr[2], wblk[2];   // wipe parts of phase p (over the buffer it wipes): n = wq * ngroups + wr, groups per wipe block
    int xzero;             // x is all zeros on entry: phase 1 skips its OLD operands
};

// group g's duty in the wipe of `w`: nothing unless it is the first group of its block
template <int MODE>
__device__ __forceinline__ void m_wipe(double *w, int g, int G, int q, int r, int blk, int lane)
{
    if (g & (blk - 1)) return;                                  // blk: a power of two
    const int g1 = g + blk < G ? g + blk : G;
    const int lo = g * q + (g < r ? g : r), hi = g1 * q + (g1 < r ? g1 : r);
    unsigned long long *p = reinterpret_cast<unsigned long long *>(w);
    for (int i = lo + lane; i < hi; i += 64) {
        if constexpr (MODE == 1) __hip_atomic_store(p + i, Sentinel<double>::value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else __hip_atomic_store(p + i, Sentinel<double>::value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one phase of the fused sweep by one wave; returns the groups it finished
template <int MODE, int RPW, int NREG, int PH, int Z = 0>
__device__ __forceinline__ unsigned m_phase(const LaneMArgs &a, double *wipe, int wq, int wr, int wblk, unsigned *ticket, const bool xz, int lane, int wib, int idle, double *c_lds)
{
    const int4 *rp = reinterpret_cast<const int4 *>(a.rec);
    const int gend = a.ngroups;
    unsigned done = 0;
    if constexpr (RPW == 0) {                                    // the cluster layout (static assignment)
        static_assert(RPW != 0 || MODE != 1, "the cluster layout has no ticket form");
        const int W = (int)gridDim.x * LANE_WPB;
        int g = __builtin_amdgcn_readfirstlane((int)blockIdx.x * LANE_WPB + wib);
        if (g >= gend) return 0;
        int4 q = c_rec(rp, g, gend);
        for (; g < gend; g += W) {
            const int4 nq = c_rec(rp, g + W, gend);
            c_group<PH, Z && PH == 1, Z && PH == 2, Z == 2>(a, c_lds + wib * LANEC_UMAX, q, g, lane, idle, xz, PH == 2);
            m_wipe<MODE>(wipe, g, gend, wq, wr, wblk, lane);
            ++done;
            q = nq;
        }
    } else {
    MCtx<NREG> X;
    if constexpr (MODE != 1) {
        const int W = (int)gridDim.x * LANE_WPB;
        int g = __builtin_amdgcn_readfirstlane((int)blockIdx.x * LANE_WPB + wib);
        if (g >= gend) return 0;
        int4 q0, q1;
        m_rec(rp, g, gend, q0, q1);
        for (; g < gend; g += W) {
            int4 n0, n1;
            m_rec(rp, g + W, gend, n0, n1);
            m_slots<RPW, NREG>(a, X, q0, q1, g, lane);
            m_gather<NREG, Z && PH == 2, Z == 2 && PH == 1>(a, X, idle, xz, PH == 2);
            const double val = m_finish<RPW, NREG>(a, X, idle, nullptr, nullptr, xz);
            m_publish<RPW, MODE, NREG, PH, Z && PH == 1, Z == 2 && PH == 2>(a, X, val);
            m_wipe<MODE>(wipe, g, gend, wq, wr, wblk, lane);      // behind the publishing stores: nobody waits for these
            ++done;
            q0 = n0; q1 = n1;
        }
    } else {
        unsigned tk = 0;
        draw_ticket(ticket, tk);
        int g = ticket_number(tk);
        if (g >= gend) return 0;
        draw_ticket(ticket, tk);
        int g2 = ticket_number(tk);
        int4 q0, q1;
        m_rec(rp, g, gend, q0, q1);
        while (true) {
            int4 n0, n1;
            m_rec(rp, g2, gend, n0, n1);
            unsigned tk3 = 0;
            draw_ticket(ticket, tk3, g2 < gend);
            m_slots<RPW, NREG>(a, X, q0, q1, g, lane);
            m_gather<NREG, Z && PH == 2, Z == 2 && PH == 1>(a, X, idle, xz, PH == 2);
            const double val = m_finish<RPW, NREG>(a, X, idle, nullptr, nullptr, xz);
            m_publish<RPW, MODE, NREG, PH, Z && PH == 1, Z == 2 && PH == 2>(a, X, val);
            m_wipe<MODE>(wipe, g, gend, wq, wr, wblk, lane);
            ++done;
            if (g2 >= gend) break;
            g = g2; q0 = n0; q1 = n1;
            g2 = ticket_number(tk3);
        }
    }
    }
    return done;
}

// the completion barrier between the phases (see above); `done` = groups this wave finished, `total` = groups of the phase.  Every wave of the
// workgroup calls it.
__device__ __forceinline__ void sym_phase_barrier(unsigned *counter, unsigned *err, unsigned *sh_done, unsigned done, unsigned total)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // this wave's phase-1 stores (values and wipes) have left
    if ((threadIdx.x & 63) == 0 && done) atomicAdd(sh_done, done);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned mine = *sh_done;
        if (mine) __hip_atomic_fetch_add(counter, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned spins = 0;
        while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < total) {
            __builtin_amdgcn_s_sleep(2);
            if ((++spins & 1023u) == 0 && (spins > (1u << 21) || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
    __syncthreads();
}

// the last workgroup to leave puts the counters back to zero and flips the parity (every workgroup of the grid passes here once, after its waves
// have met: nobody polls, draws a ticket or reads the parity any more when the last add arrives)
__device__ __forceinline__ void sym_leave(unsigned *sync, unsigned parity)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned left = __hip_atomic_fetch_add(sync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (left == gridDim.x - 1) {
            for (int k = 0; k < 5; ++k) __hip_atomic_store(sync + k, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(sync + 5, parity ^ 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Z = 1: the two phases run the operator's zero-iterate plans (x = 0 on entry): phase 1 stores the numerators in ph[0].w, phase 2 reads them as its b
// Z = 2: the correction form -- the same two phases on a VIRTUAL zero iterate (b is a residual, x is never read as an operand: rows without a
//        diagonal carry 0 through both phases), phase 2 adds its values to x instead of storing them: x += sweep(0, b)
template <int MODE, int RPW, int NREG, int Z = 0>
__global__ __launch_bounds__(BLK) void gs_lanem_sym_kernel(const LaneMSymArgs a)
{
    __shared__ unsigned sh_done;
    __shared__ int sh_home;
    __shared__ double c_lds[RPW == 0 ? LANE_WPB * LANEC_UMAX : 1];
    const int lane = threadIdx.x & 63;
    const int wib = threadIdx.x >> 6;
    const int idle = (int)((((unsigned)blockIdx.x * LANE_WPB + (unsigned)wib) * 16u) % (unsigned)a.ph[0].nidle);
    const unsigned parity = __builtin_amdgcn_readfirstlane(__hip_atomic_load(a.sync + 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & 1u;
    if (threadIdx.x == 0) {
        sh_done = 0u;
        sh_home = 1;
        if constexpr (MODE == 1) sh_home = home_xcd_vote(a.sync + 4) ? 1 : 0;     // (the vote alone: this barrier is shared with sh_done)
    }
    __syncthreads();
    if (sh_home) {                                               // (uniform per workgroup: the barriers below are met by all of its waves or by none)
        double *hf = a.hf[parity], *hf_next = a.hf[parity ^ 1u];
        LaneMArgs p1 = a.ph[0], p2 = a.ph[1];
        p1.xs = hf; p1.y = nullptr;
        p2.xold = hf;
        const unsigned done = m_phase<MODE, RPW, NREG, 1, Z>(p1, p2.xs, a.wq[0], a.wr[0], a.wblk[0], a.sync + 2, a.xzero != 0, lane, wib, idle, c_lds);
        sym_phase_barrier(a.sync, p1.err, &sh_done, done, (unsigned)p1.ngroups);
        (void)m_phase<MODE, RPW, NREG, 2, Z>(p2, hf_next, a.wq[1], a.wr[1], a.wblk[1], a.sync + 3, false, lane, wib, idle, c_lds);
    }
    sym_leave(a.sync, parity);
}

// ------------------------------------------------------------------ host side
namespace {

template <typename T, int EPI, int L, int MODE>
const void *lane_kernel_k(int K)
{
    switch (K) {
        case 1: return (const void *)gs_lane_kernel<T, EPI, L, 1, MODE>;
        case 2: return (const void *)gs_lane_kernel<T, EPI, L, 2, MODE>;
        case 3: return (const void *)gs_lane_kernel<T, EPI, L, 3, MODE>;
        case 4: return (const void *)gs_lane_kernel<T, EPI, L, 4, MODE>;
    }
    return nullptr;
}

template <typename T, int EPI, int MODE>
const void *lane_kernel_l(int L, int K)
{
    switch (L) {
        case 4: return lane_kernel_k<T, EPI, 4, MODE>(K);
        case 8: return lane_kernel_k<T, EPI, 8, MODE>(K);
        case 16: return lane_kernel_k<T, EPI, 16, MODE>(K);
        case 32: return lane_kernel_k<T, EPI, 32, MODE>(K);
        case 64: return lane_kernel_k<T, EPI, 64, MODE>(K);
    }
    return nullptr;
}

// mode: 0 static across the chip, 1 one-XCD (tickets)
template <typename T>
const void *lane_kernel(int epi, int L, int K, int mode)
{
    // bsr_gauss_seidel with 1x1 blocks computes (b - sum) / a_ii as well: in this form the two are one kernel
    if (epi == EPI_SOR) return mode == 1 ? lane_kernel_l<T, EPI_SOR, 1>(L, K) : lane_kernel_l<T, EPI_SOR, 0>(L, K);
    return mode == 1 ? lane_kernel_l<T, EPI_GS, 1>(L, K) : lane_kernel_l<T, EPI_GS, 0>(L, K);
}

}  // namespace

void free_lane_part(LaneSched *t)
{
    if (!t) return;
    hipFree(t->d_cols); hipFree(t->d_rec); hipFree(t->d_vals); hipFree(t->d_prof);
    delete t;
}

// rows the lane form can hold (LANE_KMAX * 64 off-diagonal entries) -- the padding check is the planner's
bool lane_eligible(const pamg_matrix_s *A, const GsSchedule *g)
{
    return A->R == 1 && g->nlevels > 1 && g->d_xs != nullptr && A->max_row_len <= LANE_KMAX * 64 + 1 && !g->lane_unfit;
}

// one-XCD form: the vectors (x, hand-off buffer) and the polling stay inside one XCD's 4 MB L2
static bool lane_one_xcd(const pamg_matrix_s *A, const GsSchedule *g)
{
    return A->gran_xcd == 1 || (A->gran_xcd == 0 && A->nrows <= 131072 && g->nrows / std::max(1, g->nlevels) <= 1024);
}

// The layout filled on the device (the default): the host plan (pattern only, build_lane_plan with fill = false) gives the row of every
// (group, slot row) and the gates; this kernel writes cols / vals and the 16-byte slot-row records (row | NODIAG, gate, 1 / a_ii) from the
// resident CSR arrays -- no download of the values, no upload of the padded 12-byte slots (256^3 level 1: 1.5 GB, 1 s of host time per direction).
// One wave per group; the L lanes of a row all walk the row (broadcast loads), lane q keeps entries e = q, q + L, ...: the slot rule
// of the host's fill pass (entries in storage order without the diagonal, the last stored diagonal wins).
template <typename T>
__global__ __launch_bounds__(256) void lane_fill_kernel(int n, const int *__restrict__ Ap, const int *__restrict__ Aj, const T *__restrict__ Ax,
                                                        int row_start, int row_step, long long m, int L, int K, long long ngroups, const int *__restrict__ rid,
                                                        const int *__restrict__ gate, int *__restrict__ cols, T *__restrict__ vals, LaneRec *__restrict__ rec)
{
    const long long g = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63);
    if (g >= ngroups) return;
    const int RPW = 64 / L, r = lane / L, q = lane - r * L;
    const int i = rid[g * RPW + r];
    int cnt = 0;
    T d = T(0);
    if (i >= 0) {
        const long long ti = ((long long)i - row_start) * row_step;
        int e = 0;
        for (int p = Ap[i]; p < Ap[i + 1]; ++p) {
            const int j = Aj[p];
            if (j == i) { d = Ax[p]; continue; }
            if (e % L == q) {
                const size_t s = (size_t)((g * K + e / L) * 64 + lane);
                if (j < 0 || j >= n) { cols[s] = LANE_NONE; vals[s] = T(0); }
                else {
                    const long long tj = ((long long)j - row_start) * row_step;
                    const bool early = tj >= 0 && tj < m && tj < ti;
                    cols[s] = j | (early ? LANE_EARLY : 0);
                    vals[s] = Ax[p];
                }
            }
            ++e;
        }
        cnt = e;
    }
    // the slots behind the row's entries: padding (slot es = k * L + q of this lane)
    for (int k = 0; k < K; ++k)
        if (k * L + q >= cnt) {
            const size_t s = (size_t)((g * K + k) * 64 + lane);
            cols[s] = LANE_NONE; vals[s] = T(0);
        }
    if (q == 0) {
        const bool nodiag = !(d != T(0));
        const T rd = (i >= 0 && !nodiag) ? T(1) / d : T(0);
        LaneRec R;
        R.rid = (i >= 0 && nodiag) ? (i | LANE_NODIAG) : i;
        R.gate = gate[g];
        if constexpr (sizeof(T) == 8) { R.rd_lo = __double2loint((double)rd); R.rd_hi = __double2hiint((double)rd); }
        else { R.rd_lo = __float_as_int((float)rd); R.rd_hi = 0; }
        rec[g * RPW + r] = R;
    }
}

int build_lane_part(pamg_matrix_s *A, GsSchedule *g)
{
    if (g->lane) return PAMG_OK;
    PhaseTimer pt_("build_lane_part", A->nnz);
    const int ts = (int)tsize(A->dtype);
    // PAMG_LANE_HOST_FILL=1: the whole layout on the host (what the CPU suite replays); default: filled on the device.  The device
    // fill derives visit indices from (row - row_start) * row_step, which is the host's numbering for unit steps only
    const char *hf = getenv("PAMG_LANE_HOST_FILL");
    const bool host_fill = (hf && *hf == '1') || !A->d_Ap || !A->d_Aj || !A->d_Ax || (g->row_step != 1 && g->row_step != -1);
    PlanVec<unsigned char> hAx;
    if (host_fill) {
        hAx.resize((size_t)A->nnz * ts);
        if (A->nnz) PAMG_HIP(hipMemcpy(hAx.data(), A->d_Ax, (size_t)A->nnz * ts, hipMemcpyDeviceToHost));
    }
    LanePlan P;
    // Lanes per row.  Operators small enough for the one-XCD form (32 CUs): the fewest lanes that hold a row (most rows per
    // wave).  Across the chip waves are plentiful and the sweep is bound by the hand-off latency per dependency level: ONE
    // ROW PER WAVE where the rows are long enough to fill it (a wave then waits for its own row's operands only, not for the
    // slowest of 4 or 16 rows) -- level 1 of the 256^3 hierarchy, 31 entries per row: 2.65 ms with 16 lanes per row, 2.49
    // with 32, 2.37 with 64 (profiles/r04_microbench_lane_width.json).
    int want_L = A->lane_L;
    if (!want_L && !lane_one_xcd(A, g)) {
        want_L = 4;
        while (want_L < 64 && want_L < A->max_row_len - 1) want_L *= 2;
        if (want_L < 32) want_L = 0;                           // short rows: several rows per wave (stencils)
    }
    if (build_lane_plan((int)A->nrows, A->h_Ap.data(), A->h_Aj.data(), host_fill ? hAx.data() : nullptr, ts, g->row_start, g->row_step, (int)g->nrows,
                        g->nlevels, g->h_vis, g->h_lvl, want_L, P, host_fill))
        return PAMG_E_ARG;
    LaneSched *t = new (std::nothrow) LaneSched();
    if (!t) return PAMG_E_ALLOC;
    t->L = P.L; t->K = P.K; t->RPW = P.RPW; t->ngroups = P.ngroups;
    t->n_early = P.n_early; t->n_old = P.n_old; t->n_slots = P.n_slots;
    t->max_level_groups = P.max_level_groups;
    const size_t nrec = (size_t)P.ngroups * P.RPW;
    int st = PAMG_OK;
    if (host_fill) {
        std::vector<LaneRec> rec(nrec);
        for (size_t q = 0; q < nrec; ++q) {
            rec[q].rid = P.rid[q];
            rec[q].gate = P.gate[q / (size_t)P.RPW];
            rec[q].rd_lo = rec[q].rd_hi = 0;
            std::memcpy(&rec[q].rd_lo, &P.rdiag[q * (size_t)ts], (size_t)ts);
        }
        st = device_upload(&t->d_rec, rec.data(), nrec * sizeof(LaneRec), &t->bytes);
        if (!st) st = device_upload(&t->d_cols, P.cols.data(), P.cols.size() * sizeof(int), &t->bytes);
        if (!st) st = device_upload(&t->d_vals, P.vals.data(), P.vals.size(), &t->bytes);
    } else {
        int *d_rid = nullptr, *d_gate = nullptr;
        st = device_upload(&d_rid, P.rid.data(), P.rid.size() * sizeof(int), nullptr);
        if (!st) st = device_upload(&d_gate, P.gate.data(), P.gate.size() * sizeof(int), nullptr);
        if (!st) st = device_upload(&t->d_rec, nullptr, nrec * sizeof(LaneRec), &t->bytes);
        if (!st) st = device_upload(&t->d_cols, nullptr, (size_t)P.n_slots * sizeof(int), &t->bytes);
        if (!st) st = device_upload(&t->d_vals, nullptr, (size_t)P.n_slots * ts, &t->bytes);
        if (!st) {
            const unsigned grid = (unsigned)((P.ngroups + 3) / 4);
            (void)hipGetLastError();                                  // a stale error of an earlier query must not be taken for this launch's
            if (ts == 8)
                hipLaunchKernelGGL((lane_fill_kernel<double>), dim3(grid), dim3(256), 0, 0, (int)A->nrows, A->d_Ap, A->d_Aj, (const double *)A->d_Ax, g->row_start, g->row_step,
                                   (long long)g->nrows, P.L, P.K, (long long)P.ngroups, d_rid, d_gate, t->d_cols, (double *)t->d_vals, t->d_rec);
            else
                hipLaunchKernelGGL((lane_fill_kernel<float>), dim3(grid), dim3(256), 0, 0, (int)A->nrows, A->d_Ap, A->d_Aj, (const float *)A->d_Ax, g->row_start, g->row_step,
                                   (long long)g->nrows, P.L, P.K, (long long)P.ngroups, d_rid, d_gate, t->d_cols, (float *)t->d_vals, t->d_rec);
            st = (int)hipGetLastError();
            if (!st) st = (int)hipDeviceSynchronize();
        }
        hipFree(d_rid); hipFree(d_gate);
    }
    if (st) { free_lane_part(t); return st; }
    g->lane = t;
    g->bytes += t->bytes;                                      // the caller books them on the operator
    return PAMG_OK;
}

size_t lane_part_bytes(const GsSchedule *g) { return (g && g->lane) ? g->lane->bytes : 0; }

// ---- merged form, host side
void free_lanem_part(LaneMSched *t)
{
    if (!t) return;
    hipFree(t->d_cols); hipFree(t->d_vals); hipFree(t->d_rec); hipFree(t->d_prof);
    hipFree(t->d_crec); hipFree(t->d_sidx); hipFree(t->d_crid); hipFree(t->d_crd);
    delete t;
}

size_t lanem_part_bytes(const GsSchedule *g) { return (g && g->lanem) ? g->lanem->bytes : 0; }

// rows per wave of the cluster layout: PAMG_TUNE_LANEM_CLUSTER (4 / 8; 1 = off), 0 = automatic -- 8 on the large levels.  Level 1 of the 256^3 hierarchy, fused
// symmetric launch, 512 workgroups (profiles/r08_lanem_cluster_ab.txt): 3.61 ms in the pair layout at s = 3 (4.31 at s = 4); clusters of 4 / 8 rows
// 3.40 / 3.36 ms at s = 3, 3.15 / 2.95 at s = 4, 3.35 / 3.14 at s = 5 -- a wave that loads 46 unique operands per row instead of 60 affords the longer
// rows of a deeper merge.  The small levels are bound by their hand-offs and keep one row per wave (and the one-XCD ticket form).
int lanem_cluster_rows(const pamg_matrix_s *A)
{
    if (A->lanem_cluster >= 4) return A->lanem_cluster;
    if (A->lanem_cluster == 1) return 0;
    static const int env = [] { const char *e = getenv("PAMG_LANEM_CLUSTER"); return e ? atoi(e) : 0; }();     // A/B: 1 = off, 4 / 8
    if (A->nrows <= 131072 || env == 1) return 0;
    return env == 4 ? 4 : 8;
}

// levels merged per super-level: PAMG_TUNE_LANE_MERGE (1 = unmerged form, >= 2 = that many), 0 = automatic -- rows long enough to fill a wave
// (the SA coarse levels: >= 12 entries per row on average), f64
int lanem_smax(const pamg_matrix_s *A, const GsSchedule *g)
{
    if (A->dtype != PAMG_F64 || A->R != 1 || g->nlevels < 8) return 1;
    if (A->lane_merge == 1) return 1;
    if (A->lane_merge >= 2) return A->lane_merge;
    const char *e = getenv("PAMG_LANE_MERGE");
    if (e && atoi(e) >= 1) return atoi(e);
    if (A->nnz < 12 * std::max<int64_t>(1, A->nrows)) return 1;
    // large levels: 3 in the pair layout (level 1 of the 256^3 hierarchy: 1.80 ms at 2, 1.76 at 3, 2.14 at 4 -- the sweep is bound by rows per second, longer
    // rows cost), 4 in the cluster layout (above);
    // small levels are bound by their hand-offs: 8 (every unit in registers there; level 2, 44.6 K rows: 0.484 ms at 4, 0.447 at 6, 0.440 at 8; level 3,
    // 463 rows: 0.052 / 0.042 / 0.034)
    return A->nrows > 131072 ? (lanem_cluster_rows(A) ? 4 : 3) : 8;
}

static int lanem_to_device(const LaneMPlan &P, int s_max, LaneMSched **out);

int build_lanem_part(pamg_matrix_s *A, GsSchedule *g)
{
    if (g->lanem) return PAMG_OK;
    const int s_max = lanem_smax(A, g);
    if (s_max < 2) return PAMG_E_ARG;
    PhaseTimer pt_("build_lanem_part", A->nnz);
    PlanVec<double> hAx;
    hAx.resize((size_t)A->nnz + 1);
    if (A->nnz) PAMG_HIP(hipMemcpy(hAx.data(), A->d_Ax, (size_t)A->nnz * sizeof(double), hipMemcpyDeviceToHost));
    LaneMPlan P;
    // two rows per wave (32 lanes each, rows of a super-level paired by length) on the large levels: a fifth fewer padded slots (1.14 instead of 1.44
    // units per row on level 1 of the 256^3 hierarchy) and 1.74 instead of 1.81 ms -- the sweep there is bound by what the memory system delivers per
    // row, not by waves or hand-offs (profiles/r06_microbench_lanem_rows_per_wave.json); small levels are bound by their hand-offs: a wave that waits
    // for ITS row only (PAMG_TUNE_LANEM_RPW: 1 / 2, 0 = this rule)
    const int rpw = A->lanem_rpw ? A->lanem_rpw : (A->nrows > 131072 ? 2 : 1);
    const int cluster = lanem_cluster_rows(A);
    if (build_lanem_plan((int)A->nrows, A->h_Ap.data(), A->h_Aj.data(), hAx.data(), g->row_start, g->row_step, (int)g->nrows, g->nlevels, g->h_vis, g->h_lvl,
                         s_max, 1e3, P, LANEM_KMAX * 64, rpw, cluster))
        return PAMG_E_ARG;
    hAx = PlanVec<double>();
    LaneMSched *t = nullptr;
    PAMG_TRY(lanem_to_device(P, s_max, &t));
    if (!g->d_xold) {                                          // the snapshot of x (allocated here: sweeps may run inside a graph capture)
        const size_t xb = ((size_t)A->nrows + 8) * sizeof(double);
        const int st = (int)hipMalloc(&g->d_xold, xb);
        if (st) { free_lanem_part(t); return st; }
        t->bytes += xb;
    }
    g->lanem = t;
    g->bytes += t->bytes;
    return PAMG_OK;
}

// a finished plan -> its device arrays.  PAMG_E_ARG: nothing gained (every group closed at once: an operator the growth bound rejects) -- the
// unmerged form is the cheaper layout
static int lanem_to_device(const LaneMPlan &P, int s_max, LaneMSched **out)
{
    *out = nullptr;
    if (P.nsuper * 10 > P.nlevels * 9) return PAMG_E_ARG;
    LaneMSched *t = new (std::nothrow) LaneMSched();
    if (!t) return PAMG_E_ALLOC;
    t->ngroups = P.ngroups; t->n_units = P.n_units; t->nrows = P.nrows; t->rpw = P.rpw; t->nsuper = P.nsuper; t->nlevels = P.nlevels; t->s_max = s_max; t->max_len = P.max_len;
    t->closed_by_length = P.closed_by_length; t->closed_by_growth = P.closed_by_growth; t->max_growth = P.max_growth;
    t->n_early = P.n_early; t->n_old = P.n_old; t->n_b = P.n_b; t->max_super_groups = P.max_super_groups;
    t->super_grp = P.super_grp;
    t->cluster = P.cluster; t->n_uunits = P.n_uunits; t->n_uearly = P.n_uearly; t->n_uold = P.n_uold; t->n_ub = P.n_ub; t->n_early_lines = P.n_early_lines;
    if (P.cluster) {
        std::vector<int4> crec((size_t)P.ngroups);
        lane_parallel(P.ngroups, [&](int64_t g0, int64_t g1) {
            for (int64_t q = g0; q < g1; ++q)
                crec[(size_t)q] = make_int4(P.gate[(size_t)q], P.c_uunit[(size_t)q], P.c_sunit[(size_t)q],
                                            (int)P.c_KU[(size_t)q] | ((int)P.c_KS[(size_t)q] << 8) | ((int)P.c_rows[(size_t)q] << 16));
        });
        int st = device_upload(&t->d_crec, crec.data(), crec.size() * sizeof(int4), &t->bytes);
        if (!st) st = device_upload(&t->d_cols, P.ucodes.data(), P.ucodes.size() * sizeof(int), &t->bytes);
        if (!st) st = device_upload(&t->d_vals, P.svals.data(), P.svals.size() * sizeof(double), &t->bytes);
        if (!st) st = device_upload(&t->d_sidx, P.sidx.data(), P.sidx.size() * sizeof(unsigned short), &t->bytes);
        if (!st) st = device_upload(&t->d_crid, P.rid.data(), P.rid.size() * sizeof(int), &t->bytes);
        if (!st) st = device_upload(&t->d_crd, P.rdiag.data(), P.rdiag.size() * sizeof(double), &t->bytes);
        if (st) { free_lanem_part(t); return st; }
        if (getenv("PAMG_TIMING")) fprintf(stderr, "[pamg timing]     lanem plan: cluster layout, %d rows per wave: %zu bytes uploaded\n", P.cluster, t->bytes);
        *out = t;
        return PAMG_OK;
    }
    std::vector<LaneMRec> rec((size_t)P.ngroups);
    lane_parallel(P.ngroups, [&](int64_t g0, int64_t g1) {
        for (int64_t q = g0; q < g1; ++q) {
            LaneMRec &R = rec[(size_t)q];
            const size_t q0 = (size_t)q * (size_t)P.rpw;
            const double zero = 0.0;
            R.rid_a = P.rid[q0]; R.rid_b = P.rpw == 2 ? P.rid[q0 + 1] : -1;
            R.gate = P.gate[(size_t)q];
            R.unitK = P.unit[(size_t)q] * 16 + (int)P.K[(size_t)q];
            std::memcpy(&R.rda_lo, &P.rdiag[q0], 8);
            std::memcpy(&R.rdb_lo, P.rpw == 2 ? &P.rdiag[q0 + 1] : &zero, 8);
        }
    });
    int st = device_upload(&t->d_rec, rec.data(), rec.size() * sizeof(LaneMRec), &t->bytes);
    if (!st) st = device_upload(&t->d_cols, P.cols.data(), P.cols.size() * sizeof(int), &t->bytes);
    if (!st) st = device_upload(&t->d_vals, P.vals.data(), P.vals.size() * sizeof(double), &t->bytes);
    if (st) { free_lanem_part(t); return st; }
    if (getenv("PAMG_TIMING")) fprintf(stderr, "[pamg timing]     lanem plan: %d row(s) per wave: %zu bytes uploaded\n", P.rpw, t->bytes);
    *out = t;
    return PAMG_OK;
}

// =================================================================== zero-iterate plans (PAMG_TUNE_ZERO_PLANS)
// A cycle enters every coarse level with x = 0 (cycle_rec), and a symmetric sweep from zero needs half the operator in each direction:
//   forward : (D + L) y = b -- the strictly upper entries multiply zeros;
//   backward: after the forward sweep b_r - sum_{j<r} a_rj y_j = a_rr y_r for every updated row r, so the backward half is the backward sweep of
//             the UPPER triangle, (D + U) x = w with w_r = a_rr y_r: the numerator b_r - s_r the forward row holds before it multiplies by 1 / a_rr.
// The planner is linear in the operator's entries: Zf = the forward plan of tril(A), Zb = the backward plan of triu(A), same layouts and gates as the
// general plans, built from host copies of the triangles (no second device copy of the operator).  Rows without a usable diagonal keep their old
// value; they are the only source of OLD operands in these plans.  The forward kernel stores w (LaneMArgs::w), the backward kernel runs with b = w.
// Depth: PAMG_TUNE_ZERO_MERGE (2..16), 0 = automatic -- what won the scan of the 256^3 hierarchy by more than the spread of three repetitions (0.1 - 0.2 %),
// fused launch announced to start from zero (profiles/r09_microbench_zero_plan_scan.json; the general plans in the same session: level 1 2.92 ms, level 2 0.924):
//   level 1 (2.03 M rows, cluster layout, 512 workgroups): s = 4 2.556 ms, 5 2.298, 6 2.269, 8 2.804 (2.448 with 768 workgroups; s = 4 / 5 / 6 lose 2 - 5 %
//            with 768) -- a triangular row at s = 6 carries 62.5 operands, 30 unique per row: less than the full plan at s = 4 (78.6 / 46.2), with 374
//            instead of 561 hand-offs per direction;
//   level 2 (44.6 K rows, one row per wave): s = 8 0.831 ms, 12 0.811, 16 0.806 (142 / 128 / 123 super-levels; the full plan closes 217 at the
//            512-operand cap, and from s = 12 on most of these groups close there too).
int lanem_zero_smax(const pamg_matrix_s *A)
{
    if (A->zero_merge >= 2) return A->zero_merge;
    static const int env = [] { const char *e = getenv("PAMG_ZERO_MERGE"); return e ? atoi(e) : 0; }();
    if (env >= 2) return env;
    return A->nrows > 131072 ? 6 : 16;
}

int build_zero_plan(pamg_matrix_s *A, int dir)
{
    if (dir < 0 || dir > 1 || A->zplan[dir]) return PAMG_OK;
    if (A->dtype != PAMG_F64 || A->R != 1 || A->nrows < 2 || A->nrows != A->ncols || !A->d_Ax) return PAMG_E_ARG;
    PhaseTimer pt_(dir ? "build_zero_plan (backward, triu)" : "build_zero_plan (forward, tril)", A->nnz);
    const int n = (int)A->nrows;
    PlanVec<double> hAx;
    hAx.resize((size_t)A->nnz + 1);
    if (A->nnz) PAMG_HIP(hipMemcpy(hAx.data(), A->d_Ax, (size_t)A->nnz * sizeof(double), hipMemcpyDeviceToHost));
    // the triangle with its diagonal, entries in storage order
    const int *Ap = A->h_Ap.data(), *Aj = A->h_Aj.data();
    std::vector<int> Tp((size_t)n + 1, 0);
    lane_parallel(n, [&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            int c = 0;
            for (int p = Ap[i]; p < Ap[i + 1]; ++p) c += dir ? (Aj[p] >= (int)i) : (Aj[p] <= (int)i);
            Tp[(size_t)i + 1] = c;
        }
    });
    for (int i = 0; i < n; ++i) Tp[(size_t)i + 1] += Tp[(size_t)i];
    PlanVec<int> Tj;
    PlanVec<double> Tx;
    Tj.resize((size_t)Tp[(size_t)n] + 1);
    Tx.resize((size_t)Tp[(size_t)n] + 1);
    lane_parallel(n, [&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            int q = Tp[(size_t)i];
            for (int p = Ap[i]; p < Ap[i + 1]; ++p)
                if (dir ? (Aj[p] >= (int)i) : (Aj[p] <= (int)i)) { Tj[(size_t)q] = Aj[p]; Tx[(size_t)q] = hAx[(size_t)p]; ++q; }
        }
    });
    hAx = PlanVec<double>();
    std::vector<int> vis, lvl;
    int m = 0, nl = 0;
    if (sweep_levels(n, Tp.data(), Tj.data(), dir ? n - 1 : 0, dir ? -1 : n, dir ? -1 : 1, vis, lvl, m, nl) || m != n || nl < 8) return PAMG_E_ARG;
    const int s_max = lanem_zero_smax(A);
    const int rpw = A->lanem_rpw ? A->lanem_rpw : (A->nrows > 131072 ? 2 : 1);
    LaneMPlan P;
    if (build_lanem_plan(n, Tp.data(), Tj.data(), Tx.data(), dir ? n - 1 : 0, dir ? -1 : 1, m, nl, vis, lvl, s_max, 1e3, P, LANEM_KMAX * 64, rpw, lanem_cluster_rows(A)))
        return PAMG_E_ARG;
    LaneMSched *t = nullptr;
    PAMG_TRY(lanem_to_device(P, s_max, &t));
    A->zplan[dir] = t;
    return PAMG_OK;
}

void free_zero_plans(pamg_matrix_s *A)
{
    for (int d = 0; d < 2; ++d) { free_lanem_part(A->zplan[d]); A->zplan[d] = nullptr; }
    hipFree(A->d_zw);
    A->d_zw = nullptr;
}

size_t zero_plan_bytes(const pamg_matrix_s *A)
{
    size_t b = A->d_zw ? ((size_t)A->nrows + 8) * sizeof(double) : 0;
    for (int d = 0; d < 2; ++d) if (A->zplan[d]) b += A->zplan[d]->bytes;
    return b;
}

// both plans in the layout of the general plans of the two schedules, and the numerator vector
bool zero_plans_ready(const pamg_matrix_s *A, const GsSchedule *gf, const GsSchedule *gb)
{
    const LaneMSched *zf = A->zplan[0], *zb = A->zplan[1];
    if (A->zero_plans == 1 || !zf || !zb || !A->d_zw || !gf || !gb || !gf->lanem || !gb->lanem) return false;
    return zf->rpw == zb->rpw && zf->cluster == zb->cluster && zf->rpw == gf->lanem->rpw && zf->cluster == gf->lanem->cluster &&
           zb->rpw == gb->lanem->rpw && zb->cluster == gb->lanem->cluster && zf->ngroups >= 1 && zb->ngroups >= 1;
}

// the layout-dependent operands of a launch
static void lanem_layout_args(const LaneMSched *t, LaneMArgs &a)
{
    a.cols = t->d_cols; a.vals = t->d_vals;
    a.rec = t->cluster ? reinterpret_cast<const LaneMRec *>(t->d_crec) : t->d_rec;
    a.sidx = t->d_sidx; a.crid = t->d_crid; a.crd = t->d_crd; a.crows = t->cluster;
}

// the instantiation of a layout: the cluster layout (static form only), two rows per wave with four units in registers, one row per wave with
// every unit (all_regs) or two in registers; xcd: the ticket form inside one XCD.  Z as in the kernels
template <int Z>
static const void *lanem_kernel(int cluster, int rpw, bool all_regs, bool xcd)
{
    if (cluster) return (const void *)gs_lanem_kernel<0, 0, 8, Z>;
    if (rpw == 2) return xcd ? (const void *)gs_lanem_kernel<1, 2, 4, Z> : (const void *)gs_lanem_kernel<0, 2, 4, Z>;
    if (all_regs) return xcd ? (const void *)gs_lanem_kernel<1, 1, 8, Z> : (const void *)gs_lanem_kernel<0, 1, 8, Z>;
    return xcd ? (const void *)gs_lanem_kernel<1, 1, 2, Z> : (const void *)gs_lanem_kernel<0, 1, 2, Z>;
}
template <int Z>
static const void *lanem_sym_kernel(int cluster, int rpw, bool all_regs, bool xcd)
{
    if (cluster) return (const void *)gs_lanem_sym_kernel<0, 0, 8, Z>;
    if (rpw == 2) return xcd ? (const void *)gs_lanem_sym_kernel<1, 2, 4, Z> : (const void *)gs_lanem_sym_kernel<0, 2, 4, Z>;
    if (all_regs) return xcd ? (const void *)gs_lanem_sym_kernel<1, 1, 8, Z> : (const void *)gs_lanem_sym_kernel<0, 1, 8, Z>;
    return xcd ? (const void *)gs_lanem_sym_kernel<1, 1, 2, Z> : (const void *)gs_lanem_sym_kernel<0, 1, 2, Z>;
}

// every unit of a row in registers: one-row-per-wave plans of the small levels (PAMG_LANEM_NREG, A/B: 2 / 8 units whatever the level)
static bool lanem_all_regs(const pamg_matrix_s *A, const LaneMSched *t)
{
    static const int nreg_env = [] { const char *e = getenv("PAMG_LANEM_NREG"); return e ? atoi(e) : 0; }();
    return t->rpw == 1 && (nreg_env ? nreg_env == 8 : A->nrows <= 131072);
}

// the ticket form inside one XCD only for tiny levels: one row per group means one ticket per ROW, and the ticket counter is one address whose
// atomics serialise (11.4 ns each) -- level 2 of the 256^3 hierarchy (44.6 K rows): 0.58 ms inside one XCD, 0.48 across the chip
// (the cluster layout: static form only)
static bool lanem_one_xcd(const pamg_matrix_s *A, const GsSchedule *g, const LaneMSched *t)
{
    return !t->cluster && (A->gran_xcd == 1 || (A->gran_xcd == 0 && lane_one_xcd(A, g) && A->nrows <= ONE_XCD_MAX_ROWS));
}

// workgroups a plan wants, given `cap` co-resident ones per CU on `cus` CUs
static int lanem_want_grid(const pamg_matrix_s *A, const LaneMSched *t, int cap, int cus)
{
    // waves wanted: 4 x the rows of an average super-level (level 2 of the 256^3 hierarchy, 199 rows per super-level at s = 6: 0.487 ms with 115
    // workgroups, 0.459 with 192, 0.473 with 256, 0.52 with 384), capped below
    const int per_level = (int)((t->ngroups + t->nsuper - 1) / std::max(1, t->nsuper));
    const int64_t want_waves = std::max<int64_t>(128, ((int64_t)A->lanem_ahead10 * per_level + 9) / 10);
    // three workgroups per CU at most: from 768 workgroups on the sweep delivers what it delivers, more waves only slow each other down
    // (level 1 of the 256^3 hierarchy, s = 3: 1.76 ms with 768 workgroups, 1.88 with 1 024, 2.17 with 1 536, 2.33 with 1 792)
    // (two rows per wave, s = 3: 1.74 ms with 512 workgroups, 1.89 with 768, 2.08 with 1 024: two per CU)
    int G = (int)std::min<int64_t>((want_waves + LANE_WPB - 1) / LANE_WPB, (int64_t)std::min(cap, (t->rpw == 2 || t->cluster) ? 2 : 3) * cus);
    if (A->lane_G > 0) G = std::min(A->lane_G, cap * cus);
    return (int)std::max<int64_t>(1, std::min<int64_t>(G, (t->ngroups + LANE_WPB - 1) / LANE_WPB));
}

// t: the schedule's own plan, or a zero-iterate plan of the operator run on the schedule's buffers (w: where Zf stores its numerators)
// acc: the backward half of the correction form -- the schedule's snapshot already holds the forward half's values (the caller swept into it), so
// only the hand-off buffer is prepared, and the kernel adds its values to x
static int lanem_launch_plan(pamg_matrix_s *A, GsSchedule *g, LaneMSched *t, void *x, const void *b, double *w, hipStream_t s, bool acc = false)
{
    if (!t || !g->d_xold) return PAMG_E_STATE;
    const int64_t n = A->nrows;
    LaneMArgs a;
    lanem_layout_args(t, a);
    a.use_gate = (A->lane_flags & 1) ? 1 : 0;
    a.xold = (const double *)g->d_xold; a.y = (double *)x; a.xs = (double *)g->d_xs; a.b = (const double *)b;
    a.w = w;
    a.err = g->d_sync + 1; a.ticket = g->d_sync + 20;
    a.ngroups = (int)t->ngroups;
    a.nidle = (int)std::max<int64_t>(1, std::min<int64_t>(n, 1 << 20));
    if (A->gs_prof && !t->cluster) PAMG_TRY(ensure_profile(&t->d_prof, t->ngroups));
    a.prof = (A->gs_prof && !t->cluster) ? t->d_prof : nullptr;
    const int fgrid = (int)std::min<int64_t>(4096, (n + BLK - 1) / BLK);
    if (acc) hipLaunchKernelGGL((fill_sentinel_kernel<double>), dim3(fgrid), dim3(BLK), 0, s, (double *)g->d_xs, n);
    else hipLaunchKernelGGL(lanem_prepare_kernel, dim3(fgrid), dim3(BLK), 0, s, (const double *)x, (double *)g->d_xold, (double *)g->d_xs, n);
    PAMG_HIP(hipGetLastError());
    const bool xcd = lanem_one_xcd(A, g, t);
    const bool all_regs = lanem_all_regs(A, t);
    const int Z = acc ? 2 : w ? 1 : 0;
    const void *k = Z == 0 ? lanem_kernel<0>(t->cluster, t->rpw, all_regs, xcd)
                  : Z == 1 ? lanem_kernel<1>(t->cluster, t->rpw, all_regs, xcd)
                           : lanem_kernel<2>(t->cluster, t->rpw, all_regs, xcd);
    const int cus = device_cus();
    const int cap = resident_cap(t->cap, t->cap_kernel, k);
    void *args[] = {(void *)&a};
    return launch_persistent(k, args, lanem_want_grid(A, t, cap, cus), xcd, g->d_sync + 20, cus, cap, &t->last_grid, s);
}

int lanem_launch(pamg_matrix_s *A, GsSchedule *g, void *x, const void *b, hipStream_t s) { return lanem_launch_plan(A, g, g->lanem, x, b, nullptr, s); }

// the symmetric sweep from x = 0 as two launches on the zero-iterate plans (PAMG_TUNE_SYM_FUSED = 0, or where the fused kernel does not apply): what the
// fused launch computes, bit for bit -- the same plans, the same row sums, w across the kernel boundary
// acc: the correction form, x += sweep(0, b).  The forward half sweeps a zeroed vector -- the backward schedule's snapshot buffer, which the backward
// half would otherwise fill with a copy of exactly these values -- and the backward half adds what it computes to x: no scratch vector, no copy, no add pass
int lanem_zero_pair_launch(pamg_matrix_s *A, GsSchedule *gf, GsSchedule *gb, void *x, const void *b, bool acc, hipStream_t s)
{
    if (!zero_plans_ready(A, gf, gb)) return PAMG_E_UNSUPPORTED;
    if (acc) {
        if (!gb->d_xold) return PAMG_E_STATE;
        PAMG_HIP(hipMemsetAsync(gb->d_xold, 0, (size_t)A->nrows * sizeof(double), s));
        PAMG_TRY(lanem_launch_plan(A, gf, A->zplan[0], gb->d_xold, b, (double *)A->d_zw, s));
        PAMG_TRY(lanem_launch_plan(A, gb, A->zplan[1], x, A->d_zw, nullptr, s, true));
    } else {
        PAMG_TRY(lanem_launch_plan(A, gf, A->zplan[0], x, b, (double *)A->d_zw, s));
        PAMG_TRY(lanem_launch_plan(A, gb, A->zplan[1], x, A->d_zw, nullptr, s));
    }
    A->zero_plan_launches++;
    return PAMG_OK;
}

int sym_fill_sentinels(void *p, int64_t n)
{
    if (n <= 0) return PAMG_OK;
    const int fgrid = (int)std::min<int64_t>(4096, (n + BLK - 1) / BLK);
    hipLaunchKernelGGL((fill_sentinel_kernel<double>), dim3(fgrid), dim3(BLK), 0, 0, (double *)p, n);
    PAMG_HIP(hipGetLastError());
    PAMG_HIP(hipDeviceSynchronize());
    return PAMG_OK;
}

// The fused symmetric sweep (gs_lanem_sym_kernel).  PAMG_E_UNSUPPORTED: the two schedules would not run the same kernel -- the caller sweeps
// them one after the other.  The grid is the larger of the two directional wishes (lanem_want_grid) under the fused kernel's own co-residency cap.
// acc: the correction form, x += sweep(0, b), on the zero-iterate plans (PAMG_E_UNSUPPORTED without them): the launch announced from zero whose second
// phase adds to x
int lanem_sym_launch(pamg_matrix_s *A, GsSchedule *gf, GsSchedule *gb, void *x, const void *b, bool x_zero, hipStream_t s, bool acc)
{
    LaneMSched *tf = gf->lanem, *tb = gb->lanem;
    if (!tf || !tb || !A->d_sym_hf[0] || !A->d_sym_hf[1] || !A->d_sym_hb || !A->d_sym_sync) return PAMG_E_STATE;
    if (acc && !zero_plans_ready(A, gf, gb)) return PAMG_E_UNSUPPORTED;
    if (acc) x_zero = true;                                     // (the VIRTUAL iterate is zero: phase 1 skips its OLD operands)
    // x = 0 and the operator holds its zero-iterate plans: phase 1 runs Zf and stores the numerators, phase 2 runs Zb on them
    const bool zero = x_zero && zero_plans_ready(A, gf, gb);
    if (zero) { tf = A->zplan[0]; tb = A->zplan[1]; }
    const int64_t n = A->nrows;
    const bool xcd = lanem_one_xcd(A, gf, gf->lanem);
    if (xcd != lanem_one_xcd(A, gb, gb->lanem) || tf->rpw != tb->rpw || tf->cluster != tb->cluster || tf->ngroups < 1 || tb->ngroups < 1) return PAMG_E_UNSUPPORTED;
    LaneMSymArgs a;
    LaneMSched *ts2[2] = {tf, tb};
    for (int p = 0; p < 2; ++p) {
        LaneMSched *t = ts2[p];
        LaneMArgs &q = a.ph[p];
        lanem_layout_args(t, q);
        q.use_gate = (A->lane_flags & 1) ? 1 : 0;
        q.b = (const double *)b;
        q.w = nullptr;
        q.err = gf->d_sync + 1; q.ticket = nullptr;
        q.ngroups = (int)t->ngroups;
        q.nidle = (int)std::max<int64_t>(1, std::min<int64_t>(n, 1 << 20));
        q.prof = nullptr;
        a.wq[p] = (int)(n / t->ngroups); a.wr[p] = (int)(n % t->ngroups);
        a.wblk[p] = 1;                                          // groups per wipe block: the power of two whose groups own >= 64 entries together
        while ((int64_t)a.wblk[p] * n < 64 * t->ngroups && a.wblk[p] < (1 << 20)) a.wblk[p] *= 2;
    }
    a.ph[0].xold = (const double *)x; a.ph[0].y = nullptr;     a.ph[0].xs = nullptr;                     // (xs / xold of the parity's H_f: set by the kernel)
    a.ph[1].xold = nullptr;           a.ph[1].y = (double *)x; a.ph[1].xs = (double *)A->d_sym_hb;
    if (zero) { a.ph[0].w = (double *)A->d_zw; a.ph[1].b = (const double *)A->d_zw; }
    a.hf[0] = (double *)A->d_sym_hf[0]; a.hf[1] = (double *)A->d_sym_hf[1];
    a.sync = A->d_sym_sync;
    a.xzero = x_zero ? 1 : 0;
    const bool all_regs = lanem_all_regs(A, tf);
    const int Z = acc ? 2 : zero ? 1 : 0;
    const void *k = Z == 0 ? lanem_sym_kernel<0>(tf->cluster, tf->rpw, all_regs, xcd)
                  : Z == 1 ? lanem_sym_kernel<1>(tf->cluster, tf->rpw, all_regs, xcd)
                           : lanem_sym_kernel<2>(tf->cluster, tf->rpw, all_regs, xcd);
    const int cus = device_cus();
    // (the kernels alternate within a cycle: one cached answer each)
    const int cap = acc  ? resident_cap(A->csym_cap, A->csym_cap_kernel, k)
                  : zero ? resident_cap(A->zsym_cap, A->zsym_cap_kernel, k)
                         : resident_cap(A->sym_cap, A->sym_cap_kernel, k);
    int G = std::max(lanem_want_grid(A, tf, cap, cus), lanem_want_grid(A, tb, cap, cus));      // the larger wish of the two directions
    if (xcd) G = 8 * std::max(1, std::min(G, (cus / 8) * cap));   // 8x the wanted grid; the workgroups off the home XCD leave at once
    void *args[] = {(void *)&a};
    PAMG_HIP(hipLaunchKernel(k, dim3(G), dim3(BLK), args, 0, s));
    A->sym_form = xcd ? 3 : 1; A->sym_grid = G;
    if (zero) tf->last_grid = tb->last_grid = G;               // (diagnostics: the grid of the zero-iterate launch, which differs from the general one's)
    else A->sym_general_grid = G;
    A->sym_launches++;
    if (x_zero) A->sym_zero_launches++;
    if (zero) A->zero_plan_launches++;
    return PAMG_OK;
}

// info[0..11] = super-levels, dependency levels, groups (rows), 64-slot units, early / old / b operands, longest merged row, levels merged at most,
//               groups closed early by length / by growth, workgroups of the last launch;  growth = largest accepted growth factor
// info[12..19] = rows per wave of the cluster layout (0: the row / pair layout), groups (waves' work items), padded slots (64 x units), units of unique
//               operands, unique early / old / b operands and distinct 64-byte lines of the unique early operands, each summed over the groups (the
//               row / pair layouts share nothing: their unique operands ARE info[4..6], lines are not counted)
int lanem_info(const GsSchedule *g, int64_t *info, double *growth) { return lanem_plan_info(g ? g->lanem : nullptr, info, growth); }

int lanem_plan_info(const LaneMSched *t, int64_t *info, double *growth)
{
    for (int i = 0; i < 20; ++i) info[i] = 0;
    if (growth) *growth = 0.0;
    if (!t) return PAMG_OK;
    info[0] = t->nsuper; info[1] = t->nlevels; info[2] = t->nrows; info[3] = t->n_units; info[4] = t->n_early; info[5] = t->n_old; info[6] = t->n_b;
    info[7] = t->max_len; info[8] = t->s_max; info[9] = t->closed_by_length; info[10] = t->closed_by_growth; info[11] = t->last_grid;
    info[12] = t->cluster; info[13] = t->ngroups; info[14] = t->n_units * 64; info[15] = t->n_uunits;
    info[16] = t->cluster ? t->n_uearly : t->n_early; info[17] = t->cluster ? t->n_uold : t->n_old; info[18] = t->cluster ? t->n_ub : t->n_b; info[19] = t->n_early_lines;
    if (growth) *growth = t->max_growth;
    return PAMG_OK;
}


template <typename T>
static int lane_launch_t(pamg_matrix_s *A, GsSchedule *g, int epi, void *x, const void *b, double omega, hipStream_t s)
{
    LaneSched *t = g->lane;
    const size_t ts = tsize(A->dtype);
    const int64_t n = A->nrows;
    LaneArgs<T> a;
    a.cols = t->d_cols; a.vals = (const T *)t->d_vals; a.rec = t->d_rec;
    a.use_gate = (A->lane_flags & 1) ? 1 : 0;
    a.x = (const T *)x; a.y = (T *)x; a.xs = (T *)g->d_xs; a.b = (const T *)b;
    a.err = g->d_sync + 1; a.ticket = g->d_sync + 20;
    a.ngroups = (int)t->ngroups;
    a.nidle = (int)std::max<int64_t>(1, std::min<int64_t>(n, 1 << 20));
    a.omega = (T)omega;
    if (!g->symmetric) {
        // write-after-read hazards are not ordered by the waits: old values come from a snapshot
        if (!g->d_xold) return PAMG_E_STATE;
        PAMG_HIP(hipMemcpyAsync(g->d_xold, x, (size_t)n * ts, hipMemcpyDeviceToDevice, s));
        a.x = (const T *)g->d_xold;
    }
    if (A->gs_prof) PAMG_TRY(ensure_profile(&t->d_prof, t->ngroups));
    a.prof = A->gs_prof ? t->d_prof : nullptr;
    const int fgrid = (int)std::min<int64_t>(4096, (n + BLK - 1) / BLK);
    hipLaunchKernelGGL((fill_sentinel_kernel<T>), dim3(fgrid), dim3(BLK), 0, s, (T *)g->d_xs, n);
    PAMG_HIP(hipGetLastError());
    const int per_level = (int)((t->ngroups + g->nlevels - 1) / g->nlevels);
    const bool xcd = lane_one_xcd(A, g);
    const void *k = lane_kernel<T>(epi, t->L, t->K, xcd ? 1 : 0);
    if (!k) return PAMG_E_ARG;
    const int cus = device_cus();
    const int cap = resident_cap(t->cap, t->cap_kernel, k);
    // waves wanted: ~4 dependency levels of look-ahead (a wave that runs ahead waits in its poll loop with its operands in
    // registers) -- more waves poll more and the polls load the memory system (measured on the 256^3 hierarchy,
    // profiles/r04_microbench_lane_first.json: level 1, 227 groups per dependency level: 2.67 ms with 512 waves, 2.72 with
    // 1 024, 3.28 with 2 048, 4.71 with 4 096)
    // with one row per wave 2.3 levels: 2.37 ms with 2 048 waves, 2.40 with 3 072, 2.57 with 6 144, 2.46 with 1 536)
    const int64_t want_waves = std::max<int64_t>(128, t->RPW == 1 ? ((int64_t)23 * per_level + 9) / 10 : (int64_t)4 * per_level);
    int G = (int)std::min<int64_t>((want_waves + LANE_WPB - 1) / LANE_WPB, (int64_t)cap * cus);
    if (A->lane_G > 0) G = std::min(A->lane_G, cap * cus);
    G = (int)std::max<int64_t>(1, std::min<int64_t>(G, (t->ngroups + LANE_WPB - 1) / LANE_WPB));
    void *args[] = {(void *)&a};
    return launch_persistent(k, args, G, xcd, g->d_sync + 20, cus, cap, &t->last_grid, s);
}

int lane_launch(pamg_matrix_s *A, GsSchedule *g, int epi, void *x, const void *b, double omega, hipStream_t s)
{
    if (g->lanem && epi != EPI_SOR && A->dtype == PAMG_F64) return lanem_launch(A, g, x, b, s);
    if (!g->lane) return PAMG_E_STATE;                       // built by the caller (pamg_matrix.hip: gs_sweep_scalar_t)
    if (A->dtype == PAMG_F64) return lane_launch_t<double>(A, g, epi, x, b, omega, s);
    return lane_launch_t<float>(A, g, epi, x, b, omega, s);
}

// info[0..7] = lanes per row, slots per lane, groups, entry slots, early entries, workgroups of the last launch, widest level (groups), bytes
int lane_info(const GsSchedule *g, int64_t *info)
{
    for (int i = 0; i < 8; ++i) info[i] = 0;
    if (!g || !g->lane) return PAMG_OK;
    const LaneSched *t = g->lane;
    info[0] = t->L; info[1] = t->K; info[2] = t->ngroups; info[3] = t->n_slots; info[4] = t->n_early; info[5] = t->last_grid;
    info[6] = t->max_level_groups; info[7] = (int64_t)t->bytes;
    return PAMG_OK;
}

// first row of every super-level of the merged plan (nsuper + 1 values)
int lanem_levels(const GsSchedule *g, int64_t *out, int64_t cap, int64_t *n)
{
    *n = 0;
    if (!g || !g->lanem) return PAMG_OK;
    *n = (int64_t)g->lanem->super_grp.size();
    if (out && cap >= *n) std::memcpy(out, g->lanem->super_grp.data(), (size_t)*n * sizeof(int64_t));
    return PAMG_OK;
}

int lane_profile(const GsSchedule *g, long long *out, int64_t cap, int64_t *n)
{
    *n = 0;
    // merged form: per ROW {arrival | spins << 52, slots arrived, all operands present, published}
    if (g && g->lanem && g->lanem->d_prof) return read_profile(g->lanem->d_prof, g->lanem->ngroups, out, cap, n);
    if (!g || !g->lane || !g->lane->d_prof) return PAMG_OK;
    return read_profile(g->lane->d_prof, g->lane->ngroups, out, cap, n);
}

}  // namespace pamg
