// pamg_classical.hip -- the setup of classical (Ruge-Stuben) AMG on the device: strength of connection, the MIS / PMIS splitting,
// direct and classical interpolation.  Layer 1 of the C ABI: HOST arrays in, HOST arrays out, amg_core's argument order.  The per-row
// arithmetic is pamg_classical.h (replayed on the host by tests/classical_emul.cpp); every result is the reference's, bit for bit.
//
//   strength   one lane per row: count, exclusive scan, fill (the row maximum, the filter, magnitudes, the scaling and the dropped zeros
//              in one pass over the row each time)
//   MIS        one plain launch per synchronous round over two state buffers; a node that stays active raises the round's flag, the host
//              reads the flags back every MIS_BATCH rounds.  No persistent kernel, no waiting between workgroups.  PMIS builds the
//              transposed pattern (and with it the in-degree weights) with atomics -- the order inside a transposed row is not
//              reproducible, and a round's decision does not depend on it
//   direct     one lane per row, the sums in stored order
//   classical  a group of W = 8 / 16 / 32 / 64 lanes per F-row by its strong-entry count (the Schwarz size classes): the strong entries
//              staged in LDS (column, value, C/F kind), a lane per strong F-neighbour k computes that k's inner denominator ONCE, then a
//              lane per strong C-neighbour j accumulates its weight over k in stored order.  Rows beyond 64 strong entries: a wave per
//              row that loops, with the kinds and inner denominators in global scratch instead of LDS
#include "pamg_common.h"
#include "pamg_classical.h"
#include "pamg_host_call.h"

#include <climits>

using namespace pamg;

namespace {

constexpr int MIS_BATCH = 8;                // rounds between two read-backs of the activity flags

int cgrid(int64_t n) { return launch_grid(n, BLK, 8192); }

// out[i] = in[0] + ... + in[i-1], out[n] = the total; one workgroup, a chunk per lane
__global__ __launch_bounds__(BLK) void excl_scan_kernel(int n, const int *__restrict__ in, int *__restrict__ out, unsigned *__restrict__ overflow)
{
    __shared__ long long s[BLK];
    const int t = threadIdx.x;
    const long long chunk = ((long long)n + BLK - 1) / BLK;
    const int lo = t * chunk < n ? (int)(t * chunk) : n, hi = lo + chunk < n ? (int)(lo + chunk) : n;
    long long sum = 0;
    for (int i = lo; i < hi; ++i) sum += in[i];
    s[t] = sum;
    __syncthreads();
    if (t == 0) {
        long long run = 0;
        for (int k = 0; k < BLK; ++k) { const long long v = s[k]; s[k] = run; run += v; }
        if (run > INT_MAX || run < 0) *overflow = 1u;
        out[n] = (int)run;
    }
    __syncthreads();
    long long run = s[t];
    for (int i = lo; i < hi; ++i) { const int v = in[i]; out[i] = (int)run; run += v; }
}

// counts -> pointer on the device; *total = ptr[n]
int scan_counts(int n, const int *d_cnt, int *d_ptr, unsigned *d_flag, int *total)
{
    PAMG_HIP(hipMemset(d_flag, 0, sizeof(unsigned)));
    hipLaunchKernelGGL(excl_scan_kernel, dim3(1), dim3(BLK), 0, 0, n, d_cnt, d_ptr, d_flag);
    PAMG_HIP(hipGetLastError());
    unsigned of = 0;
    PAMG_HIP(hipMemcpy(&of, d_flag, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (of) return PAMG_E_UNSUPPORTED;
    PAMG_HIP(hipMemcpy(total, d_ptr + n, sizeof(int), hipMemcpyDeviceToHost));
    return PAMG_OK;
}

// ------------------------------------------------------------------------------------------------ strength of connection
template <bool MIN, bool FILL>
__global__ __launch_bounds__(BLK) void strength_kernel(int n, double theta, const int *__restrict__ Ap, const int *__restrict__ Aj,
                                                       const double *__restrict__ Ax, int *__restrict__ cnt, const int *__restrict__ Sp,
                                                       int *__restrict__ Sj, double *__restrict__ Sx)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) {
        if (FILL) cls::strength_row<MIN>(i, theta, Ap, Aj, Ax, Sj + Sp[i], Sx + Sp[i]);
        else cnt[i] = cls::strength_row<MIN>(i, theta, Ap, Aj, Ax, nullptr, nullptr);
    }
}

template <bool MIN>
int strength(int n, double theta, const int *Ap, int Ap_size, const int *Aj, int Aj_size, const double *Ax, int Ax_size, int *Sp, int Sp_size,
             int *Sj, int Sj_size, double *Sx, int Sx_size)
{
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(n, n, Ap, Ap_size, Aj, Aj_size, &nnz));
    if (nnz > Ax_size || (nnz && !Ax) || !Sp || Sp_size < n + 1) return PAMG_E_ARG;
    Sp[0] = 0;
    if (n == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dAp, *dAj, *dcnt, *dSp, *dSj;
    double *dAx, *dSx;
    unsigned *dflag;
    PAMG_TRY(d.put(&dAp, Ap, (size_t)n + 1)); PAMG_TRY(d.put(&dAj, Aj, (size_t)nnz)); PAMG_TRY(d.put(&dAx, Ax, (size_t)nnz));
    PAMG_TRY(d.get(&dcnt, (size_t)n)); PAMG_TRY(d.get(&dSp, (size_t)n + 1)); PAMG_TRY(d.get(&dflag, 1));
    hipLaunchKernelGGL((strength_kernel<MIN, false>), dim3(cgrid(n)), dim3(BLK), 0, 0, n, theta, dAp, dAj, dAx, dcnt, (const int *)nullptr,
                       (int *)nullptr, (double *)nullptr);
    PAMG_HIP(hipGetLastError());
    int total = 0;
    PAMG_TRY(scan_counts(n, dcnt, dSp, dflag, &total));
    if (total > Sj_size || total > Sx_size || (total && (!Sj || !Sx))) return PAMG_E_ARG;
    PAMG_TRY(d.get(&dSj, (size_t)total)); PAMG_TRY(d.get(&dSx, (size_t)total));
    hipLaunchKernelGGL((strength_kernel<MIN, true>), dim3(cgrid(n)), dim3(BLK), 0, 0, n, theta, dAp, dAj, dAx, (int *)nullptr, (const int *)dSp,
                       dSj, dSx);
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(Sp, dSp, (size_t)n + 1));
    PAMG_TRY(Bufs::fetch(Sj, dSj, (size_t)total));
    PAMG_TRY(Bufs::fetch(Sx, dSx, (size_t)total));
    return PAMG_OK;
}

// ------------------------------------------------------------------------------------------------ MIS / PMIS
// flag |= 1 when an off-diagonal entry (i, j) has no (j, i)
__global__ __launch_bounds__(BLK) void symmetric_kernel(int n, const int *__restrict__ Gp, const int *__restrict__ Gj, unsigned *__restrict__ flag)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) {
        bool bad = false;
        for (int p = Gp[i]; p < Gp[i + 1]; ++p) {
            const int j = Gj[p];
            if (j == i) continue;
            bool found = false;
            for (int q = Gp[j]; q < Gp[j + 1] && !found; ++q) found = Gj[q] == i;
            bad = bad || !found;
        }
        if (bad) atomicOr(flag, 1u);
    }
}

__global__ __launch_bounds__(BLK) void mis_round_kernel(int n, const int *__restrict__ Gp, const int *__restrict__ Gj, const int *__restrict__ Tp,
                                                        const int *__restrict__ Tj, const double *__restrict__ y, const int *__restrict__ prev,
                                                        int *__restrict__ next, int active, int C, int F, unsigned *__restrict__ flag)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) {
        int x = prev[i];
        if (x == active) {
            x = cls::mis_node(i, Gp, Gj, Tp, Tj, y, prev, active, C, F);
            if (x == active) *flag = 1u;                    // every writer stores the same value
        }
        next[i] = x;
    }
}

// rounds until no node is active.  d_x[0] holds the start states; *final_buf = the buffer with the result.  At least the largest active
// node is decided in every round, so n rounds always suffice: needing more is an internal error
int mis_rounds(int n, const int *Gp, const int *Gj, const int *Tp, const int *Tj, const double *y, int *d_x[2], int active, int C, int F,
               unsigned *d_flags, int *final_buf, int *rounds_out)
{
    int cur = 0, rounds = 0;
    bool done = n == 0;
    while (!done) {
        const int batch = std::min(MIS_BATCH, n - rounds);
        if (batch <= 0) return PAMG_E_NOCONV;
        PAMG_HIP(hipMemset(d_flags, 0, sizeof(unsigned) * MIS_BATCH));
        for (int r = 0; r < batch; ++r) {
            hipLaunchKernelGGL(mis_round_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, Gp, Gj, Tp, Tj, y, (const int *)d_x[cur], d_x[cur ^ 1], active,
                               C, F, d_flags + r);
            cur ^= 1;
        }
        PAMG_HIP(hipGetLastError());
        unsigned h[MIS_BATCH];
        PAMG_TRY(Bufs::fetch(h, d_flags, MIS_BATCH));
        for (int r = 0; r < batch; ++r) {
            ++rounds;
            if (!h[r]) { done = true; break; }              // the rounds after it in this batch changed nothing
        }
    }
    *final_buf = cur;
    *rounds_out = rounds;
    return PAMG_OK;
}

// in-degree of the off-diagonal pattern; then the transposed pattern through per-column cursors
__global__ __launch_bounds__(BLK) void indegree_kernel(int n, const int *__restrict__ Sp, const int *__restrict__ Sj, int *__restrict__ deg)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK)
        for (int p = Sp[i]; p < Sp[i + 1]; ++p)
            if (Sj[p] != i) atomicAdd(&deg[Sj[p]], 1);
}

__global__ __launch_bounds__(BLK) void transpose_fill_kernel(int n, const int *__restrict__ Sp, const int *__restrict__ Sj, const int *__restrict__ Tp,
                                                             int *__restrict__ cursor, int *__restrict__ Tj)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK)
        for (int p = Sp[i]; p < Sp[i + 1]; ++p) {
            const int j = Sj[p];
            if (j != i) Tj[Tp[j] + atomicAdd(&cursor[j], 1)] = i;
        }
}

// weights = in-degree + the caller's random numbers; every node starts active (-1)
__global__ __launch_bounds__(BLK) void pmis_init_kernel(int n, const int *__restrict__ deg, const double *__restrict__ rnd, double *__restrict__ y,
                                                        int *__restrict__ x)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) { y[i] = (double)deg[i] + rnd[i]; x[i] = -1; }
}

// _set_dirichlet: a node without a neighbour in S union S^T ends as F
__global__ __launch_bounds__(BLK) void pmis_dirichlet_kernel(int n, const int *__restrict__ Sp, const int *__restrict__ Sj, const int *__restrict__ deg,
                                                             int *__restrict__ x)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) {
        bool any = deg[i] > 0;
        for (int p = Sp[i]; p < Sp[i + 1] && !any; ++p) any = Sj[p] != i;
        if (!any) x[i] = cls::F_NODE;
    }
}

// ------------------------------------------------------------------------------------------------ interpolation
__global__ __launch_bounds__(BLK) void interp_count_kernel(int n, const int *__restrict__ Sp, const int *__restrict__ Sj, const int *__restrict__ splitting,
                                                           int *__restrict__ cnt)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) cnt[i] = cls::interp_count_row(i, Sp, Sj, splitting);
}

// the caller's Pp against the counts of pass 1
__global__ __launch_bounds__(BLK) void interp_check_kernel(int n, const int *__restrict__ Sp, const int *__restrict__ Sj, const int *__restrict__ splitting,
                                                           const int *__restrict__ Pp, unsigned *__restrict__ flag)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK)
        if (Pp[i + 1] - Pp[i] != cls::interp_count_row(i, Sp, Sj, splitting) || (i == 0 && Pp[0] != 0)) atomicOr(flag, 1u);
}

__global__ __launch_bounds__(BLK) void direct_kernel(int n, const int *__restrict__ Ap, const int *__restrict__ Aj, const double *__restrict__ Ax,
                                                     const int *__restrict__ Sp, const int *__restrict__ Sj, const double *__restrict__ Sx,
                                                     const int *__restrict__ splitting, const int *__restrict__ Pp, const int *__restrict__ map,
                                                     int *__restrict__ Pj, double *__restrict__ Px)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) cls::direct_row(i, Ap, Aj, Ax, Sp, Sj, Sx, splitting, Pp, map, Pj, Px);
}

__global__ __launch_bounds__(BLK) void remove_ff_kernel(int n, const int *__restrict__ Sp, const int *__restrict__ Sj, double *__restrict__ Sx,
                                                        const int *__restrict__ splitting)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) cls::remove_ff_row(i, Sp, Sj, Sx, splitting);
}

// C-rows: injection.  F-rows: the outer denominator
__global__ __launch_bounds__(BLK) void classical_prologue_kernel(int n, const int *__restrict__ Ap, const double *__restrict__ Ax, const int *__restrict__ Sp,
                                                                 const int *__restrict__ Sj, const double *__restrict__ Sx,
                                                                 const int *__restrict__ splitting, const int *__restrict__ Pp,
                                                                 const int *__restrict__ map, int *__restrict__ Pj, double *__restrict__ Px,
                                                                 double *__restrict__ den)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) {
        if (splitting[i] == cls::C_NODE) { Pj[Pp[i]] = map[i]; Px[Pp[i]] = 1.0; }
        else den[i] = cls::classical_denominator(i, Ap, Ax, Sp, Sj, Sx);
    }
}

// One group of W lanes per listed F-row.  STAGED: the row has at most W strong entries and lives in LDS; otherwise the lanes loop over the
// row and the kinds / inner denominators live in global scratch aligned with S.  The barriers are reached by every lane of the workgroup
// the same number of times: the outer loop's bounds depend on the workgroup only.
template <int W, bool STAGED>
__global__ __launch_bounds__(BLK) void classical_rows_kernel(int nlist, const int *__restrict__ rows, const int *__restrict__ Ap, const int *__restrict__ Aj,
                                                             const double *__restrict__ Ax, const int *__restrict__ Sp, const int *__restrict__ Sj,
                                                             const double *__restrict__ Sx, const int *__restrict__ splitting,
                                                             const int *__restrict__ Pp, const int *__restrict__ map, const double *__restrict__ den,
                                                             int *__restrict__ Pj, double *__restrict__ Px, int modified, unsigned char *g_kind,
                                                             double *g_inner, double *g_akk)
{
    constexpr int G = BLK / W, LDS = STAGED ? BLK : 1;
    __shared__ int s_col[LDS];
    __shared__ double s_val[LDS], s_inner[LDS], s_akk[LDS];
    __shared__ unsigned char s_kind[LDS];
    const int g = threadIdx.x / W, lane = threadIdx.x % W;
    for (int base = blockIdx.x * G; base < nlist; base += gridDim.x * G) {
        const bool live = base + g < nlist;
        const int i = live ? rows[base + g] : 0;
        const int s0 = live ? Sp[i] : 0, ns = live ? Sp[i + 1] - s0 : 0;
        const int *col = STAGED ? s_col + g * W : Sj + s0;
        const double *val = STAGED ? s_val + g * W : Sx + s0;
        unsigned char *kind = STAGED ? s_kind + g * W : g_kind + s0;
        double *inner = STAGED ? s_inner + g * W : g_inner + s0;
        double *akk = STAGED ? s_akk + g * W : g_akk + s0;
        for (int t = lane; t < ns; t += W) {
            const int c = Sj[s0 + t];
            if (STAGED) { s_col[g * W + t] = c; s_val[g * W + t] = Sx[s0 + t]; }
            kind[t] = cls::strong_kind(i, c, splitting);
        }
        __syncthreads();
        for (int t = lane; t < ns; t += W)
            if (kind[t] == cls::K_F) cls::classical_inner(ns, col, kind, col[t], Ap, Aj, Ax, modified != 0, &inner[t], &akk[t]);
        __syncthreads();
        for (int t = lane; t < ns; t += W)
            if (kind[t] == cls::K_C) {
                const int w = Pp[i] + cls::c_rank(kind, t);
                Pj[w] = map[col[t]];
                Px[w] = cls::classical_weight(ns, col, val, kind, inner, akk, t, Ap, Aj, Ax, modified != 0, den[i]);
            }
        __syncthreads();                                    // the LDS slots are restaged by the next row
    }
}

template <int W, bool STAGED>
void launch_class(int nlist, const int *rows, const int *Ap, const int *Aj, const double *Ax, const int *Sp, const int *Sj, const double *Sx,
                  const int *splitting, const int *Pp, const int *map, const double *den, int *Pj, double *Px, int modified, unsigned char *g_kind,
                  double *g_inner, double *g_akk)
{
    if (!nlist) return;
    const int G = BLK / W;
    hipLaunchKernelGGL((classical_rows_kernel<W, STAGED>), dim3(std::min(8192, (nlist + G - 1) / G)), dim3(BLK), 0, 0, nlist, rows, Ap, Aj, Ax, Sp, Sj,
                       Sx, splitting, Pp, map, den, Pj, Px, modified, g_kind, g_inner, g_akk);
}

struct InterpArgs {
    int n;
    const int *Ap, *Aj; const double *Ax; int Ap_size, Aj_size, Ax_size;
    const int *Sp, *Sj; const double *Sx; int Sp_size, Sj_size, Sx_size;
    const int *splitting; int splitting_size;
    const int *Pp; int Pp_size;
    int *Pj; int Pj_size;
    double *Px; int Px_size;
};

int interp_pass1(int n, const int *Sp, int Sp_size, const int *Sj, int Sj_size, const int *splitting, int splitting_size, int *Pp, int Pp_size)
{
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(n, n, Sp, Sp_size, Sj, Sj_size, &nnz));
    if (!Pp || Pp_size < n + 1 || splitting_size < n || (n && !splitting)) return PAMG_E_ARG;
    Pp[0] = 0;
    if (n == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dSp, *dSj, *dsp, *dcnt, *dPp;
    unsigned *dflag;
    PAMG_TRY(d.put(&dSp, Sp, (size_t)n + 1)); PAMG_TRY(d.put(&dSj, Sj, (size_t)nnz)); PAMG_TRY(d.put(&dsp, splitting, (size_t)n));
    PAMG_TRY(d.get(&dcnt, (size_t)n)); PAMG_TRY(d.get(&dPp, (size_t)n + 1)); PAMG_TRY(d.get(&dflag, 1));
    hipLaunchKernelGGL(interp_count_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, dSp, dSj, dsp, dcnt);
    PAMG_HIP(hipGetLastError());
    int total = 0;
    PAMG_TRY(scan_counts(n, dcnt, dPp, dflag, &total));
    PAMG_TRY(Bufs::fetch(Pp, dPp, (size_t)n + 1));
    return PAMG_OK;
}

// pass 2 of either interpolation; modified < 0: direct
int interp_pass2(const InterpArgs &a, int modified)
{
    const int n = a.n;
    int64_t nnzA = 0, nnzS = 0;
    PAMG_TRY(check_pattern(n, n, a.Ap, a.Ap_size, a.Aj, a.Aj_size, &nnzA));
    PAMG_TRY(check_pattern(n, n, a.Sp, a.Sp_size, a.Sj, a.Sj_size, &nnzS));
    if (nnzA > a.Ax_size || (nnzA && !a.Ax) || nnzS > a.Sx_size || (nnzS && !a.Sx)) return PAMG_E_ARG;
    if (a.splitting_size < n || (n && !a.splitting) || !a.Pp || a.Pp_size < n + 1) return PAMG_E_ARG;
    if (n == 0) return PAMG_OK;
    const int nnzP = a.Pp[n];
    if (nnzP < 0 || nnzP > a.Pj_size || nnzP > a.Px_size || (nnzP && (!a.Pj || !a.Px))) return PAMG_E_ARG;
    PAMG_TRY(have_device());
    Bufs d;
    int *dAp, *dAj, *dSp, *dSj, *dsp, *dPp, *dmap, *dPj;
    double *dAx, *dSx, *dPx;
    unsigned *dflag;
    PAMG_TRY(d.put(&dAp, a.Ap, (size_t)n + 1)); PAMG_TRY(d.put(&dAj, a.Aj, (size_t)nnzA)); PAMG_TRY(d.put(&dAx, a.Ax, (size_t)nnzA));
    PAMG_TRY(d.put(&dSp, a.Sp, (size_t)n + 1)); PAMG_TRY(d.put(&dSj, a.Sj, (size_t)nnzS)); PAMG_TRY(d.put(&dSx, a.Sx, (size_t)nnzS));
    PAMG_TRY(d.put(&dsp, a.splitting, (size_t)n)); PAMG_TRY(d.put(&dPp, a.Pp, (size_t)n + 1));
    PAMG_TRY(d.get(&dmap, (size_t)n + 1)); PAMG_TRY(d.get(&dPj, (size_t)nnzP)); PAMG_TRY(d.get(&dPx, (size_t)nnzP)); PAMG_TRY(d.get(&dflag, 1));
    // the rows of P must be the rows pass 1 counted: nothing below writes outside [Pp[i], Pp[i + 1])
    PAMG_HIP(hipMemset(dflag, 0, sizeof(unsigned)));
    hipLaunchKernelGGL(interp_check_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, dSp, dSj, dsp, dPp, dflag);
    PAMG_HIP(hipGetLastError());
    unsigned bad = 0;
    PAMG_HIP(hipMemcpy(&bad, dflag, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (bad) return PAMG_E_ARG;
    int nc = 0;
    PAMG_TRY(scan_counts(n, dsp, dmap, dflag, &nc));        // the coarse number of every C-point
    if (modified < 0) {
        hipLaunchKernelGGL(direct_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, dAp, dAj, dAx, dSp, dSj, dSx, dsp, dPp, dmap, dPj, dPx);
        PAMG_HIP(hipGetLastError());
    } else {
        double *dden;
        PAMG_TRY(d.get(&dden, (size_t)n));
        hipLaunchKernelGGL(classical_prologue_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, dAp, dAx, dSp, dSj, dSx, dsp, dPp, dmap, dPj, dPx, dden);
        PAMG_HIP(hipGetLastError());
        // the F-rows by size class, each class in row order
        std::vector<int> lists[cls::NCLASS];
        for (int i = 0; i < n; ++i) {
            const int ns = a.Sp[i + 1] - a.Sp[i];
            if (a.splitting[i] != cls::C_NODE && ns > 0) lists[cls::size_class(ns)].push_back(i);
        }
        int *drows[cls::NCLASS];
        for (int c = 0; c < cls::NCLASS; ++c) PAMG_TRY(d.put(&drows[c], (const int *)lists[c].data(), lists[c].size()));
        unsigned char *gk = nullptr;
        double *gi = nullptr, *ga = nullptr;
        if (!lists[4].empty()) { PAMG_TRY(d.get(&gk, (size_t)nnzS)); PAMG_TRY(d.get(&gi, (size_t)nnzS)); PAMG_TRY(d.get(&ga, (size_t)nnzS)); }
#define PAMG_CLS_LAUNCH(c, W, STAGED) \
        launch_class<W, STAGED>((int)lists[c].size(), drows[c], dAp, dAj, dAx, dSp, dSj, dSx, dsp, dPp, dmap, dden, dPj, dPx, modified, gk, gi, ga)
        PAMG_CLS_LAUNCH(0, 8, true); PAMG_CLS_LAUNCH(1, 16, true); PAMG_CLS_LAUNCH(2, 32, true); PAMG_CLS_LAUNCH(3, 64, true);
        PAMG_CLS_LAUNCH(4, 64, false);
#undef PAMG_CLS_LAUNCH
        PAMG_HIP(hipGetLastError());
    }
    PAMG_TRY(Bufs::fetch(a.Pj, dPj, (size_t)nnzP));
    PAMG_TRY(Bufs::fetch(a.Px, dPx, (size_t)nnzP));
    if (!nnzP) PAMG_HIP(hipDeviceSynchronize());
    return PAMG_OK;
}

}  // namespace

// declared in pamg_host_call.h: PMIS and the CLJP selection (pamg_cljp.hip) build the same transposed pattern
int pamg::device_transposed_pattern(int n, int64_t nnz, const int *dSp, const int *dSj, int *ddeg, int *dTp, int *dTj, int *dcur, unsigned *dflag)
{
    PAMG_HIP(hipMemset(ddeg, 0, sizeof(int) * (size_t)n));
    PAMG_HIP(hipMemset(dcur, 0, sizeof(int) * (size_t)n));
    hipLaunchKernelGGL(indegree_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, dSp, dSj, ddeg);
    PAMG_HIP(hipGetLastError());
    int tn = 0;
    PAMG_TRY(scan_counts(n, ddeg, dTp, dflag, &tn));
    if (tn > nnz) return PAMG_E_STATE;
    hipLaunchKernelGGL(transpose_fill_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, dSp, dSj, dTp, dcur, dTj);
    PAMG_HIP(hipGetLastError());
    return PAMG_OK;
}

extern "C" {

int pamg_classical_strength_of_connection_abs(int32_t n_row, double theta, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size,
                                              const double *Ax, int Ax_size, int32_t *Sp, int Sp_size, int32_t *Sj, int Sj_size, double *Sx,
                                              int Sx_size)
{ return strength<false>(n_row, theta, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, Sp, Sp_size, Sj, Sj_size, Sx, Sx_size); }

int pamg_classical_strength_of_connection_min(int32_t n_row, double theta, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size,
                                              const double *Ax, int Ax_size, int32_t *Sp, int Sp_size, int32_t *Sj, int Sj_size, double *Sx,
                                              int Sx_size)
{ return strength<true>(n_row, theta, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, Sp, Sp_size, Sj, Sj_size, Sx, Sx_size); }

int pamg_maximal_independent_set(int32_t num_rows, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, int32_t active, int32_t C,
                                 int32_t F, int32_t *x, int x_size, const double *y, int y_size, int32_t max_iters, int32_t *n_mis,
                                 int32_t *rounds)
{
    const int n = num_rows;
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(n, n, Ap, Ap_size, Aj, Aj_size, &nnz));
    if (x_size < n || y_size < n || (n && (!x || !y)) || active == C || active == F) return PAMG_E_ARG;
    if (max_iters != -1) return PAMG_E_UNSUPPORTED;         // a bounded number of the reference's in-place sweeps depends on the sweep order
    if (n_mis) *n_mis = 0;
    if (rounds) *rounds = 0;
    if (n == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dGp, *dGj, *dx[2];
    double *dy;
    unsigned *dflags;
    PAMG_TRY(d.put(&dGp, Ap, (size_t)n + 1)); PAMG_TRY(d.put(&dGj, Aj, (size_t)nnz)); PAMG_TRY(d.put(&dy, y, (size_t)n));
    PAMG_TRY(d.put(&dx[0], (const int *)x, (size_t)n)); PAMG_TRY(d.get(&dx[1], (size_t)n)); PAMG_TRY(d.get(&dflags, MIS_BATCH));
    PAMG_HIP(hipMemset(dflags, 0, sizeof(unsigned)));
    hipLaunchKernelGGL(symmetric_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, dGp, dGj, dflags);
    PAMG_HIP(hipGetLastError());
    unsigned bad = 0;
    PAMG_HIP(hipMemcpy(&bad, dflags, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (bad) return PAMG_E_UNSUPPORTED;                     // the synchronous rounds need a symmetric pattern
    int fin = 0, nr = 0;
    PAMG_TRY(mis_rounds(n, dGp, dGj, nullptr, nullptr, dy, dx, active, C, F, dflags, &fin, &nr));
    std::vector<int> out((size_t)n);
    PAMG_TRY(Bufs::fetch(out.data(), dx[fin], (size_t)n));
    int count = 0;
    for (int i = 0; i < n; ++i) { count += x[i] == active && out[(size_t)i] == C; x[i] = out[(size_t)i]; }
    if (n_mis) *n_mis = count;
    if (rounds) *rounds = nr;
    return PAMG_OK;
}

int pamg_pmis_splitting(int32_t n_nodes, const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size, const double *rnd, int rnd_size,
                        int32_t *splitting, int splitting_size, int32_t *rounds)
{
    const int n = n_nodes;
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(n, n, Sp, Sp_size, Sj, Sj_size, &nnz));
    if (rnd_size < n || splitting_size < n || (n && (!rnd || !splitting))) return PAMG_E_ARG;
    if (rounds) *rounds = 0;
    if (n == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dSp, *dSj, *ddeg, *dTp, *dTj, *dcur, *dx[2];
    double *drnd, *dy;
    unsigned *dflags;
    PAMG_TRY(d.put(&dSp, Sp, (size_t)n + 1)); PAMG_TRY(d.put(&dSj, Sj, (size_t)nnz)); PAMG_TRY(d.put(&drnd, rnd, (size_t)n));
    PAMG_TRY(d.get(&ddeg, (size_t)n)); PAMG_TRY(d.get(&dTp, (size_t)n + 1)); PAMG_TRY(d.get(&dTj, (size_t)nnz)); PAMG_TRY(d.get(&dcur, (size_t)n));
    PAMG_TRY(d.get(&dy, (size_t)n)); PAMG_TRY(d.get(&dx[0], (size_t)n)); PAMG_TRY(d.get(&dx[1], (size_t)n)); PAMG_TRY(d.get(&dflags, MIS_BATCH));
    PAMG_TRY(device_transposed_pattern(n, nnz, dSp, dSj, ddeg, dTp, dTj, dcur, dflags));
    hipLaunchKernelGGL(pmis_init_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, ddeg, drnd, dy, dx[0]);
    PAMG_HIP(hipGetLastError());
    int fin = 0, nr = 0;
    PAMG_TRY(mis_rounds(n, dSp, dSj, dTp, dTj, dy, dx, -1, cls::C_NODE, cls::F_NODE, dflags, &fin, &nr));
    hipLaunchKernelGGL(pmis_dirichlet_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, dSp, dSj, ddeg, dx[fin]);
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(splitting, dx[fin], (size_t)n));
    if (rounds) *rounds = nr;
    return PAMG_OK;
}

int pamg_rs_direct_interpolation_pass1(int32_t n_nodes, const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size, const int32_t *splitting,
                                       int splitting_size, int32_t *Pp, int Pp_size)
{ return interp_pass1(n_nodes, Sp, Sp_size, Sj, Sj_size, splitting, splitting_size, Pp, Pp_size); }

int pamg_rs_classical_interpolation_pass1(int32_t n_nodes, const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size, const int32_t *splitting,
                                          int splitting_size, int32_t *Pp, int Pp_size)
{ return interp_pass1(n_nodes, Sp, Sp_size, Sj, Sj_size, splitting, splitting_size, Pp, Pp_size); }

int pamg_rs_direct_interpolation_pass2(int32_t n_nodes, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const double *Ax, int Ax_size,
                                       const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size, const double *Sx, int Sx_size,
                                       const int32_t *splitting, int splitting_size, const int32_t *Pp, int Pp_size, int32_t *Pj, int Pj_size,
                                       double *Px, int Px_size)
{
    const InterpArgs a = {n_nodes, Ap, Aj, Ax, Ap_size, Aj_size, Ax_size, Sp, Sj, Sx, Sp_size, Sj_size, Sx_size, splitting, splitting_size,
                          Pp, Pp_size, Pj, Pj_size, Px, Px_size};
    return interp_pass2(a, -1);
}

int pamg_rs_classical_interpolation_pass2(int32_t n_nodes, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const double *Ax,
                                          int Ax_size, const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size, const double *Sx, int Sx_size,
                                          const int32_t *splitting, int splitting_size, const int32_t *Pp, int Pp_size, int32_t *Pj, int Pj_size,
                                          double *Px, int Px_size, int modified)
{
    const InterpArgs a = {n_nodes, Ap, Aj, Ax, Ap_size, Aj_size, Ax_size, Sp, Sj, Sx, Sp_size, Sj_size, Sx_size, splitting, splitting_size,
                          Pp, Pp_size, Pj, Pj_size, Px, Px_size};
    return interp_pass2(a, modified ? 1 : 0);
}

int pamg_remove_strong_FF_connections(int32_t n_nodes, const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size, double *Sx, int Sx_size,
                                      const int32_t *splitting, int splitting_size)
{
    const int n = n_nodes;
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(n, n, Sp, Sp_size, Sj, Sj_size, &nnz));
    if (nnz > Sx_size || (nnz && !Sx) || splitting_size < n || (n && !splitting)) return PAMG_E_ARG;
    if (n == 0 || nnz == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dSp, *dSj, *dsp;
    double *dSx;
    PAMG_TRY(d.put(&dSp, Sp, (size_t)n + 1)); PAMG_TRY(d.put(&dSj, Sj, (size_t)nnz)); PAMG_TRY(d.put(&dSx, (const double *)Sx, (size_t)nnz));
    PAMG_TRY(d.put(&dsp, splitting, (size_t)n));
    hipLaunchKernelGGL(remove_ff_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, dSp, dSj, dSx, dsp);
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(Sx, dSx, (size_t)nnz));
    return PAMG_OK;
}

}  // extern "C"
