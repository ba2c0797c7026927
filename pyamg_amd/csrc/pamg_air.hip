// pamg_air.hip -- the setup of approximate ideal restriction (AIR) AMG on the device: one-point interpolation and the local solves of
// approx_ideal_restriction_pass1 / _pass2.  Layer 1 of the C ABI: HOST arrays in, HOST arrays out, amg_core's argument order.  The per-row
// arithmetic is pamg_air.h (replayed on the host by tests/air_emul.cpp); every result is the reference's, bit for bit.
//
//   one point  one lane per row: the strongest C-neighbour (count), the host's scan of the counts, the same routine again (fill)
//   pass 1     one lane per C-row builds the ascending, unique neighbourhood in its own 64-entry slot of LDS.  A neighbourhood beyond 64
//              entries is counted on the host threads by the same routine
//   pass 2     the counts again, held against the caller's Rp (PAMG_E_ARG before anything is written); one lane per C-row writes the
//              neighbourhood and the identity entry; then a group of W = 8 / 16 / 32 / 64 lanes per C-row by its N: lane k gathers and
//              owns column k of the local system and row k of Q, both in LDS (the 64-wide class keeps Q in global scratch: R and Q
//              together are 64 KB at N = 64).  Rows with N > 64 are solved on the host threads by air::solve_serial
//
// A workgroup is ONE wave of 64 lanes holding 64 / W systems: its barriers cost a wait, and every loop around a barrier has bounds that
// depend on the workgroup only (the largest N of its systems).
#include "pamg_common.h"
#include "pamg_air.h"
#include "pamg_host_call.h"
#include "pamg_stream_plan.h"

#include <climits>

using namespace pamg;

namespace {

constexpr int AIR_BLK = 64;                 // one wave
constexpr int SLOT = air::MAX_STAGED + 1;   // ints per lane of the counting kernel (odd: the lanes' slots start on different banks)

int agrid(int64_t n, int per_block, int cap = 8192) { return launch_grid(n, per_block, cap); }

// counts -> pointer on the host; PAMG_E_UNSUPPORTED beyond int32
int scan_host(int n, const int *cnt, int *ptr)
{
    long long run = 0;
    for (int i = 0; i < n; ++i) { ptr[i] = (int)run; run += cnt[i]; }
    if (run > INT_MAX) return PAMG_E_UNSUPPORTED;
    ptr[n] = (int)run;
    return PAMG_OK;
}

// ------------------------------------------------------------------------------------------------ one-point interpolation
template <bool FILL>
__global__ __launch_bounds__(BLK) void one_point_kernel(int n, const int *__restrict__ Cp, const int *__restrict__ Cj, const double *__restrict__ Cx,
                                                        const int *__restrict__ splitting, const int *__restrict__ map, int *__restrict__ cnt,
                                                        const int *__restrict__ Pp, int *__restrict__ Pj, double *__restrict__ Px)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) {
        if (FILL) {
            if (Pp[i + 1] > Pp[i]) air::one_point_row(i, Cp, Cj, Cx, splitting, map, Pj + Pp[i], Px + Pp[i]);
        } else cnt[i] = air::one_point_row(i, Cp, Cj, Cx, splitting, map, nullptr, nullptr);
    }
}

// ------------------------------------------------------------------------------------------------ neighbourhoods
// cnt[row] = N of the C-row, -1 beyond MAX_STAGED
__global__ __launch_bounds__(AIR_BLK) void air_count_kernel(int nc, const int *__restrict__ Cp, const int *__restrict__ Cj, const int *__restrict__ Cpts,
                                                            const int *__restrict__ splitting, int distance, int *__restrict__ cnt)
{
    __shared__ int s_buf[AIR_BLK * SLOT];
    int *buf = s_buf + threadIdx.x * SLOT;
    for (int row = blockIdx.x * AIR_BLK + threadIdx.x; row < nc; row += gridDim.x * AIR_BLK)
        cnt[row] = air::neighbourhood(Cpts[row], Cp, Cj, splitting, distance, buf, air::MAX_STAGED);
}

// the listed C-rows (N <= MAX_STAGED, Rp checked against the counts): the neighbourhood straight into the row of Rj, then the identity
__global__ __launch_bounds__(AIR_BLK) void air_fill_kernel(int nlist, const int *__restrict__ rows, const int *__restrict__ Cp, const int *__restrict__ Cj,
                                                           const int *__restrict__ Cpts, const int *__restrict__ splitting, int distance,
                                                           const int *__restrict__ Rp, int *__restrict__ Rj, double *__restrict__ Rx,
                                                           unsigned *__restrict__ flag)
{
    for (int t = blockIdx.x * AIR_BLK + threadIdx.x; t < nlist; t += gridDim.x * AIR_BLK) {
        const int row = rows[t], r0 = Rp[row], N = Rp[row + 1] - r0 - 1, c = Cpts[row];
        if (air::neighbourhood(c, Cp, Cj, splitting, distance, Rj + r0, N) != N) { atomicOr(flag, 1u); continue; }   // (the check before excludes it)
        Rj[r0 + N] = c;
        Rx[r0 + N] = 1.0;
    }
}

// ------------------------------------------------------------------------------------------------ the local solves
// One group of W lanes per listed C-row, 64 / W rows per workgroup.  Per group in LDS: R [W * (W + 1)], Q the same (QGLOBAL: a
// 64 x 64 slab of gQ per workgroup instead), v, b, rhs [W] and {tau, kept}.
template <int W, bool QGLOBAL>
__global__ __launch_bounds__(AIR_BLK) void air_solve_kernel(int nlist, const int *__restrict__ rows, const int *__restrict__ Ap, const int *__restrict__ Aj,
                                                            const double *__restrict__ Ax, const int *__restrict__ Cpts, const int *__restrict__ Rp,
                                                            const int *__restrict__ Rj, double *__restrict__ Rx, double *__restrict__ gQ)
{
    constexpr int G = AIR_BLK / W, LD = W + 1, LDQ = QGLOBAL ? W : LD;
    __shared__ double s_R[G * W * LD];
    __shared__ double s_Q[QGLOBAL ? 1 : G * W * LD];
    __shared__ double s_v[G * W], s_b[G * W], s_rhs[G * W], s_hdr[G * 2];
    __shared__ int s_nmax;
    const int g = threadIdx.x / W, lane = threadIdx.x % W;
    double *R = s_R + g * W * LD;
    double *Q = QGLOBAL ? gQ + (size_t)blockIdx.x * W * W : s_Q + g * W * LD;
    double *v = s_v + g * W, *b = s_b + g * W, *rhs = s_rhs + g * W, *hdr = s_hdr + g * 2;
    for (int base = blockIdx.x * G; base < nlist; base += gridDim.x * G) {
        const bool live = base + g < nlist;
        const int row = live ? rows[base + g] : 0;
        const int r0 = live ? Rp[row] : 0, N = live ? Rp[row + 1] - r0 - 1 : 0;
        const int *Nf = Rj + r0;
        if (threadIdx.x == 0) s_nmax = 0;
        __syncthreads();
        if (lane == 0) atomicMax(&s_nmax, N);
        __syncthreads();
        const int nmax = s_nmax;
        if (lane < N) {
            air::gather_column(lane, N, Nf, Ap, Aj, Ax, R, LD);
            b[lane] = air::gather_rhs(lane, Nf, Ap, Aj, Ax, Cpts[row]);
            air::q_identity_row(lane, N, Q, LDQ);
        }
        __syncthreads();
        for (int j = 0; j < nmax; ++j) {
            if (lane == j && j < N) {
                double tau = 0.0;
                const bool kept = air::qr_head(j, N, R, LD, v, &tau);
                hdr[0] = tau;
                hdr[1] = kept ? 1.0 : 0.0;
            }
            __syncthreads();
            if (j < N && lane < N && hdr[1] != 0.0) {
                const double tau = hdr[0];
                if (lane >= j) air::qr_col(j, lane, N, R, LD, v, tau);
                air::qr_row(j, lane, N, Q, LDQ, v, tau);
            }
            __syncthreads();
        }
        if (QGLOBAL) __threadfence_block();                 // the rows of Q were written by their own lanes; the columns are read next
        __syncthreads();
        if (lane < N) rhs[lane] = air::rhs_entry(lane, N, b, Q, LDQ);
        __syncthreads();
        if (lane == 0 && N > 0) air::back_substitute(N, R, LD, rhs, Rx + r0);
        __syncthreads();                                    // the LDS slots are restaged by the next row
    }
}

template <int W, bool QGLOBAL>
int launch_solve(Bufs &d, int nlist, const int *rows, const int *Ap, const int *Aj, const double *Ax, const int *Cpts, const int *Rp, const int *Rj,
                 double *Rx)
{
    if (!nlist) return PAMG_OK;
    constexpr int G = AIR_BLK / W;
    const int grid = agrid(nlist, G, QGLOBAL ? 2048 : 8192);
    double *gQ = nullptr;
    if (QGLOBAL) PAMG_TRY(d.get(&gQ, (size_t)grid * W * W));
    hipLaunchKernelGGL((air_solve_kernel<W, QGLOBAL>), dim3(grid), dim3(AIR_BLK), 0, 0, nlist, rows, Ap, Aj, Ax, Cpts, Rp, Rj, Rx, gQ);
    PAMG_HIP(hipGetLastError());
    return PAMG_OK;
}

}  // namespace

// N of every C-row: the device's counts, and the host threads for what did not fit its slots
int pamg::air_neighbourhood_counts(int n, int nc, const int *Cp, const int *Cj, const int *Cpts, const int *splitting, int distance, const int *dCp,
                         const int *dCj, const int *dCpts, const int *dsp, Bufs &d, std::vector<int> &cnt)
{
    cnt.assign((size_t)nc, 0);
    if (nc == 0) return PAMG_OK;
    int *dcnt;
    PAMG_TRY(d.get(&dcnt, (size_t)nc));
    hipLaunchKernelGGL(air_count_kernel, dim3(agrid(nc, AIR_BLK)), dim3(AIR_BLK), 0, 0, nc, dCp, dCj, dCpts, dsp, distance, dcnt);
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(cnt.data(), dcnt, (size_t)nc));
    std::vector<int> big;
    for (int r = 0; r < nc; ++r) if (cnt[(size_t)r] < 0) big.push_back(r);
    plan_parallel((int64_t)big.size(), [&](int64_t lo, int64_t hi, int) {
        std::vector<int> buf((size_t)n + 1);
        for (int64_t t = lo; t < hi; ++t) {
            const int r = big[(size_t)t];
            cnt[(size_t)r] = air::neighbourhood(Cpts[r], Cp, Cj, splitting, distance, buf.data(), n);
        }
    }, 1);
    return PAMG_OK;
}

int pamg::air_check_cf(int n, const int *Cpts, int Cpts_size, const int *splitting, int splitting_size)
{
    if (Cpts_size < 0 || (Cpts_size && !Cpts) || splitting_size < n || (n && !splitting)) return PAMG_E_ARG;
    for (int r = 0; r < Cpts_size; ++r) if (Cpts[r] < 0 || Cpts[r] >= n) return PAMG_E_ARG;
    return PAMG_OK;
}

extern "C" {

int pamg_one_point_interpolation(int32_t *Pp, int Pp_size, int32_t *Pj, int Pj_size, double *Px, int Px_size, const int32_t *Cp, int Cp_size,
                                 const int32_t *Cj, int Cj_size, const double *Cx, int Cx_size, const int32_t *splitting, int splitting_size)
{
    const int n = Pp_size - 1;
    int64_t nnz = 0;
    if (!Pp) return PAMG_E_ARG;
    PAMG_TRY(check_pattern(n, n, Cp, Cp_size, Cj, Cj_size, &nnz));
    if (nnz > Cx_size || (nnz && !Cx) || splitting_size < n || (n && !splitting)) return PAMG_E_ARG;
    Pp[0] = 0;
    if (n == 0) return PAMG_OK;
    std::vector<int> map((size_t)n + 1), cnt((size_t)n);
    PAMG_TRY(scan_host(n, splitting, map.data()));          // the coarse number of every C-point (air.h:58-62)
    PAMG_TRY(have_device());
    Bufs d;
    int *dCp, *dCj, *dsp, *dmap, *dcnt, *dPp, *dPj;
    double *dCx, *dPx;
    PAMG_TRY(d.put(&dCp, Cp, (size_t)n + 1)); PAMG_TRY(d.put(&dCj, Cj, (size_t)nnz)); PAMG_TRY(d.put(&dCx, Cx, (size_t)nnz));
    PAMG_TRY(d.put(&dsp, splitting, (size_t)n)); PAMG_TRY(d.put(&dmap, (const int *)map.data(), (size_t)n + 1)); PAMG_TRY(d.get(&dcnt, (size_t)n));
    const int grid = agrid(n, BLK);
    hipLaunchKernelGGL((one_point_kernel<false>), dim3(grid), dim3(BLK), 0, 0, n, dCp, dCj, dCx, dsp, dmap, dcnt, (const int *)nullptr, (int *)nullptr,
                       (double *)nullptr);
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(cnt.data(), dcnt, (size_t)n));
    std::vector<int> ptr((size_t)n + 1);
    PAMG_TRY(scan_host(n, cnt.data(), ptr.data()));
    const int total = ptr[(size_t)n];
    if (total > Pj_size || total > Px_size || (total && (!Pj || !Px))) return PAMG_E_ARG;
    PAMG_TRY(d.put(&dPp, (const int *)ptr.data(), (size_t)n + 1)); PAMG_TRY(d.get(&dPj, (size_t)total)); PAMG_TRY(d.get(&dPx, (size_t)total));
    hipLaunchKernelGGL((one_point_kernel<true>), dim3(grid), dim3(BLK), 0, 0, n, dCp, dCj, dCx, dsp, dmap, (int *)nullptr, (const int *)dPp, dPj, dPx);
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(Pj, dPj, (size_t)total));
    PAMG_TRY(Bufs::fetch(Px, dPx, (size_t)total));
    if (!total) PAMG_HIP(hipDeviceSynchronize());
    for (int i = 0; i <= n; ++i) Pp[i] = ptr[(size_t)i];
    return PAMG_OK;
}

int pamg_approx_ideal_restriction_pass1(int32_t *Rp, int Rp_size, const int32_t *Cp, int Cp_size, const int32_t *Cj, int Cj_size,
                                        const int32_t *Cpts, int Cpts_size, const int32_t *splitting, int splitting_size, int32_t distance)
{
    const int n = Cp_size - 1, nc = Cpts_size;
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(n, n, Cp, Cp_size, Cj, Cj_size, &nnz));
    PAMG_TRY(air_check_cf(n, Cpts, Cpts_size, splitting, splitting_size));
    if (!Rp || Rp_size < nc + 1) return PAMG_E_ARG;
    Rp[0] = 0;
    if (nc == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dCp, *dCj, *dCpts, *dsp;
    PAMG_TRY(d.put(&dCp, Cp, (size_t)n + 1)); PAMG_TRY(d.put(&dCj, Cj, (size_t)nnz)); PAMG_TRY(d.put(&dCpts, Cpts, (size_t)nc));
    PAMG_TRY(d.put(&dsp, splitting, (size_t)n));
    std::vector<int> cnt;
    PAMG_TRY(air_neighbourhood_counts(n, nc, Cp, Cj, Cpts, splitting, distance, dCp, dCj, dCpts, dsp, d, cnt));
    for (int &c : cnt) c += 1;                              // the identity entry
    return scan_host(nc, cnt.data(), Rp);
}

int pamg_approx_ideal_restriction_pass2(const int32_t *Rp, int Rp_size, int32_t *Rj, int Rj_size, double *Rx, int Rx_size, const int32_t *Ap,
                                        int Ap_size, const int32_t *Aj, int Aj_size, const double *Ax, int Ax_size, const int32_t *Cp, int Cp_size,
                                        const int32_t *Cj, int Cj_size, const double *Cx, int Cx_size, const int32_t *Cpts, int Cpts_size,
                                        const int32_t *splitting, int splitting_size, int32_t distance, int32_t use_gmres, int32_t maxiter,
                                        int32_t precondition)
{
    (void)Cx; (void)Cx_size; (void)maxiter; (void)precondition;     // the reference reads the pattern of C only; the rest is GMRES's
    if (use_gmres != 0) return PAMG_E_UNSUPPORTED;
    const int n = Ap_size - 1, nc = Cpts_size;
    int64_t nnzA = 0, nnzC = 0;
    PAMG_TRY(check_pattern(n, n, Ap, Ap_size, Aj, Aj_size, &nnzA));
    PAMG_TRY(check_pattern(n, n, Cp, Cp_size, Cj, Cj_size, &nnzC));
    PAMG_TRY(air_check_cf(n, Cpts, Cpts_size, splitting, splitting_size));
    if (nnzA > Ax_size || (nnzA && !Ax) || !Rp || Rp_size < nc + 1 || Rp[0] != 0) return PAMG_E_ARG;
    if (nc == 0) return PAMG_OK;
    const int nnzR = Rp[nc];
    if (nnzR < 0 || nnzR > Rj_size || nnzR > Rx_size || (nnzR && (!Rj || !Rx))) return PAMG_E_ARG;
    PAMG_TRY(have_device());
    Bufs d;
    int *dAp, *dAj, *dCp, *dCj, *dCpts, *dsp, *dRp, *dRj;
    double *dAx, *dRx;
    unsigned *dflag;
    PAMG_TRY(d.put(&dCp, Cp, (size_t)n + 1)); PAMG_TRY(d.put(&dCj, Cj, (size_t)nnzC)); PAMG_TRY(d.put(&dCpts, Cpts, (size_t)nc));
    PAMG_TRY(d.put(&dsp, splitting, (size_t)n));
    // the rows of R must be the rows pass 1 counted: nothing below writes outside [Rp[row], Rp[row + 1])
    std::vector<int> cnt;
    PAMG_TRY(air_neighbourhood_counts(n, nc, Cp, Cj, Cpts, splitting, distance, dCp, dCj, dCpts, dsp, d, cnt));
    for (int r = 0; r < nc; ++r) if (Rp[r + 1] - Rp[r] != cnt[(size_t)r] + 1) return PAMG_E_ARG;
    PAMG_TRY(d.put(&dAp, Ap, (size_t)n + 1)); PAMG_TRY(d.put(&dAj, Aj, (size_t)nnzA)); PAMG_TRY(d.put(&dAx, Ax, (size_t)nnzA));
    PAMG_TRY(d.put(&dRp, Rp, (size_t)nc + 1)); PAMG_TRY(d.get(&dRj, (size_t)nnzR)); PAMG_TRY(d.get(&dRx, (size_t)nnzR)); PAMG_TRY(d.get(&dflag, 1));
    PAMG_HIP(hipMemset(dRj, 0, sizeof(int) * (size_t)nnzR));
    PAMG_HIP(hipMemset(dRx, 0, sizeof(double) * (size_t)nnzR));     // air.h:208: Rx starts as zero
    PAMG_HIP(hipMemset(dflag, 0, sizeof(unsigned)));
    // the C-rows by size class, each class in row order; class 4 stays on the host
    std::vector<int> lists[air::NCLASS], staged;
    for (int r = 0; r < nc; ++r) {
        const int N = cnt[(size_t)r];
        if (N <= air::MAX_STAGED) staged.push_back(r);
        if (N > 0) lists[air::size_class(N)].push_back(r);
    }
    int *dstaged, *drows[4];
    PAMG_TRY(d.put(&dstaged, (const int *)staged.data(), staged.size()));
    for (int c = 0; c < 4; ++c) PAMG_TRY(d.put(&drows[c], (const int *)lists[c].data(), lists[c].size()));
    if (!staged.empty()) {
        hipLaunchKernelGGL(air_fill_kernel, dim3(agrid((int64_t)staged.size(), AIR_BLK)), dim3(AIR_BLK), 0, 0, (int)staged.size(), dstaged, dCp, dCj, dCpts,
                           dsp, distance, dRp, dRj, dRx, dflag);
        PAMG_HIP(hipGetLastError());
    }
    PAMG_TRY((launch_solve<8, false>(d, (int)lists[0].size(), drows[0], dAp, dAj, dAx, dCpts, dRp, dRj, dRx)));
    PAMG_TRY((launch_solve<16, false>(d, (int)lists[1].size(), drows[1], dAp, dAj, dAx, dCpts, dRp, dRj, dRx)));
    PAMG_TRY((launch_solve<32, false>(d, (int)lists[2].size(), drows[2], dAp, dAj, dAx, dCpts, dRp, dRj, dRx)));
    PAMG_TRY((launch_solve<64, true>(d, (int)lists[3].size(), drows[3], dAp, dAj, dAx, dCpts, dRp, dRj, dRx)));
    // the rows beyond the cap on the host threads while the device works, into buffers of their own
    const std::vector<int> &big = lists[4];
    std::vector<std::vector<int>> bigNf(big.size());
    std::vector<std::vector<double>> bigx(big.size());
    plan_parallel((int64_t)big.size(), [&](int64_t lo, int64_t hi, int) {
        for (int64_t t = lo; t < hi; ++t) {
            const int r = big[(size_t)t], N = cnt[(size_t)r];
            std::vector<int> &Nf = bigNf[(size_t)t];
            std::vector<double> &x = bigx[(size_t)t];
            Nf.resize((size_t)N); x.resize((size_t)N);
            air::neighbourhood(Cpts[r], Cp, Cj, splitting, distance, Nf.data(), N);
            std::vector<double> R((size_t)N * N), Q((size_t)N * N), w((size_t)3 * N);
            air::solve_serial(N, Nf.data(), Cpts[r], Ap, Aj, Ax, R.data(), N, Q.data(), N, w.data(), w.data() + N, w.data() + 2 * N, x.data());
        }
    }, 1);
    unsigned bad = 0;
    PAMG_HIP(hipMemcpy(&bad, dflag, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (bad) return PAMG_E_STATE;
    PAMG_TRY(Bufs::fetch(Rj, dRj, (size_t)nnzR));
    PAMG_TRY(Bufs::fetch(Rx, dRx, (size_t)nnzR));
    for (size_t t = 0; t < big.size(); ++t) {
        const int r = big[t], N = cnt[(size_t)r], r0 = Rp[r];
        for (int i = 0; i < N; ++i) { Rj[r0 + i] = bigNf[t][(size_t)i]; Rx[r0 + i] = bigx[t][(size_t)i]; }
        Rj[r0 + N] = Cpts[r];
        Rx[r0 + N] = 1.0;
    }
    return PAMG_OK;
}

}  // extern "C"
