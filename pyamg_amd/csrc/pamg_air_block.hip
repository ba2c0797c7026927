// pamg_air_block.hip -- the BLOCK (BSR) setup of approximate ideal restriction AMG on the device: the block strength measure and the local
// solves of block_approx_ideal_restriction_pass2.  Layer 1 of the C ABI: HOST arrays in, HOST arrays out, amg_core's argument order.  The
// per-row arithmetic is pamg_air_block.h over pamg_air.h (replayed on the host by tests/block_air_emul.cpp); every result is the
// reference's, bit for bit.  Pass 1 and the one-point interpolation are the scalar entry points of pamg_air.hip on the block pattern.
//
//   measure    one lane per stored block
//   pass 2     the neighbourhood counts of pamg_air.hip, held against the caller's Rp (PAMG_E_ARG before anything is written); one lane per
//              C-row writes the neighbourhood, the identity column and the identity block; then a group of W = 8 / 16 / 32 / 64 lanes per
//              C-row by the order n = N * b of its system: lane k gathers and owns column k of the system and row k of Q and gathers
//              entry k of the b right-hand sides; ONE Householder QR; Q^T b for the b right-hand sides by the lanes, the b back
//              substitutions by b lanes, the blocks of R by the lanes again.  R, Q and the right-hand sides live in LDS (the 64-wide class
//              keeps Q in global scratch, as the scalar kernel does).  Systems with n > 64, and neighbourhoods above the staging cap, are
//              solved on the host threads by air_block::solve_serial
//
// A workgroup is ONE wave of 64 lanes holding 64 / W systems; every loop around a barrier has bounds that depend on the workgroup only.
#include "pamg_common.h"
#include "pamg_air_block.h"
#include "pamg_host_call.h"
#include "pamg_stream_plan.h"

using namespace pamg;

namespace {

constexpr int AIR_BLK = 64;                 // one wave
constexpr int MAX_B = air_block::MAX_B;

int bgrid(int64_t n, int per_block, int cap = 8192) { return launch_grid(n, per_block, cap); }

__global__ __launch_bounds__(BLK) void block_measure_kernel(int nblk, int b, int norm, const double *__restrict__ Ax, double *__restrict__ out)
{
    for (int p = blockIdx.x * BLK + threadIdx.x; p < nblk; p += gridDim.x * BLK) out[p] = air_block::measure(norm, b, Ax + (size_t)p * b * b);
}

// the listed C-rows (N <= MAX_STAGED, Rp checked against the counts): the neighbourhood straight into the row of Rj, then the identity
__global__ __launch_bounds__(AIR_BLK) void block_fill_kernel(int nlist, const int *__restrict__ rows, const int *__restrict__ Cp, const int *__restrict__ Cj,
                                                             const int *__restrict__ Cpts, const int *__restrict__ splitting, int distance, int b,
                                                             const int *__restrict__ Rp, int *__restrict__ Rj, double *__restrict__ Rx,
                                                             unsigned *__restrict__ flag)
{
    for (int t = blockIdx.x * AIR_BLK + threadIdx.x; t < nlist; t += gridDim.x * AIR_BLK) {
        const int row = rows[t], r0 = Rp[row], N = Rp[row + 1] - r0 - 1, c = Cpts[row];
        if (air::neighbourhood(c, Cp, Cj, splitting, distance, Rj + r0, N) != N) { atomicOr(flag, 1u); continue; }   // (the check before excludes it)
        Rj[r0 + N] = c;
        air_block::identity_block(b, Rx + (size_t)(r0 + N) * b * b);
    }
}

// One group of W lanes per listed C-row (n = N * b <= W), 64 / W rows per workgroup.  Per group in LDS: R [W * (W + 1)], Q the same
// (QGLOBAL: a 64 x 64 slab of gQ per workgroup instead), v [W], the right-hand sides and Q^T b [MAX_B * W] each, and {tau, kept}.
template <int W, bool QGLOBAL>
__global__ __launch_bounds__(AIR_BLK) void block_solve_kernel(int nlist, const int *__restrict__ rows, int b, const int *__restrict__ Ap,
                                                              const int *__restrict__ Aj, const double *__restrict__ Ax, const int *__restrict__ Cpts,
                                                              const int *__restrict__ Rp, const int *__restrict__ Rj, double *__restrict__ Rx,
                                                              double *__restrict__ gQ)
{
    constexpr int G = AIR_BLK / W, LD = W + 1, LDQ = QGLOBAL ? W : LD;
    __shared__ double s_R[G * W * LD];
    __shared__ double s_Q[QGLOBAL ? 1 : G * W * LD];
    __shared__ double s_v[G * W], s_b[G * W * MAX_B], s_rhs[G * W * MAX_B], s_hdr[G * 2];
    __shared__ int s_nmax;
    const int g = threadIdx.x / W, lane = threadIdx.x % W;
    double *R = s_R + g * W * LD;
    double *Q = QGLOBAL ? gQ + (size_t)blockIdx.x * W * W : s_Q + g * W * LD;
    double *v = s_v + g * W, *b0 = s_b + g * W * MAX_B, *rhs = s_rhs + g * W * MAX_B, *hdr = s_hdr + g * 2;
    for (int base = blockIdx.x * G; base < nlist; base += gridDim.x * G) {
        const bool live = base + g < nlist;
        const int row = live ? rows[base + g] : 0;
        const int r0 = live ? Rp[row] : 0, N = live ? Rp[row + 1] - r0 - 1 : 0, n = N * b;
        const int *Nf = Rj + r0;
        if (threadIdx.x == 0) s_nmax = 0;
        __syncthreads();
        if (lane == 0) atomicMax(&s_nmax, n);
        __syncthreads();
        const int nmax = s_nmax;
        if (lane < n) {
            air_block::gather_column(lane, N, b, Nf, Ap, Aj, Ax, R, LD);
            air_block::gather_rhs(lane, n, b, Nf, Ap, Aj, Ax, Cpts[row], b0);
            air::q_identity_row(lane, n, Q, LDQ);
        }
        __syncthreads();
        for (int j = 0; j < nmax; ++j) {
            if (lane == j && j < n) {
                double tau = 0.0;
                const bool kept = air::qr_head(j, n, R, LD, v, &tau);
                hdr[0] = tau;
                hdr[1] = kept ? 1.0 : 0.0;
            }
            __syncthreads();
            if (j < n && lane < n && hdr[1] != 0.0) {
                const double tau = hdr[0];
                if (lane >= j) air::qr_col(j, lane, n, R, LD, v, tau);
                air::qr_row(j, lane, n, Q, LDQ, v, tau);
            }
            __syncthreads();
        }
        if (QGLOBAL) __threadfence_block();                 // the rows of Q were written by their own lanes; the columns are read next
        __syncthreads();
        if (lane < n)
            for (int r = 0; r < b; ++r) rhs[r * n + lane] = air::rhs_entry(lane, n, b0 + r * n, Q, LDQ);
        __syncthreads();
        if (n > 0 && lane < b) air::back_substitute(n, R, LD, rhs + lane * n, b0 + lane * n);       // the solution replaces its right-hand side
        __syncthreads();
        if (lane < n) air_block::store_solution(lane, n, b, b0, Rx + (size_t)r0 * b * b);
        __syncthreads();                                    // the LDS slots are restaged by the next row
    }
}

template <int W, bool QGLOBAL>
int launch_solve(Bufs &d, int nlist, const int *rows, int b, const int *Ap, const int *Aj, const double *Ax, const int *Cpts, const int *Rp, const int *Rj,
                 double *Rx)
{
    if (!nlist) return PAMG_OK;
    constexpr int G = AIR_BLK / W;
    const int grid = bgrid(nlist, G, QGLOBAL ? 2048 : 8192);
    double *gQ = nullptr;
    if (QGLOBAL) PAMG_TRY(d.get(&gQ, (size_t)grid * W * W));
    hipLaunchKernelGGL((block_solve_kernel<W, QGLOBAL>), dim3(grid), dim3(AIR_BLK), 0, 0, nlist, rows, b, Ap, Aj, Ax, Cpts, Rp, Rj, Rx, gQ);
    PAMG_HIP(hipGetLastError());
    return PAMG_OK;
}

}  // namespace

extern "C" {

int pamg_block_strength_measure(int32_t n_blocks, int32_t blocksize, int32_t norm, const double *Ax, int Ax_size, double *out, int out_size)
{
    const int b = blocksize;
    if (n_blocks < 0 || b < 1 || norm < air_block::NORM_ABS || norm > air_block::NORM_FRO) return PAMG_E_ARG;
    if (b > MAX_B || (norm == air_block::NORM_FRO && b == MAX_B)) return PAMG_E_UNSUPPORTED;      // (NumPy's eight-accumulator sum: the header)
    if ((int64_t)n_blocks * b * b > Ax_size || n_blocks > out_size || (n_blocks && (!Ax || !out))) return PAMG_E_ARG;
    if (n_blocks == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    double *dAx, *dout;
    PAMG_TRY(d.put(&dAx, Ax, (size_t)n_blocks * b * b)); PAMG_TRY(d.get(&dout, (size_t)n_blocks));
    hipLaunchKernelGGL(block_measure_kernel, dim3(bgrid(n_blocks, BLK)), dim3(BLK), 0, 0, n_blocks, b, norm, dAx, dout);
    PAMG_HIP(hipGetLastError());
    return Bufs::fetch(out, dout, (size_t)n_blocks);
}

int pamg_block_approx_ideal_restriction_pass2(const int32_t *Rp, int Rp_size, int32_t *Rj, int Rj_size, double *Rx, int Rx_size, const int32_t *Ap,
                                              int Ap_size, const int32_t *Aj, int Aj_size, const double *Ax, int Ax_size, const int32_t *Cp,
                                              int Cp_size, const int32_t *Cj, int Cj_size, const double *Cx, int Cx_size, const int32_t *Cpts,
                                              int Cpts_size, const int32_t *splitting, int splitting_size, int32_t blocksize, int32_t distance,
                                              int32_t use_gmres, int32_t maxiter, int32_t precondition)
{
    (void)Cx; (void)Cx_size; (void)maxiter; (void)precondition;     // the reference reads the pattern of C only; the rest is GMRES's
    if (use_gmres != 0) return PAMG_E_UNSUPPORTED;
    const int b = blocksize;
    if (b < 1) return PAMG_E_ARG;
    if (b > MAX_B) return PAMG_E_UNSUPPORTED;
    const int bb = b * b, n = Ap_size - 1, nc = Cpts_size;
    int64_t nnzA = 0, nnzC = 0;
    PAMG_TRY(check_pattern(n, n, Ap, Ap_size, Aj, Aj_size, &nnzA));
    PAMG_TRY(check_pattern(n, n, Cp, Cp_size, Cj, Cj_size, &nnzC));
    PAMG_TRY(air_check_cf(n, Cpts, Cpts_size, splitting, splitting_size));
    if (nnzA * bb > Ax_size || (nnzA && !Ax) || !Rp || Rp_size < nc + 1 || Rp[0] != 0) return PAMG_E_ARG;
    if (nc == 0) return PAMG_OK;
    const int nnzR = Rp[nc];
    if (nnzR < 0 || nnzR > Rj_size || (int64_t)nnzR * bb > Rx_size || (nnzR && (!Rj || !Rx))) return PAMG_E_ARG;
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
    const size_t nRx = (size_t)nnzR * bb;
    PAMG_TRY(d.put(&dAp, Ap, (size_t)n + 1)); PAMG_TRY(d.put(&dAj, Aj, (size_t)nnzA)); PAMG_TRY(d.put(&dAx, Ax, (size_t)nnzA * bb));
    PAMG_TRY(d.put(&dRp, Rp, (size_t)nc + 1)); PAMG_TRY(d.get(&dRj, (size_t)nnzR)); PAMG_TRY(d.get(&dRx, nRx)); PAMG_TRY(d.get(&dflag, 1));
    PAMG_HIP(hipMemset(dRj, 0, sizeof(int) * (size_t)nnzR));
    PAMG_HIP(hipMemset(dRx, 0, sizeof(double) * nRx));      // air.h:375: Rx starts as zero
    PAMG_HIP(hipMemset(dflag, 0, sizeof(unsigned)));
    // the C-rows by the size class of n = N * b, each class in row order; class 4 stays on the host
    std::vector<int> lists[air::NCLASS], staged;
    for (int r = 0; r < nc; ++r) {
        const int N = cnt[(size_t)r];
        if (N <= air::MAX_STAGED) staged.push_back(r);
        if (N > 0) lists[N > air::MAX_STAGED ? 4 : air::size_class(N * b)].push_back(r);
    }
    int *dstaged, *drows[4];
    PAMG_TRY(d.put(&dstaged, (const int *)staged.data(), staged.size()));
    for (int c = 0; c < 4; ++c) PAMG_TRY(d.put(&drows[c], (const int *)lists[c].data(), lists[c].size()));
    if (!staged.empty()) {
        hipLaunchKernelGGL(block_fill_kernel, dim3(bgrid((int64_t)staged.size(), AIR_BLK)), dim3(AIR_BLK), 0, 0, (int)staged.size(), dstaged, dCp, dCj, dCpts,
                           dsp, distance, b, dRp, dRj, dRx, dflag);
        PAMG_HIP(hipGetLastError());
    }
    PAMG_TRY((launch_solve<8, false>(d, (int)lists[0].size(), drows[0], b, dAp, dAj, dAx, dCpts, dRp, dRj, dRx)));
    PAMG_TRY((launch_solve<16, false>(d, (int)lists[1].size(), drows[1], b, dAp, dAj, dAx, dCpts, dRp, dRj, dRx)));
    PAMG_TRY((launch_solve<32, false>(d, (int)lists[2].size(), drows[2], b, dAp, dAj, dAx, dCpts, dRp, dRj, dRx)));
    PAMG_TRY((launch_solve<64, true>(d, (int)lists[3].size(), drows[3], b, dAp, dAj, dAx, dCpts, dRp, dRj, dRx)));
    // the systems beyond the cap on the host threads while the device works, into buffers of their own
    const std::vector<int> &big = lists[4];
    std::vector<std::vector<int>> bigNf(big.size());
    std::vector<std::vector<double>> bigx(big.size());
    plan_parallel((int64_t)big.size(), [&](int64_t lo, int64_t hi, int) {
        for (int64_t t = lo; t < hi; ++t) {
            const int r = big[(size_t)t], N = cnt[(size_t)r];
            const size_t m = (size_t)N * b;
            std::vector<int> &Nf = bigNf[(size_t)t];
            std::vector<double> &x = bigx[(size_t)t];
            Nf.resize((size_t)N); x.resize((size_t)N * bb);
            air::neighbourhood(Cpts[r], Cp, Cj, splitting, distance, Nf.data(), N);
            std::vector<double> R(m * m), Q(m * m), w(2 * m + (size_t)b * m);
            air_block::solve_serial(N, b, Nf.data(), Cpts[r], Ap, Aj, Ax, R.data(), (int)m, Q.data(), (int)m, w.data(), w.data() + 2 * m, w.data() + m,
                                    x.data());
        }
    }, 1);
    unsigned bad = 0;
    PAMG_HIP(hipMemcpy(&bad, dflag, sizeof(unsigned), hipMemcpyDeviceToHost));
    if (bad) return PAMG_E_STATE;
    PAMG_TRY(Bufs::fetch(Rj, dRj, (size_t)nnzR));
    PAMG_TRY(Bufs::fetch(Rx, dRx, nRx));
    for (size_t t = 0; t < big.size(); ++t) {
        const int r = big[t], N = cnt[(size_t)r], r0 = Rp[r];
        for (int i = 0; i < N; ++i) Rj[r0 + i] = bigNf[t][(size_t)i];
        for (size_t e = 0; e < (size_t)N * bb; ++e) Rx[(size_t)r0 * bb + e] = bigx[t][e];
        Rj[r0 + N] = Cpts[r];
        air_block::identity_block(b, Rx + (size_t)(r0 + N) * bb);
    }
    return PAMG_OK;
}

}  // extern "C"
