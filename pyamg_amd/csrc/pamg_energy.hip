// pamg_energy.hip -- energy-minimisation prolongation smoothing with CG and GMRES (aggregation/smooth.py:17-58, :275-442, :648-872) on the
// device.  The arithmetic is pamg_energy.h, replayed on the host by tests/energy_emul.cpp and tests/energy_gmres_emul.cpp.
//
// Layer 1 (HOST arrays in and out, amg_core's argument order): incomplete_mat_mult_bsr, satisfy_constraints_helper, and
// satisfy_constraints with its U @ B on the device as well.  All three are the reference's bit for bit.
// Layer 2: pamg_energy_cg_f64 and pamg_energy_gmres_f64, the whole Krylov loop resident -- one upload, one download of T.
//
// Mapping: a group of GW = 8 / 16 / 32 / 64 lanes per block row of the pattern, GW chosen per call from the mean number of stored
// elements per row; a lane owns the elements lane, lane + GW, ... of the row, so a row of any length is taken by the same group (it
// loops) and nothing goes to the host.  An element of A B is one serial chain -- A's stored row, within it the operand's stored row,
// within a block cc ascending -- so a lane walks the operand's rows itself and keeps the contributions whose column is its own: the
// column indices it compares are the same address for the whole group (one request), only the matching lanes load values, and there
// is no table of n_bcol pointers.  Phases that need the whole row (U @ B after the product, the projection after U @ B, the row's
// partial sum after the projection) are separated by workgroup barriers; every workgroup makes the same number of passes, so the
// barriers are uniform.  The r x K row of U @ B lives in LDS.
//
// Per CG iteration four steps (six launches, each reduction being two): reduce <R, Dinv R> -> newsum, beta and the stop flag (the only
// value read back); direction: P = Dinv R + beta P_old formed where it is read, AP = A P on the pattern, projected, the row's partial
// of <P, AP>; reduce -> alpha; update: T, C-point rows, R, and the row's partial of the next <R, Dinv R>.  P is double-buffered because
// a row reads its neighbours' old direction while it writes its own new one.  The two sums use the fixed tree of pamg_energy.h (no
// floating-point atomics), so a result depends on the operands alone, not on GW or the grid.
//
// GMRES (pamg_energy_gmres_f64, smooth.py:648-872; replayed by tests/energy_gmres_emul.cpp): the Krylov basis V_0 .. V_maxiter is one
// buffer of maxiter + 1 arrays on the pattern's structure.  gmres_product_kernel owns a block row as cg_direction_kernel does: it gathers
// V_i through A's column indices, scales the row by Dinv, projects, and leaves the row's partial of <V_0, W>.  Then i + 1 times
// gmres_mgs_kernel: W -= h V_j with h = H[j, i] from the reduction before it, fused with the row's partial of the next inner product
// (<V_{j+1}, W>, at last <W, W>).  Each reduction ends in gmres_step_kernel, where one lane runs the header's step function: it keeps the
// coefficient, or finishes the column (H[i+1, i], the earlier rotations, the new one, g, normr, the stop flag -- the one int read back).
// gmres_scale_kernel normalises W into V_{i+1}; after the loop H and g come back once, the host solves the triangular system, y goes
// up and gmres_combine_kernel forms T and resets the C-point rows.  3 i + 7 launches in iteration i (a reduction is two).
//
// Plain launches only; no lane of any kernel waits for another outside a workgroup barrier.
#include "pamg_common.h"
#include "pamg_energy.h"
#include "pamg_host_call.h"

using namespace pamg;

namespace {

constexpr int MAXQ = energy::MAX_BLOCK * energy::MAX_NULLDIM;           // entries of a row of U @ B

// device-side scalars of the driver
struct CgScalars {
    double newsum, oldsum, beta, alpha;
    int stop, nsums;
};

struct RowMap {                                              // what every row kernel needs of the pattern and the block shapes
    int n, r, c, K;
    const int *Sp, *Sj;
};

// ------------------------------------------------------------------------------------------------ kernels
// every row kernel: workgroup-uniform passes over BLK / GW rows each; `live` guards the work, never a barrier
#define PAMG_EN_FOR_ROWS(GW) \
    for (int64_t base = (int64_t)blockIdx.x * (BLK / GW); base < M.n; base += (int64_t)gridDim.x * (BLK / GW))
#define PAMG_EN_ROW(GW)                                        \
    const int lane = threadIdx.x % GW, grp = threadIdx.x / GW; \
    const bool live = base + grp < M.n;                        \
    const int row = live ? (int)(base + grp) : 0

template <int GW>
__global__ __launch_bounds__(BLK) void imm_kernel(RowMap M, const int *__restrict__ Ap, const int *__restrict__ Aj, const double *__restrict__ Ax,
                                                  const int *__restrict__ Bp, const int *__restrict__ Bj, const double *__restrict__ Bx, int m,
                                                  double *Sx)
{
    PAMG_EN_FOR_ROWS(GW) {
        PAMG_EN_ROW(GW);
        if (live) energy::imm_lane(lane, GW, row, Ap, Aj, Ax, Bp, Bj, energy::StoredBlocks{Bx, m, M.c}, M.Sp, M.Sj, Sx, Sx, false, M.r, m, M.c);
    }
}

// UB given (satisfy_constraints_helper) or, UBin == nullptr, formed here first (satisfy_constraints)
template <int GW>
__global__ __launch_bounds__(BLK) void constraints_kernel(RowMap M, const double *__restrict__ Bc, const double *__restrict__ UBin,
                                                          const double *__restrict__ BtBinv, double *Sx)
{
    __shared__ double ub_s[(BLK / GW) * MAXQ];
    PAMG_EN_FOR_ROWS(GW) {
        PAMG_EN_ROW(GW);
        double *ub = ub_s + grp * MAXQ;
        if (live) {
            if (UBin) for (int q = lane; q < M.r * M.K; q += GW) ub[q] = UBin[(int64_t)row * M.r * M.K + q];
            else energy::ub_lane(lane, GW, row, M.Sp, M.Sj, Sx, Bc, ub, M.r, M.c, M.K);
        }
        __syncthreads();
        if (live) energy::project_lane(lane, GW, row, M.Sp, M.Sj, Sx, ub, BtBinv, Bc, M.r, M.c, M.K);
        __syncthreads();
    }
}

// R = -(A T) on the pattern, projected; the row's partial of <R, Dinv R>
template <int GW>
__global__ __launch_bounds__(BLK) void cg_init_kernel(RowMap M, const int *__restrict__ Ap, const int *__restrict__ Aj, const double *__restrict__ Ax,
                                                      const double *__restrict__ T, const double *__restrict__ Bc, const double *__restrict__ BtBinv,
                                                      const double *__restrict__ Dinv, double *R, double *rowsum, int *rownzb)
{
    __shared__ double ub_s[(BLK / GW) * MAXQ];
    PAMG_EN_FOR_ROWS(GW) {
        PAMG_EN_ROW(GW);
        double *ub = ub_s + grp * MAXQ;
        if (live) energy::imm_lane(lane, GW, row, Ap, Aj, Ax, M.Sp, M.Sj, energy::StoredBlocks{T, M.r, M.c}, M.Sp, M.Sj, nullptr, R, true, M.r, M.r, M.c);
        __syncthreads();
        if (live) energy::ub_lane(lane, GW, row, M.Sp, M.Sj, R, Bc, ub, M.r, M.c, M.K);
        __syncthreads();
        if (live) energy::project_lane(lane, GW, row, M.Sp, M.Sj, R, ub, BtBinv, Bc, M.r, M.c, M.K);
        __syncthreads();
        if (live && lane == 0) rowsum[row] = energy::row_rz(R, Dinv, row, M.Sp[row], M.Sp[row + 1], M.r, M.c, rownzb + row);
    }
}

template <int GW>
__global__ __launch_bounds__(BLK) void cg_direction_kernel(RowMap M, const int *__restrict__ Ap, const int *__restrict__ Aj,
                                                           const double *__restrict__ Ax, const double *__restrict__ R,
                                                           const double *__restrict__ Pold, double *Pnew, double *AP,
                                                           const double *__restrict__ Bc, const double *__restrict__ BtBinv,
                                                           const double *__restrict__ Dinv, const CgScalars *sc, int first, double *rowsum)
{
    __shared__ double ub_s[(BLK / GW) * MAXQ];
    const energy::Direction dir{R, Pold, Dinv, &sc->beta, M.r, M.c, first};
    PAMG_EN_FOR_ROWS(GW) {
        PAMG_EN_ROW(GW);
        double *ub = ub_s + grp * MAXQ;
        if (live) {
            energy::pnew_lane(lane, GW, row, M.Sp, dir, Pnew, M.r, M.c);
            energy::imm_lane(lane, GW, row, Ap, Aj, Ax, M.Sp, M.Sj, dir, M.Sp, M.Sj, nullptr, AP, false, M.r, M.r, M.c);
        }
        __syncthreads();
        if (live) energy::ub_lane(lane, GW, row, M.Sp, M.Sj, AP, Bc, ub, M.r, M.c, M.K);
        __syncthreads();
        if (live) energy::project_lane(lane, GW, row, M.Sp, M.Sj, AP, ub, BtBinv, Bc, M.r, M.c, M.K);
        __syncthreads();
        if (live && lane == 0) rowsum[row] = energy::row_dot(Pnew, AP, (int64_t)M.Sp[row] * M.r * M.c, (int64_t)M.Sp[row + 1] * M.r * M.c);
    }
}

template <int GW>
__global__ __launch_bounds__(BLK) void cg_update_kernel(RowMap M, double *T, double *R, const double *__restrict__ P, const double *__restrict__ AP,
                                                        const CgScalars *sc, const unsigned char *__restrict__ cmask, const double *__restrict__ PI,
                                                        const double *__restrict__ Dinv, double *rowsum, int *rownzb)
{
    const double alpha = sc->alpha;
    PAMG_EN_FOR_ROWS(GW) {
        PAMG_EN_ROW(GW);
        if (live) energy::update_lane(lane, GW, row, M.Sp, T, R, P, AP, alpha, cmask, PI, M.r, M.c);
        __syncthreads();
        if (live && lane == 0) rowsum[row] = energy::row_rz(R, Dinv, row, M.Sp[row], M.Sp[row + 1], M.r, M.c, rownzb + row);
    }
}

// the halving fold of pamg_energy.h's tree_fold, one lane per value; the counts ride along (integers: any order)
__device__ double fold(double v, long long *cnt)
{
    __shared__ double vs[energy::RED_LANES];
    __shared__ long long cs[energy::RED_LANES];
    const int t = threadIdx.x;
    vs[t] = v;
    cs[t] = *cnt;
    __syncthreads();
    for (int s = energy::RED_LANES / 2; s > 0; s >>= 1) {
        if (t < s) {
            vs[t] = vs[t] + vs[t + s];
            cs[t] += cs[t + s];
        }
        __syncthreads();
    }
    *cnt = cs[0];
    const double out = vs[0];
    __syncthreads();
    return out;
}

// level 1: one workgroup per chunk of RED_CHUNK row partials
__global__ __launch_bounds__(energy::RED_LANES) void reduce_chunks_kernel(int64_t n, const double *__restrict__ rowsum, const int *__restrict__ rownzb,
                                                                          double *chunksum, long long *chunknzb)
{
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * energy::RED_CHUNK;
    long long cnt = 0;
    if (rownzb)
        for (int q = 0; q < energy::RED_PER; ++q) {
            const int64_t idx = base + (int64_t)t * energy::RED_PER + q;
            if (idx < n) cnt += rownzb[idx];
        }
    const double s = fold(energy::lane_partial(rowsum, n, base, t), &cnt);
    if (t == 0) {
        chunksum[blockIdx.x] = s;
        if (chunknzb) chunknzb[blockIdx.x] = cnt;
    }
}

// level 2, one workgroup: the chunk sums, and what the host loop would do with the result.  what 0: newsum at the head of iteration
// `iter` (stop flag, history, beta); 1: alpha = newsum / <P, AP>
__global__ __launch_bounds__(energy::RED_LANES) void reduce_final_kernel(int64_t nchunks, const double *__restrict__ chunksum,
                                                                         const long long *__restrict__ chunknzb, int what, int iter, double resid0,
                                                                         double blocksize, double tol, CgScalars *sc, double *history)
{
    const int t = threadIdx.x;
    long long cnt = 0;
    if (what == 0) for (int64_t idx = t; idx < nchunks; idx += energy::RED_LANES) cnt += chunknzb[idx];
    const double total = fold(energy::lane_strided(chunksum, nchunks, t), &cnt);
    if (t != 0) return;
    if (what == 1) {
        sc->alpha = sc->newsum / total;
        return;
    }
    const double resid = iter == 0 ? resid0 : (double)cnt * blocksize;
    const int stop = energy::cg_stop(resid, total, tol);
    sc->stop = stop;
    if (stop == 2) return;
    sc->newsum = total;
    history[iter] = total;
    sc->nsums = iter + 1;
    if (stop == 0) {
        if (iter > 0) sc->beta = total / sc->oldsum;
        sc->oldsum = total;
    }
}

// ---- GMRES.  Out = Dinv (A In) on the pattern (negate: Dinv (-(A In)), the initial residual from In = T), projected, and the row's
// partial of <With, Out>.  With is V_0 (the first coefficient of the column) or Out itself (the initial <R, R>)
template <int GW>
__global__ __launch_bounds__(BLK) void gmres_product_kernel(RowMap M, const int *__restrict__ Ap, const int *__restrict__ Aj, const double *__restrict__ Ax,
                                                            const double *__restrict__ In, double *Out, const double *__restrict__ Bc,
                                                            const double *__restrict__ BtBinv, const double *__restrict__ Dinv, const double *With,
                                                            int negate, double *rowsum)
{
    __shared__ double ub_s[(BLK / GW) * MAXQ];
    PAMG_EN_FOR_ROWS(GW) {
        PAMG_EN_ROW(GW);
        double *ub = ub_s + grp * MAXQ;
        if (live) energy::imm_scaled_lane(lane, GW, row, Ap, Aj, Ax, energy::StoredBlocks{In, M.r, M.c}, M.Sp, M.Sj, Dinv, Out, negate != 0, M.r, M.c);
        __syncthreads();
        if (live) energy::ub_lane(lane, GW, row, M.Sp, M.Sj, Out, Bc, ub, M.r, M.c, M.K);
        __syncthreads();
        if (live) energy::project_lane(lane, GW, row, M.Sp, M.Sj, Out, ub, BtBinv, Bc, M.r, M.c, M.K);
        __syncthreads();
        if (live && lane == 0) rowsum[row] = energy::row_dot(With, Out, (int64_t)M.Sp[row] * M.r * M.c, (int64_t)M.Sp[row + 1] * M.r * M.c);
    }
}

// one modified Gram-Schmidt pass, W -= h V_j with h = <V_j, W> from the reduction before it, and the row's partial of the next inner
// product: <Next, W> with Next = V_{j+1}, or Next = W after the last pass (the norm)
template <int GW>
__global__ __launch_bounds__(BLK) void gmres_mgs_kernel(RowMap M, double *W, const double *__restrict__ Vj, const double *Next,
                                                        const energy::GmresState *st, double *rowsum)
{
    const double h = st->h;
    PAMG_EN_FOR_ROWS(GW) {
        PAMG_EN_ROW(GW);
        if (live) energy::mgs_lane(lane, GW, row, M.Sp, W, Vj, h, M.r, M.c);
        __syncthreads();
        if (live && lane == 0) rowsum[row] = energy::row_dot(Next, W, (int64_t)M.Sp[row] * M.r * M.c, (int64_t)M.Sp[row + 1] * M.r * M.c);
    }
}

// V = scale V, unless the step before found nothing to normalise (normr = 0.0, or the breakdown H[i+1, i] = 0.0)
template <int GW>
__global__ __launch_bounds__(BLK) void gmres_scale_kernel(RowMap M, double *V, const energy::GmresState *st)
{
    if (!st->scaled) return;
    const double s = st->scale;
    PAMG_EN_FOR_ROWS(GW) {
        PAMG_EN_ROW(GW);
        if (live) energy::scale_lane(lane, GW, row, M.Sp, V, s, M.r, M.c);
    }
}

template <int GW>
__global__ __launch_bounds__(BLK) void gmres_combine_kernel(RowMap M, double *T, const double *__restrict__ V, int64_t stride, const double *__restrict__ y,
                                                            int ny, const unsigned char *__restrict__ cmask, const double *__restrict__ PI)
{
    PAMG_EN_FOR_ROWS(GW) {
        PAMG_EN_ROW(GW);
        if (live) energy::combine_lane(lane, GW, row, M.Sp, T, V, stride, y, ny, cmask, PI, M.r, M.c);
    }
}

// level 2 of a GMRES reduction, one workgroup, and the Krylov side's step with the result, by one lane.  what 0: <R, R> of the initial
// residual; 1: the coefficient H[j, i]; 2: <W, W>, the end of column i
__global__ __launch_bounds__(energy::RED_LANES) void gmres_step_kernel(int64_t nchunks, const double *__restrict__ chunksum, int what, int j, int i,
                                                                       int maxiter, double tol, energy::GmresState *st)
{
    long long none = 0;
    const double total = fold(energy::lane_strided(chunksum, nchunks, threadIdx.x), &none);
    if (threadIdx.x != 0) return;
    if (what == 0) energy::gmres_start(*st, total, maxiter, tol);
    else if (what == 1) energy::gmres_coefficient(*st, j, i, total);
    else energy::gmres_column(*st, i, total, maxiter, tol);
}

// ------------------------------------------------------------------------------------------------ host side
// launch KERNEL<GW> over the rows of M with GW from the pattern
#define PAMG_EN_LAUNCH(KERNEL, gw, M, ...)                                                                                        \
    do {                                                                                                                          \
        switch (gw) {                                                                                                             \
        case 8: hipLaunchKernelGGL((KERNEL<8>), dim3(launch_grid(M.n, BLK / 8, 16384)), dim3(BLK), 0, 0, M, __VA_ARGS__); break;   \
        case 16: hipLaunchKernelGGL((KERNEL<16>), dim3(launch_grid(M.n, BLK / 16, 16384)), dim3(BLK), 0, 0, M, __VA_ARGS__); break; \
        case 32: hipLaunchKernelGGL((KERNEL<32>), dim3(launch_grid(M.n, BLK / 32, 16384)), dim3(BLK), 0, 0, M, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL((KERNEL<64>), dim3(launch_grid(M.n, BLK / 64, 16384)), dim3(BLK), 0, 0, M, __VA_ARGS__); break; \
        }                                                                                                                         \
    } while (0)

bool shape_ok(int v) { return v >= 1; }
bool shape_fits(int r, int c, int K) { return r <= energy::MAX_BLOCK && c <= energy::MAX_BLOCK && K <= energy::MAX_NULLDIM; }

// the checks and uploads the two constraint entries share; UB == nullptr: U @ B on the device
int constraints(int r, int c, int n, int K, const double *Bc, int B_size, const double *UB, int UB_size, const double *BtBinv, int BtBinv_size,
                const int *Sp, int Sp_size, const int *Sj, int Sj_size, double *Sx, int Sx_size, bool with_ub)
{
    if (!shape_ok(r) || !shape_ok(c) || !shape_ok(K) || n < 0 || !Sp || Sp_size < n + 1) return PAMG_E_ARG;
    if (!shape_fits(r, c, K)) return PAMG_E_UNSUPPORTED;
    if (!Bc || B_size < 0 || B_size % (c * K) || !BtBinv || (int64_t)n * K * K > BtBinv_size) return PAMG_E_ARG;
    if (with_ub && (!UB || (int64_t)n * r * K > UB_size)) return PAMG_E_ARG;
    const int n_bcol = B_size / (c * K);
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(n, n_bcol, Sp, Sp_size, Sj, Sj_size, &nnz));
    const int64_t E = nnz * r * c;
    if (E > Sx_size || (E && !Sx)) return PAMG_E_ARG;
    if (n == 0 || nnz == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dSp, *dSj;
    double *dB, *dUB = nullptr, *dBt, *dSx;
    PAMG_TRY(d.put(&dSp, Sp, (size_t)n + 1)); PAMG_TRY(d.put(&dSj, Sj, (size_t)nnz));
    PAMG_TRY(d.put(&dB, Bc, (size_t)B_size)); PAMG_TRY(d.put(&dBt, BtBinv, (size_t)n * K * K));
    if (with_ub) PAMG_TRY(d.put(&dUB, UB, (size_t)n * r * K));
    PAMG_TRY(d.put(&dSx, (const double *)Sx, (size_t)E));
    const RowMap M{n, r, c, K, dSp, dSj};
    PAMG_EN_LAUNCH(constraints_kernel, energy::group_width(E, n), M, dB, dUB, dBt, dSx);
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(Sx, dSx, (size_t)E));
    return PAMG_OK;
}

// what the two Krylov drivers check of their common arguments before anything is written
int driver_arguments(int n, int n_bcol, int r, int c, int K, const int *Ap, int Ap_size, const int *Aj, int Aj_size, const double *Ax, int64_t Ax_size,
                     const int *Sp, int Sp_size, const int *Sj, int Sj_size, const double *Tx, int64_t Tx_size, const double *B, int B_size,
                     const double *BtBinv, int64_t BtBinv_size, const double *Dinv, int Dinv_size, const unsigned char *cmask, const double *PIx,
                     int maxiter, int64_t *nnzA, int64_t *nnzS, int64_t *E)
{
    if (!shape_ok(r) || !shape_ok(c) || !shape_ok(K) || n < 0 || n_bcol < 0 || maxiter < 0) return PAMG_E_ARG;
    if (!shape_fits(r, c, K)) return PAMG_E_UNSUPPORTED;
    if ((cmask == nullptr) != (PIx == nullptr)) return PAMG_E_ARG;
    PAMG_TRY(check_pattern(n, n, Ap, Ap_size, Aj, Aj_size, nnzA));
    PAMG_TRY(check_pattern(n, n_bcol, Sp, Sp_size, Sj, Sj_size, nnzS));
    *E = *nnzS * r * c;
    if (*nnzA * r * r > Ax_size || *E > Tx_size || (*nnzA && !Ax) || (*E && !Tx)) return PAMG_E_ARG;
    if (!B || (int64_t)n_bcol * c * K > B_size || !BtBinv || (int64_t)n * K * K > BtBinv_size || !Dinv || (int64_t)n * r > Dinv_size) return PAMG_E_ARG;
    return PAMG_OK;
}

}  // namespace

extern "C" {

int pamg_incomplete_mat_mult_bsr_f64(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const double *Ax, int Ax_size,
                                     const int32_t *Bp, int Bp_size, const int32_t *Bj, int Bj_size, const double *Bx, int Bx_size,
                                     const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size, double *Sx, int Sx_size, int32_t n_brow,
                                     int32_t n_bcol, int32_t brow_A, int32_t bcol_A, int32_t bcol_B)
{
    const int n = n_brow, r = brow_A, m = bcol_A, c = bcol_B;
    if (!shape_ok(r) || !shape_ok(m) || !shape_ok(c) || n < 0 || n_bcol < 0 || Bp_size < 1) return PAMG_E_ARG;
    if (!shape_fits(r, c, 1) || m > energy::MAX_BLOCK) return PAMG_E_UNSUPPORTED;
    const int nB = Bp_size - 1;                             // block rows of B = block columns of A
    int64_t nnzA = 0, nnzB = 0, nnzS = 0;
    PAMG_TRY(check_pattern(n, nB, Ap, Ap_size, Aj, Aj_size, &nnzA));
    PAMG_TRY(check_pattern(nB, n_bcol, Bp, Bp_size, Bj, Bj_size, &nnzB));
    PAMG_TRY(check_pattern(n, n_bcol, Sp, Sp_size, Sj, Sj_size, &nnzS));
    if (nnzA * r * m > Ax_size || nnzB * m * c > Bx_size || nnzS * r * c > Sx_size) return PAMG_E_ARG;
    if ((nnzA && !Ax) || (nnzB && !Bx) || (nnzS && !Sx)) return PAMG_E_ARG;
    if (n == 0 || nnzS == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dAp, *dAj, *dBp, *dBj, *dSp, *dSj;
    double *dAx, *dBx, *dSx;
    const int64_t E = nnzS * r * c;
    PAMG_TRY(d.put(&dAp, Ap, (size_t)n + 1)); PAMG_TRY(d.put(&dAj, Aj, (size_t)nnzA)); PAMG_TRY(d.put(&dAx, Ax, (size_t)(nnzA * r * m)));
    PAMG_TRY(d.put(&dBp, Bp, (size_t)nB + 1)); PAMG_TRY(d.put(&dBj, Bj, (size_t)nnzB)); PAMG_TRY(d.put(&dBx, Bx, (size_t)(nnzB * m * c)));
    PAMG_TRY(d.put(&dSp, Sp, (size_t)n + 1)); PAMG_TRY(d.put(&dSj, Sj, (size_t)nnzS)); PAMG_TRY(d.put(&dSx, (const double *)Sx, (size_t)E));
    const RowMap M{n, r, c, 1, dSp, dSj};
    PAMG_EN_LAUNCH(imm_kernel, energy::group_width(E, n), M, dAp, dAj, dAx, dBp, dBj, dBx, m, dSx);
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(Sx, dSx, (size_t)E));
    return PAMG_OK;
}

int pamg_satisfy_constraints_helper_f64(int32_t rows_per_block, int32_t cols_per_block, int32_t num_block_rows, int32_t NullDim,
                                        const double *Bt, int Bt_size, const double *UB, int UB_size, const double *BtBinv, int BtBinv_size,
                                        const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size, double *Sx, int Sx_size)
{
    return constraints(rows_per_block, cols_per_block, num_block_rows, NullDim, Bt, Bt_size, UB, UB_size, BtBinv, BtBinv_size, Sp, Sp_size, Sj,
                       Sj_size, Sx, Sx_size, true);
}

int pamg_satisfy_constraints_f64(int32_t rows_per_block, int32_t cols_per_block, int32_t num_block_rows, int32_t NullDim, const double *B,
                                 int B_size, const double *BtBinv, int BtBinv_size, const int32_t *Sp, int Sp_size, const int32_t *Sj,
                                 int Sj_size, double *Sx, int Sx_size)
{
    return constraints(rows_per_block, cols_per_block, num_block_rows, NullDim, B, B_size, nullptr, 0, BtBinv, BtBinv_size, Sp, Sp_size, Sj,
                       Sj_size, Sx, Sx_size, false);
}

int pamg_energy_cg_f64(int32_t n_brow, int32_t n_bcol, int32_t r, int32_t c, int32_t NullDim, const int32_t *Ap, int Ap_size,
                       const int32_t *Aj, int Aj_size, const double *Ax, int64_t Ax_size, const int32_t *Sp, int Sp_size, const int32_t *Sj,
                       int Sj_size, double *Tx, int64_t Tx_size, const double *B, int B_size, const double *BtBinv, int64_t BtBinv_size,
                       const double *Dinv, int Dinv_size, const unsigned char *cmask, const double *PIx, int32_t maxiter, double tol,
                       int32_t *iterations, double *newsums, int32_t *n_newsums)
{
    const int n = n_brow, K = NullDim;
    if (!iterations || !n_newsums || (maxiter > 0 && !newsums)) return PAMG_E_ARG;
    int64_t nnzA = 0, nnzS = 0, E = 0;
    PAMG_TRY(driver_arguments(n, n_bcol, r, c, K, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, Sp, Sp_size, Sj, Sj_size, Tx, Tx_size, B, B_size, BtBinv,
                              BtBinv_size, Dinv, Dinv_size, cmask, PIx, maxiter, &nnzA, &nnzS, &E));
    *iterations = 0;
    *n_newsums = 0;
    if (n == 0 || nnzS == 0 || maxiter == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dAp, *dAj, *dSp, *dSj, *dnzb;
    double *dAx, *dT, *dB, *dBt, *dDinv, *dPI = nullptr, *dR, *dP[2], *dAP, *drow, *dchunk, *dhist;
    unsigned char *dmask = nullptr;
    long long *dchunknzb;
    CgScalars *dsc;
    const int64_t nchunks = energy::chunks(n);
    PAMG_TRY(d.put(&dAp, Ap, (size_t)n + 1)); PAMG_TRY(d.put(&dAj, Aj, (size_t)nnzA)); PAMG_TRY(d.put(&dAx, Ax, (size_t)(nnzA * r * r)));
    PAMG_TRY(d.put(&dSp, Sp, (size_t)n + 1)); PAMG_TRY(d.put(&dSj, Sj, (size_t)nnzS)); PAMG_TRY(d.put(&dT, (const double *)Tx, (size_t)E));
    PAMG_TRY(d.put(&dB, B, (size_t)n_bcol * c * K)); PAMG_TRY(d.put(&dBt, BtBinv, (size_t)n * K * K)); PAMG_TRY(d.put(&dDinv, Dinv, (size_t)n * r));
    if (cmask) { PAMG_TRY(d.put(&dmask, cmask, (size_t)n * r)); PAMG_TRY(d.put(&dPI, PIx, (size_t)E)); }
    PAMG_TRY(d.get(&dR, (size_t)E)); PAMG_TRY(d.get(&dP[0], (size_t)E)); PAMG_TRY(d.get(&dP[1], (size_t)E)); PAMG_TRY(d.get(&dAP, (size_t)E));
    PAMG_TRY(d.get(&drow, (size_t)n)); PAMG_TRY(d.get(&dnzb, (size_t)n)); PAMG_TRY(d.get(&dchunk, (size_t)nchunks));
    PAMG_TRY(d.get(&dchunknzb, (size_t)nchunks)); PAMG_TRY(d.get(&dhist, (size_t)maxiter)); PAMG_TRY(d.get(&dsc, 1));
    PAMG_HIP(hipMemset(dsc, 0, sizeof(CgScalars)));
    const RowMap M{n, r, c, K, dSp, dSj};
    const int gw = energy::group_width(E, n);
    const double bs = (double)r * c, resid0 = (double)nnzS * bs;
    auto reduce = [&](int what, int iter) {
        hipLaunchKernelGGL(reduce_chunks_kernel, dim3((unsigned)nchunks), dim3(energy::RED_LANES), 0, 0, (int64_t)n, drow, what == 0 ? dnzb : nullptr,
                           dchunk, what == 0 ? dchunknzb : nullptr);
        hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(energy::RED_LANES), 0, 0, nchunks, dchunk, dchunknzb, what, iter, resid0, bs, tol, dsc, dhist);
    };
    PAMG_EN_LAUNCH(cg_init_kernel, gw, M, dAp, dAj, dAx, dT, dB, dBt, dDinv, dR, drow, dnzb);
    PAMG_HIP(hipGetLastError());
    int it = 0, cur = 0;
    for (; it < maxiter; ++it) {
        reduce(0, it);
        PAMG_HIP(hipGetLastError());
        int stop = 0;
        PAMG_HIP(hipMemcpy(&stop, &dsc->stop, sizeof(int), hipMemcpyDeviceToHost));     // the one value read back per iteration
        if (stop) break;
        PAMG_EN_LAUNCH(cg_direction_kernel, gw, M, dAp, dAj, dAx, dR, dP[cur], dP[cur ^ 1], dAP, dB, dBt, dDinv, dsc, it == 0 ? 1 : 0, drow);
        reduce(1, it);
        PAMG_EN_LAUNCH(cg_update_kernel, gw, M, dT, dR, dP[cur ^ 1], dAP, dsc, dmask, dPI, dDinv, drow, dnzb);
        PAMG_HIP(hipGetLastError());
        cur ^= 1;
    }
    CgScalars sc;
    PAMG_TRY(Bufs::fetch(&sc, dsc, 1));
    PAMG_TRY(Bufs::fetch(newsums, dhist, (size_t)sc.nsums));
    PAMG_TRY(Bufs::fetch(Tx, dT, (size_t)E));
    *iterations = it;
    *n_newsums = sc.nsums;
    return PAMG_OK;
}

int pamg_energy_gmres_f64(int32_t n_brow, int32_t n_bcol, int32_t r, int32_t c, int32_t NullDim, const int32_t *Ap, int Ap_size,
                          const int32_t *Aj, int Aj_size, const double *Ax, int64_t Ax_size, const int32_t *Sp, int Sp_size, const int32_t *Sj,
                          int Sj_size, double *Tx, int64_t Tx_size, const double *B, int B_size, const double *BtBinv, int64_t BtBinv_size,
                          const double *Dinv, int Dinv_size, const unsigned char *cmask, const double *PIx, int32_t maxiter, double tol,
                          int32_t *iterations, double *normrs, int32_t *n_normrs, double *H)
{
    const int n = n_brow, K = NullDim;
    if (!iterations || !n_normrs || !normrs) return PAMG_E_ARG;
    int64_t nnzA = 0, nnzS = 0, E = 0;
    PAMG_TRY(driver_arguments(n, n_bcol, r, c, K, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, Sp, Sp_size, Sj, Sj_size, Tx, Tx_size, B, B_size, BtBinv,
                              BtBinv_size, Dinv, Dinv_size, cmask, PIx, maxiter, &nnzA, &nnzS, &E));
    if (maxiter > energy::GMRES_MAXITER) return PAMG_E_UNSUPPORTED;         // the basis: maxiter + 1 arrays of the pattern's size
    *iterations = 0;
    *n_normrs = 0;
    if (n == 0 || nnzS == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dAp, *dAj, *dSp, *dSj;
    double *dAx, *dT, *dB, *dBt, *dDinv, *dPI = nullptr, *dV, *drow, *dchunk, *dy;
    unsigned char *dmask = nullptr;
    energy::GmresState *dst;
    const int64_t nchunks = energy::chunks(n);
    PAMG_TRY(d.put(&dAp, Ap, (size_t)n + 1)); PAMG_TRY(d.put(&dAj, Aj, (size_t)nnzA)); PAMG_TRY(d.put(&dAx, Ax, (size_t)(nnzA * r * r)));
    PAMG_TRY(d.put(&dSp, Sp, (size_t)n + 1)); PAMG_TRY(d.put(&dSj, Sj, (size_t)nnzS)); PAMG_TRY(d.put(&dT, (const double *)Tx, (size_t)E));
    PAMG_TRY(d.put(&dB, B, (size_t)n_bcol * c * K)); PAMG_TRY(d.put(&dBt, BtBinv, (size_t)n * K * K)); PAMG_TRY(d.put(&dDinv, Dinv, (size_t)n * r));
    if (cmask) { PAMG_TRY(d.put(&dmask, cmask, (size_t)n * r)); PAMG_TRY(d.put(&dPI, PIx, (size_t)E)); }
    PAMG_TRY(d.get(&dV, (size_t)E * (maxiter + 1)));         // the Krylov basis V_0 .. V_maxiter
    PAMG_TRY(d.get(&drow, (size_t)n)); PAMG_TRY(d.get(&dchunk, (size_t)nchunks)); PAMG_TRY(d.get(&dy, (size_t)energy::GMRES_MAXITER));
    PAMG_TRY(d.get(&dst, 1));
    PAMG_HIP(hipMemset(dst, 0, sizeof(energy::GmresState)));
    const RowMap M{n, r, c, K, dSp, dSj};
    const int gw = energy::group_width(E, n);
    auto basis = [&](int j) { return dV + (int64_t)j * E; };
    auto reduce = [&](int what, int j, int i) {
        hipLaunchKernelGGL(reduce_chunks_kernel, dim3((unsigned)nchunks), dim3(energy::RED_LANES), 0, 0, (int64_t)n, drow, nullptr, dchunk, nullptr);
        hipLaunchKernelGGL(gmres_step_kernel, dim3(1), dim3(energy::RED_LANES), 0, 0, nchunks, dchunk, what, j, i, (int)maxiter, tol, dst);
    };
    PAMG_EN_LAUNCH(gmres_product_kernel, gw, M, dAp, dAj, dAx, dT, basis(0), dB, dBt, dDinv, basis(0), 1, drow);
    reduce(0, 0, 0);
    PAMG_EN_LAUNCH(gmres_scale_kernel, gw, M, basis(0), dst);                          // V_0 = (1.0 / normr) R
    PAMG_HIP(hipGetLastError());
    for (int i = 0; i < maxiter; ++i) {
        int stop = 0;
        PAMG_HIP(hipMemcpy(&stop, &dst->stop, sizeof(int), hipMemcpyDeviceToHost));    // the one value read back per iteration
        if (stop) break;
        double *W = basis(i + 1);
        PAMG_EN_LAUNCH(gmres_product_kernel, gw, M, dAp, dAj, dAx, basis(i), W, dB, dBt, dDinv, basis(0), 0, drow);
        reduce(1, 0, i);
        for (int j = 0; j <= i; ++j) {
            PAMG_EN_LAUNCH(gmres_mgs_kernel, gw, M, W, basis(j), j < i ? basis(j + 1) : W, dst, drow);
            if (j < i) reduce(1, j + 1, i);
            else reduce(2, 0, i);
        }
        PAMG_EN_LAUNCH(gmres_scale_kernel, gw, M, W, dst);                             // V_{i+1} = (1.0 / H[i+1, i]) W
        PAMG_HIP(hipGetLastError());
    }
    std::vector<energy::GmresState> st(1);
    PAMG_TRY(Bufs::fetch(st.data(), dst, 1));
    const int its = st[0].iterations;
    double y[energy::GMRES_MAXITER] = {0.0};
    if (its > 0) {
        energy::gmres_solve(st[0], its, y);                  // at most maxiter x maxiter: on the host, as the reference's la.solve
        PAMG_HIP(hipMemcpy(dy, y, sizeof(double) * (size_t)its, hipMemcpyHostToDevice));
    }
    if (its > 0 || cmask) {
        PAMG_EN_LAUNCH(gmres_combine_kernel, gw, M, dT, dV, E, dy, its, dmask, dPI);
        PAMG_HIP(hipGetLastError());
    }
    PAMG_TRY(Bufs::fetch(Tx, dT, (size_t)E));
    for (int q = 0; q <= its; ++q) normrs[q] = st[0].normr[q];
    if (H)
        for (int a = 0; a <= maxiter; ++a)
            for (int b = 0; b <= maxiter; ++b) H[a * (maxiter + 1) + b] = st[0].H[a * energy::GMRES_LD + b];
    *iterations = its;
    *n_normrs = its + 1;
    return PAMG_OK;
}

}  // extern "C"
