// pamg_evolution.hip -- the amg_core calls of the evolution strength measure (evolution_strength.h) on the device.  Layer 1 of the C ABI:
// HOST arrays in, HOST arrays out, amg_core's argument order.  The per-row / per-entry arithmetic is pamg_evolution.h (replayed on the
// host by tests/evolution_emul.cpp); every result is the reference's, bit for bit.
//
//   incomplete_mat_mult  a group of 16 lanes per row of S; a lane owns the entries p, p + 16, ... of the row and walks the row of A and
//                        its column of B by the two-pointer merge.  The row of A is read by all lanes of the group at the same time
//                        (one request, from L1 after the first), so it is not staged; rows longer than the group loop
//   helper               one row per lane, one wave per workgroup, one instantiation per K1 = K + 1 = 2 .. 7.  With K1 a template constant
//                        the loops of the SVD unroll, and the two factors, the singular values, LHS and RHS (3 K1^2 + 3 K1 doubles, 168 at
//                        K1 = 7) stay in registers: no scratch and no LDS in any instantiation; at K1 = 7 the compiler reports 256 VGPRs
//                        plus 43 AGPRs, 18 of the former spilled into the latter, one wave per SIMD.  z, zhat, Bi and DBi
//                        are re-gathered, so there is no cap on the row length
//   filters, min_blocks  one lane per row / per block
//   one candidate        the group-per-row mapping of the product again, one fused expression per stored entry
//
// Plain launches only; no lane of any kernel waits for another.
#include "pamg_common.h"
#include "pamg_evolution.h"
#include "pamg_host_call.h"

#include <climits>

using namespace pamg;

namespace {

constexpr int GW = 16;                      // lanes per row of the entry-parallel kernels
constexpr int HBLK = 64;                    // the helper: one wave per workgroup, so that a long solve holds back 63 rows and no more

int egrid(int64_t n, int per_block) { return launch_grid(n, per_block, 16384); }

// ------------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(BLK) void imm_kernel(int n, const int *__restrict__ Ap, const int *__restrict__ Aj, const double *__restrict__ Ax,
                                                  const int *__restrict__ Bp, const int *__restrict__ Bj, const double *__restrict__ Bx,
                                                  const int *__restrict__ Sp, const int *__restrict__ Sj, double *__restrict__ Sx)
{
    const int lane = threadIdx.x % GW;
    for (int64_t row = ((int64_t)blockIdx.x * BLK + threadIdx.x) / GW; row < n; row += (int64_t)gridDim.x * (BLK / GW)) {
        const int r1 = Sp[row + 1];
        for (int p = Sp[row] + lane; p < r1; p += GW) Sx[p] = evo::inner(Ap, Aj, Ax, Bp, Bj, Bx, (int)row, Sj[p]);
    }
}

template <int K1>
__global__ __launch_bounds__(HBLK) void helper_kernel(int nrows, double *Sx, const int *__restrict__ Sp, const int *__restrict__ Sj,
                                                      const double *__restrict__ B, const double *__restrict__ DB, const double *__restrict__ BDB,
                                                      double tol)
{
    for (int64_t i = (int64_t)blockIdx.x * HBLK + threadIdx.x; i < nrows; i += (int64_t)gridDim.x * HBLK)
        evo::helper_row<K1>((int)i, Sx, Sp, Sj, nrows, B, DB, BDB, tol);
}

template <bool RELATIVE>
__global__ __launch_bounds__(BLK) void distance_kernel(int n, double epsilon, const int *__restrict__ Sp, const int *__restrict__ Sj, double *Sx)
{
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLK) evo::distance_row<RELATIVE>((int)i, epsilon, Sp, Sj, Sx);
}

__global__ __launch_bounds__(BLK) void min_blocks_kernel(int n_blocks, int blocksize, const double *__restrict__ Sx, double *__restrict__ Tx)
{
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < n_blocks; i += (int64_t)gridDim.x * BLK) Tx[i] = evo::block_min(Sx + i * blocksize, blocksize);
}

__global__ __launch_bounds__(BLK) void vector_kernel(int n, double *Sx, const int *__restrict__ Sp, const int *__restrict__ Sj,
                                                     const double *__restrict__ d, const double *__restrict__ b)
{
    const int lane = threadIdx.x % GW;
    for (int64_t row = ((int64_t)blockIdx.x * BLK + threadIdx.x) / GW; row < n; row += (int64_t)gridDim.x * (BLK / GW)) {
        const int r1 = Sp[row + 1];
        const double di = d[row], bi = b[row];
        for (int p = Sp[row] + lane; p < r1; p += GW) Sx[p] = evo::vector_entry(Sx[p], di, bi, b[Sj[p]]);
    }
}

template <int K1>
void launch_helper(int nrows, double *Sx, const int *Sp, const int *Sj, const double *B, const double *DB, const double *BDB, double tol)
{
    hipLaunchKernelGGL((helper_kernel<K1>), dim3(egrid(nrows, HBLK)), dim3(HBLK), 0, 0, nrows, Sx, Sp, Sj, B, DB, BDB, tol);
}

// Sx of nnz entries up, the kernel, Sx down
template <typename Launch>
int on_values(double *Sx, int64_t nnz, Bufs &d, Launch &&launch)
{
    double *dSx;
    PAMG_TRY(d.put(&dSx, (const double *)Sx, (size_t)nnz));
    launch(dSx);
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(Sx, dSx, (size_t)nnz));
    if (!nnz) PAMG_HIP(hipDeviceSynchronize());
    return PAMG_OK;
}

template <bool RELATIVE>
int distance_filter(int n_row, double epsilon, const int *Sp, int Sp_size, const int *Sj, int Sj_size, double *Sx, int Sx_size)
{
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(n_row, INT_MAX, Sp, Sp_size, Sj, Sj_size, &nnz, true, Sx, Sx_size));
    if (n_row == 0 || nnz == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dSp, *dSj;
    PAMG_TRY(d.put(&dSp, Sp, (size_t)n_row + 1)); PAMG_TRY(d.put(&dSj, Sj, (size_t)nnz));
    return on_values(Sx, nnz, d, [&](double *dSx) {
        hipLaunchKernelGGL((distance_kernel<RELATIVE>), dim3(egrid(n_row, BLK)), dim3(BLK), 0, 0, n_row, epsilon, dSp, dSj, dSx);
    });
}

}  // namespace

extern "C" {

int pamg_incomplete_mat_mult_csr_f64(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const double *Ax, int Ax_size,
                                     const int32_t *Bp, int Bp_size, const int32_t *Bj, int Bj_size, const double *Bx, int Bx_size,
                                     const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size, double *Sx, int Sx_size, int32_t num_rows)
{
    const int n = num_rows;
    int64_t nnzA = 0, nnzB = 0, nnzS = 0;
    PAMG_TRY(check_pattern(n, n, Ap, Ap_size, Aj, Aj_size, &nnzA, true, Ax, Ax_size));
    PAMG_TRY(check_pattern(n, n, Bp, Bp_size, Bj, Bj_size, &nnzB, true, Bx, Bx_size));
    PAMG_TRY(check_pattern(n, n, Sp, Sp_size, Sj, Sj_size, &nnzS, true, Sx, Sx_size));
    if (n == 0 || nnzS == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dAp, *dAj, *dBp, *dBj, *dSp, *dSj;
    double *dAx, *dBx, *dSx;
    PAMG_TRY(d.put(&dAp, Ap, (size_t)n + 1)); PAMG_TRY(d.put(&dAj, Aj, (size_t)nnzA)); PAMG_TRY(d.put(&dAx, Ax, (size_t)nnzA));
    PAMG_TRY(d.put(&dBp, Bp, (size_t)n + 1)); PAMG_TRY(d.put(&dBj, Bj, (size_t)nnzB)); PAMG_TRY(d.put(&dBx, Bx, (size_t)nnzB));
    PAMG_TRY(d.put(&dSp, Sp, (size_t)n + 1)); PAMG_TRY(d.put(&dSj, Sj, (size_t)nnzS)); PAMG_TRY(d.get(&dSx, (size_t)nnzS));
    hipLaunchKernelGGL(imm_kernel, dim3(egrid(n, BLK / GW)), dim3(BLK), 0, 0, n, dAp, dAj, dAx, dBp, dBj, dBx, dSp, dSj, dSx);
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(Sx, dSx, (size_t)nnzS));
    return PAMG_OK;
}

int pamg_evolution_strength_helper_f64(double *Sx, int Sx_size, const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size, int32_t nrows,
                                       const double *x, int x_size, const double *y, int y_size, const double *b, int b_size,
                                       int32_t BDBCols, int32_t NullDim, double tol)
{
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(nrows, nrows, Sp, Sp_size, Sj, Sj_size, &nnz, true, Sx, Sx_size));
    if (NullDim < 1 || !x || !y || !b) return PAMG_E_ARG;
    if (NullDim > evo::MAX_NULLDIM) return PAMG_E_UNSUPPORTED;
    if (BDBCols != NullDim * (NullDim + 1) / 2) return PAMG_E_ARG;
    if ((int64_t)nrows * NullDim > x_size || (int64_t)nrows * NullDim > y_size || (int64_t)nrows * BDBCols > b_size) return PAMG_E_ARG;
    if (nrows == 0 || nnz == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dSp, *dSj;
    double *dB, *dDB, *dBDB;
    PAMG_TRY(d.put(&dSp, Sp, (size_t)nrows + 1)); PAMG_TRY(d.put(&dSj, Sj, (size_t)nnz));
    PAMG_TRY(d.put(&dB, x, (size_t)nrows * NullDim)); PAMG_TRY(d.put(&dDB, y, (size_t)nrows * NullDim));
    PAMG_TRY(d.put(&dBDB, b, (size_t)nrows * BDBCols));
    return on_values(Sx, nnz, d, [&](double *dSx) {
        switch (NullDim) {
        case 1: launch_helper<2>(nrows, dSx, dSp, dSj, dB, dDB, dBDB, tol); break;
        case 2: launch_helper<3>(nrows, dSx, dSp, dSj, dB, dDB, dBDB, tol); break;
        case 3: launch_helper<4>(nrows, dSx, dSp, dSj, dB, dDB, dBDB, tol); break;
        case 4: launch_helper<5>(nrows, dSx, dSp, dSj, dB, dDB, dBDB, tol); break;
        case 5: launch_helper<6>(nrows, dSx, dSp, dSj, dB, dDB, dBDB, tol); break;
        default: launch_helper<7>(nrows, dSx, dSp, dSj, dB, dDB, dBDB, tol); break;
        }
    });
}

int pamg_apply_distance_filter_f64(int32_t n_row, double epsilon, const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size, double *Sx,
                                   int Sx_size)
{
    return distance_filter<true>(n_row, epsilon, Sp, Sp_size, Sj, Sj_size, Sx, Sx_size);
}

int pamg_apply_absolute_distance_filter_f64(int32_t n_row, double epsilon, const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size,
                                            double *Sx, int Sx_size)
{
    return distance_filter<false>(n_row, epsilon, Sp, Sp_size, Sj, Sj_size, Sx, Sx_size);
}

int pamg_min_blocks_f64(int32_t n_blocks, int32_t blocksize, const double *Sx, int Sx_size, double *Tx, int Tx_size)
{
    if (n_blocks < 0 || blocksize < 0 || Sx_size < 0 || Tx_size < 0) return PAMG_E_ARG;
    const int64_t total = (int64_t)n_blocks * blocksize;
    if (total > Sx_size || n_blocks > Tx_size || (total && !Sx) || (n_blocks && !Tx)) return PAMG_E_ARG;
    if (n_blocks == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    double *dSx, *dTx;
    PAMG_TRY(d.put(&dSx, Sx, (size_t)total)); PAMG_TRY(d.get(&dTx, (size_t)n_blocks));
    hipLaunchKernelGGL(min_blocks_kernel, dim3(egrid(n_blocks, BLK)), dim3(BLK), 0, 0, n_blocks, blocksize, dSx, dTx);
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(Tx, dTx, (size_t)n_blocks));
    return PAMG_OK;
}

int pamg_evolution_strength_vector_f64(double *Sx, int Sx_size, const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size, int32_t nrows,
                                       const double *d, int d_size, const double *b, int b_size)
{
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(nrows, nrows, Sp, Sp_size, Sj, Sj_size, &nnz, true, Sx, Sx_size));
    if (!d || !b || d_size < nrows || b_size < nrows) return PAMG_E_ARG;
    if (nrows == 0 || nnz == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs bufs;
    int *dSp, *dSj;
    double *dd, *db;
    PAMG_TRY(bufs.put(&dSp, Sp, (size_t)nrows + 1)); PAMG_TRY(bufs.put(&dSj, Sj, (size_t)nnz));
    PAMG_TRY(bufs.put(&dd, d, (size_t)nrows)); PAMG_TRY(bufs.put(&db, b, (size_t)nrows));
    return on_values(Sx, nnz, bufs, [&](double *dSx) {
        hipLaunchKernelGGL(vector_kernel, dim3(egrid(nrows, BLK / GW)), dim3(BLK), 0, 0, nrows, dSx, dSp, dSj, dd, db);
    });
}

}  // extern "C"
