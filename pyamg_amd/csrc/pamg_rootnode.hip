// pamg_rootnode.hip -- the setup pieces of rootnode_solver around the energy-minimisation loop, on the device: amg_core::calc_BtB
// (smoothed_aggregation.h:829-907), compute_BtBinv (util/utils.py:1533-1624) and scale_T (util/utils.py:1275-1381).  The arithmetic is
// pamg_rootnode.h, replayed on the host by tests/rootnode_emul.cpp.
//
// calc_BtB: a group of GW = 8 / 32 lanes per node, a lane per entry of the upper triangle (K (K + 1) / 2 <= 21 of them); every lane walks
// the node's pattern row serially -- stored blocks in stored order, the columns of a block ascending -- with one accumulator, which is
// the reference's summation order, so BtB is the reference's bit for bit.  The column indices are one address for the whole group, and
// the K candidates of a row of B are one span of at most 48 bytes that the group's lanes read together.  A row of any length is taken by
// the same group.  The products conj(B[k, i]) B[k, j] come from the caller's Bsq (the Layer-1 twin of amg_core.calc_BtB) or are formed
// from B where they are used (compute_BtBinv), one rounded product either way.
//
// compute_BtBinv: calc_BtB, then one lane per node transposes its block and pseudo-inverts it in place (K == 1: reciprocal, zero stays
// zero; K > 1: the one-sided Jacobi SVD of pamg_jacobi_svd.h with gelss' rank rule at cond = 1e6 eps).  BtB never leaves the device.
//
// scale_T: one lane per aggregate gathers the root row's block of T (D = P_I.T @ T) and pseudo-inverts it; then one lane per stored
// element of T forms its element of T @ D in the order of SciPy's gemm, or of the injected identity in a root row.
//
// Plain launches only.
#include "pamg_common.h"
#include "pamg_energy.h"
#include "pamg_host_call.h"
#include "pamg_rootnode.h"

using namespace pamg;

namespace {

template <int GW, class Product>
__global__ __launch_bounds__(BLK) void btb_kernel(int n, int K, int cols_per_block, Product prod, const int *__restrict__ Sp,
                                                  const int *__restrict__ Sj, double *BtB)
{
    const int lane = threadIdx.x % GW, grp = threadIdx.x / GW, T = rootnode::tri_count(K);
    for (int64_t node = (int64_t)blockIdx.x * (BLK / GW) + grp; node < n; node += (int64_t)gridDim.x * (BLK / GW))
        if (lane < T) rootnode::btb_lane(prod, K, lane, Sp, Sj, (int)node, cols_per_block, BtB);
}

template <class Product>
void btb_launch(int n, int K, int cpb, Product prod, const int *dSp, const int *dSj, double *dBtB)
{
    if (rootnode::tri_count(K) <= 8)
        hipLaunchKernelGGL((btb_kernel<8, Product>), dim3(launch_grid(n, BLK / 8, 16384)), dim3(BLK), 0, 0, n, K, cpb, prod, dSp, dSj, dBtB);
    else
        hipLaunchKernelGGL((btb_kernel<32, Product>), dim3(launch_grid(n, BLK / 32, 16384)), dim3(BLK), 0, 0, n, K, cpb, prod, dSp, dSj, dBtB);
}

// the deep transpose and pinv_array of the blocks [m, n, n], in place, a lane per block
__global__ __launch_bounds__(64) void pinv_kernel(int64_t m, int n, int transpose, double rank_tol, double *AA)
{
    const int64_t blk = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (blk >= m) return;
    double *a = AA + blk * n * n;
    if (transpose)
        for (int r = 0; r < n; ++r)
            for (int c = r + 1; c < n; ++c) {
                const double up = a[r * n + c];
                a[r * n + c] = a[c * n + r];
                a[c * n + r] = up;
            }
    rootnode::pinv_block(a, n, rank_tol);
}

__global__ __launch_bounds__(64) void root_blocks_kernel(int n_agg, int bs, const int *__restrict__ Tp, const int *__restrict__ Cnodes,
                                                         const double *__restrict__ Tx, double rank_tol, double *D)
{
    const int a = blockIdx.x * 64 + threadIdx.x;
    if (a >= n_agg) return;
    double *d = D + (int64_t)a * bs * bs;
    rootnode::gather_root_block(Tx, Tp[Cnodes[a]], bs, d);
    rootnode::pinv_block(d, bs, rank_tol);
}

__global__ __launch_bounds__(BLK) void scale_kernel(int64_t E, int bs, const int *__restrict__ Tj, const double *__restrict__ Tx,
                                                    const double *__restrict__ D, const unsigned char *__restrict__ is_root,
                                                    const int *__restrict__ row_of, double *out)
{
    for (int64_t e = (int64_t)blockIdx.x * BLK + threadIdx.x; e < E; e += (int64_t)gridDim.x * BLK)
        out[e] = rootnode::scale_element(e, bs, Tj, Tx, D, is_root, row_of);
}

// filter_operator's projection: diff = S @ B - Bf for a block row (pamg_energy.h's U @ B, the order of SciPy's bsr_matvecs, then one
// subtraction), and Sx -= diff_i (BtBinv_i B_j^H) on its stored blocks.  A group of GW lanes per block row, as in pamg_energy.hip
template <int GW>
__global__ __launch_bounds__(BLK) void filter_kernel(int n, int r, int c, int K, const int *__restrict__ Sp, const int *__restrict__ Sj,
                                                     const double *__restrict__ Bc, const double *__restrict__ Bf, const double *__restrict__ BtBinv,
                                                     double *Sx)
{
    __shared__ double ub_s[(BLK / GW) * rootnode::MAX_BLOCK * rootnode::MAX_NULLDIM];
    const int lane = threadIdx.x % GW, grp = threadIdx.x / GW;
    double *ub = ub_s + grp * rootnode::MAX_BLOCK * rootnode::MAX_NULLDIM;
    for (int64_t base = (int64_t)blockIdx.x * (BLK / GW); base < n; base += (int64_t)gridDim.x * (BLK / GW)) {     // workgroup-uniform passes
        const bool live = base + grp < n;
        const int row = live ? (int)(base + grp) : 0;
        if (live) {
            energy::ub_lane(lane, GW, row, Sp, Sj, Sx, Bc, ub, r, c, K);
            for (int q = lane; q < r * K; q += GW) ub[q] = rootnode::constraint_defect(ub[q], Bf[(int64_t)row * r * K + q]);
        }
        __syncthreads();
        if (live) energy::project_lane(lane, GW, row, Sp, Sj, Sx, ub, BtBinv, Bc, r, c, K);
        __syncthreads();
    }
}

// what calc_BtB and compute_BtBinv check: the shapes, the pattern against the rows of the candidates
int btb_arguments(int K, int n, int cpb, int64_t rows_of_B, const int *Sp, int Sp_size, const int *Sj, int Sj_size, int64_t *nnz)
{
    if (K < 1 || cpb < 1 || n < 0 || rows_of_B < 0) return PAMG_E_ARG;
    if (K > rootnode::MAX_NULLDIM || cpb > rootnode::MAX_BLOCK) return PAMG_E_UNSUPPORTED;
    if (rows_of_B % cpb || rows_of_B / cpb > INT32_MAX) return PAMG_E_ARG;
    return check_pattern(n, (int)(rows_of_B / cpb), Sp, Sp_size, Sj, Sj_size, nnz);
}

}  // namespace

extern "C" {

int pamg_calc_BtB_f64(int32_t NullDim, int32_t Nnodes, int32_t cols_per_block, const double *b, int b_size, int32_t BsqCols, double *x,
                      int x_size, const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size)
{
    const int K = NullDim, n = Nnodes;
    if (K < 1 || BsqCols != rootnode::tri_count(K) || !b || b_size < 0 || b_size % BsqCols) return K > rootnode::MAX_NULLDIM ? PAMG_E_UNSUPPORTED : PAMG_E_ARG;
    int64_t nnz = 0;
    PAMG_TRY(btb_arguments(K, n, cols_per_block, b_size / BsqCols, Sp, Sp_size, Sj, Sj_size, &nnz));
    if ((int64_t)n * K * K > x_size || (n && !x)) return PAMG_E_ARG;
    if (n == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dSp, *dSj;
    double *db, *dx;
    PAMG_TRY(d.put(&dSp, Sp, (size_t)n + 1)); PAMG_TRY(d.put(&dSj, Sj, (size_t)nnz)); PAMG_TRY(d.put(&db, b, (size_t)b_size));
    PAMG_TRY(d.get(&dx, (size_t)n * K * K));
    btb_launch(n, K, cols_per_block, rootnode::Squares{db, BsqCols}, dSp, dSj, dx);
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(x, dx, (size_t)n * K * K));
    return PAMG_OK;
}

int pamg_compute_BtBinv_f64(int32_t NullDim, int32_t Nnodes, int32_t cols_per_block, const double *B, int64_t B_size, const int32_t *Sp,
                            int Sp_size, const int32_t *Sj, int Sj_size, double *BtBinv, int64_t BtBinv_size)
{
    const int K = NullDim, n = Nnodes;
    if (K < 1 || !B || B_size < 0 || B_size % K) return PAMG_E_ARG;
    int64_t nnz = 0;
    PAMG_TRY(btb_arguments(K, n, cols_per_block, B_size / K, Sp, Sp_size, Sj, Sj_size, &nnz));
    if ((int64_t)n * K * K > BtBinv_size || (n && !BtBinv)) return PAMG_E_ARG;
    if (n == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dSp, *dSj;
    double *dB, *dx;
    PAMG_TRY(d.put(&dSp, Sp, (size_t)n + 1)); PAMG_TRY(d.put(&dSj, Sj, (size_t)nnz)); PAMG_TRY(d.put(&dB, B, (size_t)B_size));
    PAMG_TRY(d.get(&dx, (size_t)n * K * K));
    btb_launch(n, K, cols_per_block, rootnode::Candidates{dB, K}, dSp, dSj, dx);
    hipLaunchKernelGGL(pinv_kernel, dim3((unsigned)launch_grid(n, 64, INT32_MAX)), dim3(64), 0, 0, (int64_t)n, K, 1, rootnode::rank_tol_f64(), dx);
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(BtBinv, dx, (size_t)n * K * K));
    return PAMG_OK;
}

int pamg_filter_constraints_f64(int32_t rows_per_block, int32_t cols_per_block, int32_t num_block_rows, int32_t NullDim, const double *B,
                                int B_size, const double *Bf, int Bf_size, const double *BtBinv, int BtBinv_size, const int32_t *Sp,
                                int Sp_size, const int32_t *Sj, int Sj_size, double *Sx, int Sx_size)
{
    const int r = rows_per_block, c = cols_per_block, n = num_block_rows, K = NullDim;
    if (r < 1 || c < 1 || K < 1 || n < 0) return PAMG_E_ARG;
    if (r > rootnode::MAX_BLOCK || c > rootnode::MAX_BLOCK || K > rootnode::MAX_NULLDIM) return PAMG_E_UNSUPPORTED;
    if (!B || B_size < 0 || B_size % (c * K) || !Bf || (int64_t)n * r * K > Bf_size || !BtBinv || (int64_t)n * K * K > BtBinv_size) return PAMG_E_ARG;
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(n, B_size / (c * K), Sp, Sp_size, Sj, Sj_size, &nnz));
    const int64_t E = nnz * r * c;
    if (E > Sx_size || (E && !Sx)) return PAMG_E_ARG;
    if (n == 0 || nnz == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dSp, *dSj;
    double *dB, *dBf, *dBt, *dSx;
    PAMG_TRY(d.put(&dSp, Sp, (size_t)n + 1)); PAMG_TRY(d.put(&dSj, Sj, (size_t)nnz)); PAMG_TRY(d.put(&dB, B, (size_t)B_size));
    PAMG_TRY(d.put(&dBf, Bf, (size_t)n * r * K)); PAMG_TRY(d.put(&dBt, BtBinv, (size_t)n * K * K)); PAMG_TRY(d.put(&dSx, (const double *)Sx, (size_t)E));
    switch (energy::group_width(E, n)) {
    case 8: hipLaunchKernelGGL((filter_kernel<8>), dim3(launch_grid(n, BLK / 8, 16384)), dim3(BLK), 0, 0, n, r, c, K, dSp, dSj, dB, dBf, dBt, dSx); break;
    case 16: hipLaunchKernelGGL((filter_kernel<16>), dim3(launch_grid(n, BLK / 16, 16384)), dim3(BLK), 0, 0, n, r, c, K, dSp, dSj, dB, dBf, dBt, dSx); break;
    case 32: hipLaunchKernelGGL((filter_kernel<32>), dim3(launch_grid(n, BLK / 32, 16384)), dim3(BLK), 0, 0, n, r, c, K, dSp, dSj, dB, dBf, dBt, dSx); break;
    default: hipLaunchKernelGGL((filter_kernel<64>), dim3(launch_grid(n, BLK / 64, 16384)), dim3(BLK), 0, 0, n, r, c, K, dSp, dSj, dB, dBf, dBt, dSx); break;
    }
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(Sx, dSx, (size_t)E));
    return PAMG_OK;
}

int pamg_scale_T_f64(int32_t n_brow, int32_t n_bcol, int32_t blocksize, const int32_t *Tp, int Tp_size, const int32_t *Tj, int Tj_size,
                     double *Tx, int64_t Tx_size, const int32_t *Cnodes, int Cnodes_size)
{
    const int n = n_brow, bs = blocksize;
    if (bs < 1 || n < 0 || n_bcol < 0 || Cnodes_size != n_bcol || (n_bcol && !Cnodes)) return PAMG_E_ARG;
    if (bs > rootnode::MAX_BLOCK) return PAMG_E_UNSUPPORTED;
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(n, n_bcol, Tp, Tp_size, Tj, Tj_size, &nnz));
    const int64_t E = nnz * bs * bs;
    if (E > Tx_size || (E && !Tx)) return PAMG_E_ARG;
    // a root row holds its aggregate's block and nothing else (T's non-overlapping block-diagonal structure): D is block diagonal
    std::vector<unsigned char> is_root((size_t)n, 0);
    for (int a = 0; a < n_bcol; ++a) {
        const int r = Cnodes[a];
        if (r < 0 || r >= n || is_root[r]) return PAMG_E_ARG;
        if (Tp[r + 1] - Tp[r] != 1 || Tj[Tp[r]] != a) return PAMG_E_UNSUPPORTED;
        is_root[r] = 1;
    }
    if (n == 0 || nnz == 0) return PAMG_OK;
    std::vector<int> row_of((size_t)nnz);
    for (int i = 0; i < n; ++i)
        for (int p = Tp[i]; p < Tp[i + 1]; ++p) row_of[p] = i;
    PAMG_TRY(have_device());
    Bufs d;
    int *dTp, *dTj, *dC, *drow;
    double *dTx, *dD, *dout;
    unsigned char *droot;
    PAMG_TRY(d.put(&dTp, Tp, (size_t)n + 1)); PAMG_TRY(d.put(&dTj, Tj, (size_t)nnz)); PAMG_TRY(d.put(&dTx, (const double *)Tx, (size_t)E));
    PAMG_TRY(d.put(&dC, Cnodes, (size_t)n_bcol)); PAMG_TRY(d.put(&drow, (const int *)row_of.data(), (size_t)nnz));
    PAMG_TRY(d.put(&droot, (const unsigned char *)is_root.data(), (size_t)n));
    PAMG_TRY(d.get(&dD, (size_t)n_bcol * bs * bs)); PAMG_TRY(d.get(&dout, (size_t)E));
    if (n_bcol)
        hipLaunchKernelGGL(root_blocks_kernel, dim3((unsigned)launch_grid(n_bcol, 64, INT32_MAX)), dim3(64), 0, 0, n_bcol, bs, dTp, dC, dTx,
                           rootnode::rank_tol_f64(), dD);
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)launch_grid(E, BLK, 65536)), dim3(BLK), 0, 0, E, bs, dTj, dTx, dD, droot, drow, dout);
    PAMG_HIP(hipGetLastError());
    PAMG_TRY(Bufs::fetch(Tx, dout, (size_t)E));
    return PAMG_OK;
}

}  // extern "C"
