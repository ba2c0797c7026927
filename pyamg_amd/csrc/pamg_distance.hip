// pamg_distance.hip -- the relaxation-vector strength measures (algebraic distance, affinity; strength.py:860-1072) and the vertex-distance
// measure (strength.py:24-111) on the device.  The per-row / per-entry arithmetic is pamg_distance.h (replayed on the host by
// tests/distance_emul.cpp); every result is the reference's, bit for bit.
//
//   relaxation   the block of R random vectors is kept interleaved, one record of R doubles per node (transposed from the reference's
//                column-major block on upload, and back on download).  One plain launch per sweep, between two alternating buffers; a
//                thread owns one (row, column) pair, t = row * R + column, and walks the row in stored order.  The R lanes of a row read
//                the same Aj / Ax words (one request per wave) and one contiguous record per stored entry, so A is read once per sweep
//                for all R columns; the store is coalesced.  Rows of any length
//   measure      a group of 16 lanes per row (8 where the rows hold seven entries or fewer on average), a lane owns the entries p,
//                p + 16, ... ; with the tail fused, the lanes then reduce the
//                minimum of the row's non-zero off-diagonal distances over the group (the minimum of numbers does not depend on the
//                order) and zero what lies at or above epsilon times it
//   vertex       the same mapping, one expression per stored entry
//
// Plain launches only; no lane of any kernel waits for another.
#include "pamg_common.h"
#include "pamg_distance.h"
#include "pamg_host_call.h"

using namespace pamg;

namespace {

constexpr int GW = 16;                      // lanes per row of the entry-parallel kernels
constexpr int GN = 8, GN_ROW = 7;           // ... of the measure kernel where the rows hold seven entries or fewer on average (5- and 7-point stencils)

int dgrid(int64_t n, int per_block) { return launch_grid(n, per_block, 16384); }

// ------------------------------------------------------------------------------------------------ kernels
// column-major [R][n] <-> one record of R per node [n][R]
template <bool TO_RECORDS>
__global__ __launch_bounds__(BLK) void records_kernel(int n, int R, const double *__restrict__ src, double *__restrict__ dst)
{
    const int64_t total = (int64_t)n * R;
    for (int64_t t = (int64_t)blockIdx.x * BLK + threadIdx.x; t < total; t += (int64_t)gridDim.x * BLK) {
        const int64_t i = t / R, r = t - i * R;
        if (TO_RECORDS) dst[t] = src[r * n + i];
        else dst[r * n + i] = src[t];
    }
}

__global__ __launch_bounds__(BLK) void relax_kernel(int n, int R, const int *__restrict__ Ap, const int *__restrict__ Aj, const double *__restrict__ Ax,
                                                    const double *__restrict__ old, double *__restrict__ out, double omega)
{
    const int64_t total = (int64_t)n * R;
    for (int64_t t = (int64_t)blockIdx.x * BLK + threadIdx.x; t < total; t += (int64_t)gridDim.x * BLK) {
        const int i = (int)(t / R), r = (int)(t - (int64_t)i * R);
        out[t] = dst::relax_value(i, r, R, Ap, Aj, Ax, old, omega);
    }
}

template <bool FILTER, int G>
__global__ __launch_bounds__(BLK) void measure_kernel(int measure, int n, int R, double epsilon, const int *__restrict__ Ap, const int *__restrict__ Aj,
                                                      const double *__restrict__ Ax, const double *__restrict__ X, double *Dx)
{
    const int lane = threadIdx.x % G;
    for (int64_t row = ((int64_t)blockIdx.x * BLK + threadIdx.x) / G; row < n; row += (int64_t)gridDim.x * (BLK / G)) {
        const int p0 = Ap[row] + lane, r1 = Ap[row + 1];
        for (int p = p0; p < r1; p += G) Dx[p] = dst::measure_entry(measure, R, (int)row, Aj[p], Ax[p], X);
        if (FILTER) {
            double mn = dst::row_min((int)row, p0, r1, G, Aj, Dx);           // (the lane's own entries: written above by itself)
            for (int m = G / 2; m; m >>= 1) mn = dst::dmin(mn, __shfl_xor(mn, m, G));
            const double threshold = epsilon * mn;
            for (int p = p0; p < r1; p += G) Dx[p] = dst::tail(Dx[p], threshold);
        }
    }
}

__global__ __launch_bounds__(BLK) void vertex_kernel(int n, int dim, const int *__restrict__ Ap, const int *__restrict__ Aj, const double *__restrict__ V,
                                                     double *__restrict__ Cx)
{
    const int lane = threadIdx.x % GW;
    for (int64_t row = ((int64_t)blockIdx.x * BLK + threadIdx.x) / GW; row < n; row += (int64_t)gridDim.x * (BLK / GW)) {
        const int r1 = Ap[row + 1];
        for (int p = Ap[row] + lane; p < r1; p += GW) Cx[p] = dst::vertex_entry((int)row, Aj[p], dim, V);
    }
}

bool known_measure(int m) { return m == dst::ALGEBRAIC_P1 || m == dst::ALGEBRAIC_P2 || m == dst::ALGEBRAIC_PINF || m == dst::AFFINITY; }

// what the three relaxation-vector entries check before anything is touched
int check_block(const int *Ap, int Ap_size, const int *Aj, int Aj_size, const double *Ax, int Ax_size, const double *X, int X_size, int n, int R,
                int64_t *nnz)
{
    PAMG_TRY(check_pattern(n, n, Ap, Ap_size, Aj, Aj_size, nnz, true, Ax, Ax_size));
    if (R < 1 || X_size < 0) return PAMG_E_ARG;
    if (R > dst::MAX_R) return PAMG_E_UNSUPPORTED;
    if ((int64_t)n * R > X_size || (n && !X)) return PAMG_E_ARG;
    return PAMG_OK;
}

// A and the column-major block up; the block as records in *dXa, a second buffer of its size in *dXb (where asked for), the raw copy in *dRaw
int upload(Bufs &d, const int *Ap, const int *Aj, const double *Ax, const double *X, int n, int R, int64_t nnz, int **dAp, int **dAj, double **dAx,
           double **dRaw, double **dXa, double **dXb)
{
    const size_t nR = (size_t)n * R;
    PAMG_TRY(d.put(dAp, Ap, (size_t)n + 1)); PAMG_TRY(d.put(dAj, Aj, (size_t)nnz)); PAMG_TRY(d.put(dAx, Ax, (size_t)nnz));
    PAMG_TRY(d.put(dRaw, X, nR)); PAMG_TRY(d.get(dXa, nR));
    if (dXb) PAMG_TRY(d.get(dXb, nR));
    hipLaunchKernelGGL((records_kernel<true>), dim3(dgrid((int64_t)nR, BLK)), dim3(BLK), 0, 0, n, R, *dRaw, *dXa);
    PAMG_HIP(hipGetLastError());
    return PAMG_OK;
}

int download_block(double *X, const double *dX, double *dRaw, int n, int R)
{
    const size_t nR = (size_t)n * R;
    hipLaunchKernelGGL((records_kernel<false>), dim3(dgrid((int64_t)nR, BLK)), dim3(BLK), 0, 0, n, R, dX, dRaw);
    PAMG_HIP(hipGetLastError());
    return Bufs::fetch(X, (const double *)dRaw, nR);
}

}  // namespace

extern "C" {

int pamg_dev_relaxation_sweeps_f64(int32_t n, int32_t R, int32_t k, double omega, const int32_t *dAp, const int32_t *dAj, const double *dAx,
                                   double *dXa, double *dXb, void *stream)
{
    if (n < 0 || R < 1 || k < 0) return PAMG_E_ARG;
    if (R > dst::MAX_R) return PAMG_E_UNSUPPORTED;
    if (n == 0) return PAMG_OK;
    if (!dAp || !dAj || !dAx || !dXa || !dXb) return PAMG_E_ARG;
    double *from = dXa, *to = dXb;
    for (int s = 0; s < k; ++s) {
        hipLaunchKernelGGL(relax_kernel, dim3(dgrid((int64_t)n * R, BLK)), dim3(BLK), 0, (hipStream_t)stream, n, R, dAp, dAj, dAx, from, to, omega);
        std::swap(from, to);
    }
    PAMG_HIP(hipGetLastError());
    return PAMG_OK;
}

int pamg_dev_distance_measure_f64(int32_t measure, int32_t filter, int32_t n, int64_t nnz, int32_t R, double epsilon, const int32_t *dAp,
                                  const int32_t *dAj, const double *dAx, const double *dX, double *dDx, void *stream)
{
    if (n < 0 || nnz < 0 || R < 1 || !known_measure(measure)) return PAMG_E_ARG;
    if (R > dst::MAX_R) return PAMG_E_UNSUPPORTED;
    if (n == 0) return PAMG_OK;
    if (!dAp || !dAj || !dAx || !dX || !dDx) return PAMG_E_ARG;
    const bool narrow = nnz <= (int64_t)GN_ROW * n;
    auto launch = [&](auto kernel, int g) {
        hipLaunchKernelGGL(kernel, dim3(dgrid(n, BLK / g)), dim3(BLK), 0, (hipStream_t)stream, measure, n, R, epsilon, dAp, dAj, dAx, dX, dDx);
    };
    if (filter && narrow) launch(measure_kernel<true, GN>, GN);
    else if (filter) launch(measure_kernel<true, GW>, GW);
    else if (narrow) launch(measure_kernel<false, GN>, GN);
    else launch(measure_kernel<false, GW>, GW);
    PAMG_HIP(hipGetLastError());
    return PAMG_OK;
}

int pamg_relaxation_vectors_f64(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const double *Ax, int Ax_size, double *X, int X_size,
                                int32_t n, int32_t R, int32_t k, double omega)
{
    int64_t nnz = 0;
    PAMG_TRY(check_block(Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, X, X_size, n, R, &nnz));
    if (k < 0) return PAMG_E_ARG;
    if (n == 0 || k == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dAp, *dAj;
    double *dAx, *dRaw, *dXa, *dXb;
    PAMG_TRY(upload(d, Ap, Aj, Ax, X, n, R, nnz, &dAp, &dAj, &dAx, &dRaw, &dXa, &dXb));
    PAMG_TRY(pamg_dev_relaxation_sweeps_f64(n, R, k, omega, dAp, dAj, dAx, dXa, dXb, nullptr));
    return download_block(X, k % 2 ? dXb : dXa, dRaw, n, R);
}

int pamg_distance_measure_f64(int32_t measure, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const double *Ax, int Ax_size,
                              const double *X, int X_size, int32_t n, int32_t R, double *Dx, int Dx_size)
{
    int64_t nnz = 0;
    PAMG_TRY(check_block(Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, X, X_size, n, R, &nnz));
    if (!known_measure(measure) || nnz > Dx_size || (nnz && !Dx)) return PAMG_E_ARG;
    if (n == 0 || nnz == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dAp, *dAj;
    double *dAx, *dRaw, *dXa, *dDx;
    PAMG_TRY(upload(d, Ap, Aj, Ax, X, n, R, nnz, &dAp, &dAj, &dAx, &dRaw, &dXa, nullptr));
    PAMG_TRY(d.get(&dDx, (size_t)nnz));
    PAMG_TRY(pamg_dev_distance_measure_f64(measure, 0, n, nnz, R, 0.0, dAp, dAj, dAx, dXa, dDx, nullptr));
    return Bufs::fetch(Dx, (const double *)dDx, (size_t)nnz);
}

int pamg_distance_strength_f64(int32_t measure, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const double *Ax, int Ax_size,
                               double *X, int X_size, int32_t n, int32_t R, int32_t k, double omega, double epsilon, double *Dx, int Dx_size)
{
    int64_t nnz = 0;
    PAMG_TRY(check_block(Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, X, X_size, n, R, &nnz));
    if (k < 0 || !known_measure(measure) || nnz > Dx_size || (nnz && !Dx)) return PAMG_E_ARG;
    if (n == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dAp, *dAj;
    double *dAx, *dRaw, *dXa, *dXb, *dDx;
    PAMG_TRY(upload(d, Ap, Aj, Ax, X, n, R, nnz, &dAp, &dAj, &dAx, &dRaw, &dXa, &dXb));
    PAMG_TRY(d.get(&dDx, (size_t)nnz));
    PAMG_TRY(pamg_dev_relaxation_sweeps_f64(n, R, k, omega, dAp, dAj, dAx, dXa, dXb, nullptr));
    double *dX = k % 2 ? dXb : dXa;
    PAMG_TRY(pamg_dev_distance_measure_f64(measure, 1, n, nnz, R, epsilon, dAp, dAj, dAx, dX, dDx, nullptr));
    PAMG_TRY(Bufs::fetch(Dx, (const double *)dDx, (size_t)nnz));
    return download_block(X, dX, dRaw, n, R);
}

int pamg_vertex_distance_f64(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const double *V, int V_size, int32_t n, int32_t dim,
                             double *Cx, int Cx_size)
{
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(n, n, Ap, Ap_size, Aj, Aj_size, &nnz));
    if (dim < 1 || V_size < 0 || nnz > Cx_size || (nnz && !Cx)) return PAMG_E_ARG;
    if (dim > dst::MAX_DIM) return PAMG_E_UNSUPPORTED;
    if ((int64_t)n * dim > V_size || (n && !V)) return PAMG_E_ARG;
    if (n == 0 || nnz == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dAp, *dAj;
    double *dV, *dCx;
    PAMG_TRY(d.put(&dAp, Ap, (size_t)n + 1)); PAMG_TRY(d.put(&dAj, Aj, (size_t)nnz));
    PAMG_TRY(d.put(&dV, V, (size_t)n * dim)); PAMG_TRY(d.get(&dCx, (size_t)nnz));
    hipLaunchKernelGGL(vertex_kernel, dim3(dgrid(n, BLK / GW)), dim3(BLK), 0, 0, n, dim, dAp, dAj, dV, dCx);
    PAMG_HIP(hipGetLastError());
    return Bufs::fetch(Cx, (const double *)dCx, (size_t)nnz);
}

}  // extern "C"
