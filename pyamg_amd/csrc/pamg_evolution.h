// pamg_evolution.h -- the per-row / per-entry arithmetic of the evolution strength measure, shared by the kernels of pamg_evolution.hip
// and the host replay tests/evolution_emul.cpp (lanes and groups as loops), as pamg_classical.h is shared by the classical setup.
//
//   inner              my_inner (evolution_strength.h:586-616): <A[row, :], B[:, col]> by the two-pointer merge, ascending, from 0.0
//   helper_row<K1>     one row of evolution_strength_helper (:368-539, real T): LHS / RHS as :417-468 build them, svd_solve
//                      (linalg.h:837-882) through JacobiSvd, zhat, the numerical-zero filter and the classification of :503-534.
//                      z, zhat, Bi and DBi are not stored: they are re-gathered from Sx, B and DB in the same order, so a row may be
//                      of any length.  Sx[jj] is read before it is written, and zhat does not depend on Sx once RHS is solved
//   distance_row       one row of apply_distance_filter / apply_absolute_distance_filter (:62-172)
//   block_min          one block of min_blocks (:220-245)
//   vector_entry       one stored entry of the one-candidate shortcut (strength.py:738-779), each rounding where NumPy's elementwise
//                      steps put it
//
// Every sum runs serially in the reference's order, so with -ffp-contract=off the results are the reference's bit for bit.
#pragma once
#include <cmath>

#include "pamg_jacobi_svd.h"

#if defined(__HIPCC__)
#define PAMG_EVO_HD __host__ __device__
#else
#define PAMG_EVO_HD inline
#endif

namespace pamg {
namespace evo {

constexpr int MAX_NULLDIM = 6;                              // K + 1 <= 7: scalar problems, 2-D (3) and 3-D (6) elasticity
constexpr double DMAX = 1.7976931348623157e308;             // numeric_limits<double>::max()
constexpr double DEPS = 2.220446049250313e-16;              // numeric_limits<double>::epsilon()

// std::min / std::max: the running value a is replaced only when the comparison holds, so a NaN operand never replaces it
PAMG_EVO_HD double dmin(double a, double b) { return b < a ? b : a; }
PAMG_EVO_HD double dmax(double a, double b) { return a < b ? b : a; }

PAMG_EVO_HD double inner(const int *Ap, const int *Aj, const double *Ax, const int *Bp, const int *Bj, const double *Bx, int row, int col)
{
    double sum = 0.0;
    int a = Ap[row], b = Bp[col];
    const int a1 = Ap[row + 1], b1 = Bp[col + 1];
    while (a < a1 && b < b1) {
        const int ja = Aj[a], jb = Bj[b];
        if (ja == jb) {
            sum += Ax[a] * Bx[b];
            ++a;
            ++b;
        } else if (ja < jb) ++a;
        else ++b;
    }
    return sum;
}

// zhat of the stored entry jj: row Sj[jj] of B (row-major, NullDim wide) times the solved RHS, k ascending from zero
PAMG_EVO_HD double zhat_at(int j, int NullDim, const double *B, const double *RHS)
{
    double s = 0.0;
    for (int k = 0; k < NullDim; ++k) s += B[(long long)j * NullDim + k] * RHS[k];
    return s;
}

// Row i of evolution_strength_helper; K1 = NullDim + 1.  B [nrows * NullDim] row-major, DB [NullDim * nrows] (one candidate after the
// other), BDB [nrows * BDBCols] row-major.
template <int K1>
PAMG_EVO_HD void helper_row(int i, double *Sx, const int *Sp, const int *Sj, int nrows, const double *B, const double *DB, const double *BDB,
                            double tol)
{
    constexpr int NullDim = K1 - 1, BDBCols = NullDim * (NullDim + 1) / 2;
    const int r0 = Sp[i], r1 = Sp[i + 1];
    if (r1 - r0 <= NullDim) {                                // B reproduces the row exactly: every connection is strong (:374-380)
        for (int p = r0; p < r1; ++p) Sx[p] = 1.0;
        return;
    }
    double LHS[K1 * K1], RHS[K1], x[K1];
    for (int q = 0; q < K1 * K1; ++q) LHS[q] = 0.0;
    double z_at_i = 1.0;
    for (int p = r0; p < r1; ++p) {                          // :421-448
        const int j = Sj[p];
        if (j == i) z_at_i = Sx[p];
        const double *bdb = BDB + (long long)j * BDBCols;
        int c = 0;
        for (int m = 0; m < NullDim; ++m) {
            LHS[m * (K1 + 1)] += bdb[c];
            c += NullDim - m;
        }
        c = 0;
        for (int m = 0; m < NullDim; ++m) {
            int counter = 1;
            for (int n = m + 1; n < NullDim; ++n) {
                const double e = bdb[c + counter];
                LHS[m * K1 + n] = LHS[m * K1 + n] + e;
                LHS[n * K1 + m] = LHS[n * K1 + m] + e;
                ++counter;
            }
            c += NullDim - m;
        }
    }
    for (int m = 0; m < NullDim; ++m) LHS[m * K1 + NullDim] = B[(long long)i * NullDim + m];      // the last row, e_i^T B (:451-452)
    for (int m = 0; m < NullDim; ++m) LHS[NullDim * K1 + m] = DB[(long long)m * nrows + i];        // the last column (:455-456)
    for (int k = 0; k < NullDim; ++k) {                      // Bi^H D_A z, jj ascending from zero, then doubled (:460-466)
        double s = 0.0;
        const double *dbk = DB + (long long)k * nrows;
        for (int p = r0; p < r1; ++p) s += dbk[Sj[p]] * Sx[p];
        RHS[k] = s * 2.0;
    }
    RHS[NullDim] = z_at_i;
    // svd_solve (linalg.h:837-882): x = U^H b, scaled by the non-zero singular values, b = V x
    JacobiSvd<double, K1> sv;
    sv.n = K1;
    sv.run(LHS);
    for (int r = 0; r < K1; ++r) {
        double s = 0.0;
        for (int k = 0; k < K1; ++k) s += sv.U[r * K1 + k] * RHS[k];
        x[r] = s;
    }
    for (int r = 0; r < K1; ++r) x[r] = sv.S[r] != 0.0 ? x[r] / sv.S[r] : 0.0;
    for (int r = 0; r < K1; ++r) {
        double s = 0.0;
        for (int k = 0; k < K1; ++k) s += sv.V[k * K1 + r] * x[k];
        RHS[r] = s;
    }
    double max_zhat = 0.0;                                   // :483-490
    for (int p = r0; p < r1; ++p) {
        const double nz = std::fabs(zhat_at(Sj[p], NullDim, B, RHS));
        if (nz > max_zhat) max_zhat = nz;
    }
    const double tol_i = tol * max_zhat;
    const double sqrt_near_zero = std::sqrt(DEPS);
    for (int p = r0; p < r1; ++p) {                          // :491-537
        const int j = Sj[p];
        if (j == i) { Sx[p] = 1.0; continue; }
        double zh = zhat_at(j, NullDim, B, RHS);
        if (std::fabs(zh) < tol_i) zh = 0.0;
        const double z = Sx[p];
        const double ratio = zh / z;
        const double dprod = zh * z + 0.0 * 0.0;
        if (ratio * ratio <= 1e-8) Sx[p] = 0.0;
        else if (dprod < 0.0) Sx[p] = 0.0;
        else {
            const double error = std::fabs(-ratio + 1.0);
            Sx[p] = error < sqrt_near_zero ? 1e-4 : error;
        }
    }
}

// Row i of apply_distance_filter (RELATIVE: the threshold is epsilon times the smallest off-diagonal entry) or of
// apply_absolute_distance_filter (the threshold is epsilon)
template <bool RELATIVE>
PAMG_EVO_HD void distance_row(int i, double epsilon, const int *Sp, const int *Sj, double *Sx)
{
    const int r0 = Sp[i], r1 = Sp[i + 1];
    double threshold = epsilon;
    if (RELATIVE) {
        double mn = DMAX;
        for (int p = r0; p < r1; ++p) if (Sj[p] != i) mn = dmin(mn, Sx[p]);
        threshold = epsilon * mn;
    }
    for (int p = r0; p < r1; ++p) {
        if (Sj[p] == i) Sx[p] = 1.0;
        else if (Sx[p] >= threshold) Sx[p] = 0.0;
    }
}

PAMG_EVO_HD double block_min(const double *block, int blocksize)
{
    double mn = DMAX;
    for (int q = 0; q < blocksize; ++q) {
        const double v = block[q];
        if (v != 0.0) mn = dmin(mn, v);
    }
    return mn;
}

// The stored entry a = Atilde(i, j) of the one-candidate shortcut: di = Atilde(i, i), bi / bj the candidate with its zeros made ones
PAMG_EVO_HD double vector_entry(double a, double di, double bi, double bj)
{
    const double t = (di / bi) * bj;                        // scale_rows of ones by d / b (1.0 * v is exact), then scale_columns by b
    const bool angle = (t * a + 0.0 * 0.0) < 0.0;
    const double r = t / a;
    const bool weak = std::fabs(r) < 1e-4;
    const double e = std::fabs(1.0 - r);
    return (weak || angle) ? 0.0 : e;
}

}  // namespace evo
}  // namespace pamg
