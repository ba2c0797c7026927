// pamg_air_block.h -- the per-row arithmetic of the BLOCK (BSR) approximate ideal restriction setup, shared by the kernels of
// pamg_air_block.hip, the host path inside the library for the systems above the lane-group cap, and the host replay
// tests/block_air_emul.cpp (lanes as loops).  Blocks are square, b x b with b = 1 .. 8, row-major as BSR stores them.  The neighbourhood
// and the Householder least squares are pamg_air.h's, unchanged: pass 1 works on the block pattern as it is.
//
//   measure           strength.py:200-214: one value per stored block -- 'abs' the largest |a|, 'min' the smallest a, 'fro' the sum of
//                     a * a taken down the rows of every column first and then across the columns, left to right (NumPy's order for
//                     b <= 7; b == 8 is refused, there NumPy sums with eight accumulators) -- and anything below 1e-16 in magnitude as +0.0
//   gather_column     the local system of air.h:432-486, of order n = N * b: the reference fills A0 row-major and hands it over as
//                     column-major, so column (jb * b + r) of the system solved is row r of block row Nf[jb] of A on the columns
//                     Nf[.] * b + c: R(ib * b + c, jb * b + r) = A[Nf[jb], Nf[ib]][r][c], the first stored match, +0.0 when absent
//   gather_rhs        the b right-hand sides of air.h:499-517: b0[r * n + ib * b + c] = -A[cpoint, Nf[ib]][r][c]
//   store_solution    air.h:559-575: block ib, entry (r, c) of the row of R is x_r[ib * b + c] where |x| > 1e-15 and +0.0 otherwise
//   identity_block    air.h:577-582
//   solve_serial      one factorisation, then per right-hand side rhs = Q^T b (the sum over k ascending from 0.0) and upper_tri_solve, by
//                     one lane: the host path, and what the replay holds the lane groups against
//
// A lane owns one column of R and one row of Q, as in pamg_air.h; the b back substitutions are independent and go to b lanes.
#pragma once
#include "pamg_air.h"

namespace pamg {
namespace air_block {

constexpr int MAX_B = 8;
constexpr int NORM_ABS = 0, NORM_MIN = 1, NORM_FRO = 2;
constexpr int MAX_DOFS = 64;                                // systems of order n = N * b beyond this are solved on the host

PAMG_AIR_HD double measure(int norm, int b, const double *blk)
{
    double m;
    if (norm == NORM_ABS) {
        m = 0.0;
        for (int e = 0; e < b * b; ++e) { const double a = std::fabs(blk[e]); if (a > m) m = a; }
    } else if (norm == NORM_MIN) {
        m = blk[0];
        for (int e = 1; e < b * b; ++e) if (blk[e] < m) m = blk[e];
    } else {
        m = 0.0;
        for (int c = 0; c < b; ++c) {
            double s = 0.0;
            for (int r = 0; r < b; ++r) s += blk[r * b + c] * blk[r * b + c];
            m += s;
        }
    }
    return std::fabs(m) < 1e-16 ? 0.0 : m;
}

// column k = jb * b + r of the local system
PAMG_AIR_HD void gather_column(int k, int N, int b, const int *Nf, const int *Ap, const int *Aj, const double *Ax, double *R, int ld)
{
    const int jb = k / b, r = k % b;
    const int r0 = Ap[Nf[jb]], r1 = Ap[Nf[jb] + 1];
    for (int ib = 0; ib < N; ++ib) {
        const int col = Nf[ib];
        const double *blk = nullptr;
        for (int p = r0; p < r1; ++p)
            if (Aj[p] == col) { blk = Ax + (size_t)p * b * b; break; }
        for (int c = 0; c < b; ++c) R[k * ld + ib * b + c] = blk ? blk[r * b + c] : 0.0;
    }
}

// entry k = ib * b + c of every right-hand side: b0[r * n + k], r = 0 .. b - 1
PAMG_AIR_HD void gather_rhs(int k, int n, int b, const int *Nf, const int *Ap, const int *Aj, const double *Ax, int cpoint, double *b0)
{
    const int ib = k / b, c = k % b;
    const double *blk = nullptr;
    for (int p = Ap[cpoint]; p < Ap[cpoint + 1]; ++p)
        if (Aj[p] == Nf[ib]) { blk = Ax + (size_t)p * b * b; break; }
    for (int r = 0; r < b; ++r) b0[r * n + k] = blk ? -blk[r * b + c] : 0.0;
}

// entry k = ib * b + c of every solution x_r = xs[r * n + .] into the blocks of the row of R that start at Rx
PAMG_AIR_HD void store_solution(int k, int n, int b, const double *xs, double *Rx)
{
    const int ib = k / b, c = k % b;
    for (int r = 0; r < b; ++r) {
        const double x = xs[r * n + k];
        Rx[(size_t)ib * b * b + r * b + c] = std::fabs(x) > 1e-15 ? x : 0.0;
    }
}

PAMG_AIR_HD void identity_block(int b, double *blk)
{
    for (int e = 0; e < b * b; ++e) blk[e] = e % (b + 1) == 0 ? 1.0 : 0.0;
}

// The local solve of one C-row by one lane: R [n * ld], Q [n * ldq], v / rhs [n] and b0 [b * n] are work space (n = N * b); Rx receives
// the N solution blocks
PAMG_AIR_HD void solve_serial(int N, int b, const int *Nf, int cpoint, const int *Ap, const int *Aj, const double *Ax, double *R, int ld, double *Q,
                              int ldq, double *v, double *b0, double *rhs, double *Rx)
{
    const int n = N * b;
    for (int k = 0; k < n; ++k) {
        gather_column(k, N, b, Nf, Ap, Aj, Ax, R, ld);
        gather_rhs(k, n, b, Nf, Ap, Aj, Ax, cpoint, b0);
        air::q_identity_row(k, n, Q, ldq);
    }
    for (int j = 0; j < n; ++j) {
        double tau = 0.0;
        if (!air::qr_head(j, n, R, ld, v, &tau)) continue;
        for (int k = j; k < n; ++k) air::qr_col(j, k, n, R, ld, v, tau);
        for (int i = 0; i < n; ++i) air::qr_row(j, i, n, Q, ldq, v, tau);
    }
    for (int r = 0; r < b; ++r) {
        for (int i = 0; i < n; ++i) rhs[i] = air::rhs_entry(i, n, b0 + r * n, Q, ldq);
        air::back_substitute(n, R, ld, rhs, b0 + r * n);    // the solution replaces its right-hand side, as in the reference
    }
    for (int k = 0; k < n; ++k) store_solution(k, n, b, b0, Rx);
}

}  // namespace air_block
}  // namespace pamg
