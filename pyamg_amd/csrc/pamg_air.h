// pamg_air.h -- the per-row arithmetic of the approximate ideal restriction (AIR) setup, shared by the kernels of pamg_air.hip, the host
// path inside the library for the rows above the lane-group cap, and the host replay tests/air_emul.cpp (lanes as loops).
//
//   one_point_row     amg_core::one_point_interpolation (air.h:46-98) for one row
//   neighbourhood     the std::set of air.h:136-154 == :235-252: the strong F-neighbours of a C-point (and theirs, distance 2), ascending
//                     and unique.  approx_ideal_restriction_pass1 counts with it and pass2 fills with it, so they cannot disagree
//   gather_column /   the local system of air.h:270-309: the reference fills A0 row-major and hands it over as column-major, so column j
//   gather_rhs        of the system solved is row Nf[j] of A on the columns Nf, and b0[i] = -A[cpoint, Nf[i]]
//   qr_head / qr_col  least_squares (linalg.h:1442-1472): QR by Householder reflections (:1172-1263), rhs = Q^T b, upper_tri_solve
//   / qr_row /        (:1298-1337), operation for operation.  The update of column k of R touches column k only and the update of row i of Q
//   rhs_entry /       touches row i only: a lane owns one column of R and one row of Q and runs every sum serially in the reference's index
//   back_substitute   order; v, tau and the skip decision of step j come from the lane that owns column j (qr_head)
//   solve_serial      the same routines by one lane: the host path, and what the replay holds the lane groups against
//
// Storage: R(i, j) = R[j * ld + i] (column-major as in the reference, with a padded leading dimension), Q(i, k) = Q[k * ldq + i].
// With -ffp-contract=off and IEEE sqrt and division the results are the reference's bit for bit.
// PRECONDITION (as in pamg_classical.h): no row of A or C holds a column twice.  The searches keep the reference's rule -- the first stored
// entry -- and rows need not be sorted.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define PAMG_AIR_HD __host__ __device__ __forceinline__
#else
#define PAMG_AIR_HD inline
#endif

namespace pamg {
namespace air {

constexpr int F_NODE = 0, C_NODE = 1;                       // ruge_stuben.h:15-16
constexpr int NCLASS = 5;                                   // lane-group widths 8 / 16 / 32 / 64 by the neighbourhood size N, and the rows beyond 64 (host)
constexpr int MAX_STAGED = 64;
PAMG_AIR_HD int size_class(int n) { return n <= 8 ? 0 : n <= 16 ? 1 : n <= 32 ? 2 : n <= 64 ? 3 : 4; }
PAMG_AIR_HD double signof(double a) { return a < 0.0 ? -1.0 : 1.0; }            // linalg.h:20: zero counts as positive

// Row `row` of the one-point interpolation; map = exclusive scan of splitting.  pj == nullptr: count only.  Returns the entries of the row
// (0 or 1).  A C-row gets (map[row], 1.0): the reference writes the column only and leaves the value to its caller.
PAMG_AIR_HD int one_point_row(int row, const int *Cp, const int *Cj, const double *Cx, const int *splitting, const int *map, int *pj, double *px)
{
    if (splitting[row] == C_NODE) {
        if (pj) { *pj = map[row]; *px = 1.0; }
        return 1;
    }
    double mx = -1.0, val = 0.0;
    int ind = -1;
    for (int p = Cp[row]; p < Cp[row + 1]; ++p)
        if (splitting[Cj[p]] == C_NODE) {
            const double vv = std::fabs(Cx[p]);
            if (vv > mx) { mx = vv; ind = Cj[p]; val = Cx[p]; }                  // strict: the first stored entry wins a tie
        }
    if (ind < 0) return 0;
    if (pj) { *pj = map[ind]; *px = -val; }
    return 1;
}

// insert x into the ascending, unique buf[0, n); returns the new length, or -1 when buf is full
PAMG_AIR_HD int set_insert(int *buf, int n, int cap, int x)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (buf[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    if (lo < n && buf[lo] == x) return n;
    if (n >= cap) return -1;
    for (int t = n; t > lo; --t) buf[t] = buf[t - 1];
    buf[lo] = x;
    return n + 1;
}

// The neighbourhood of the C-point c into buf (ascending, unique); returns its size N, or -1 when it does not fit in cap entries.
// Any distance but 2 is distance 1, as in the reference.
PAMG_AIR_HD int neighbourhood(int c, const int *Cp, const int *Cj, const int *splitting, int distance, int *buf, int cap)
{
    int n = 0;
    for (int i = Cp[c]; i < Cp[c + 1]; ++i) {
        const int f = Cj[i];
        if (splitting[f] != F_NODE) continue;
        if ((n = set_insert(buf, n, cap, f)) < 0) return -1;
        if (distance == 2)
            for (int kk = Cp[f]; kk < Cp[f + 1]; ++kk)
                if (splitting[Cj[kk]] == F_NODE)
                    if ((n = set_insert(buf, n, cap, Cj[kk])) < 0) return -1;
    }
    return n;
}

// column j of the local system: R(i, j) = A[Nf[j], Nf[i]], the first stored match, +0.0 when absent
PAMG_AIR_HD void gather_column(int j, int N, const int *Nf, const int *Ap, const int *Aj, const double *Ax, double *R, int ld)
{
    const int r0 = Ap[Nf[j]], r1 = Ap[Nf[j] + 1];
    for (int i = 0; i < N; ++i) {
        const int col = Nf[i];
        double a = 0.0;
        for (int k = r0; k < r1; ++k)
            if (Aj[k] == col) { a = Ax[k]; break; }
        R[j * ld + i] = a;
    }
}

// b0[i] = -A[cpoint, Nf[i]], the first stored match, +0.0 when absent
PAMG_AIR_HD double gather_rhs(int i, const int *Nf, const int *Ap, const int *Aj, const double *Ax, int cpoint)
{
    for (int k = Ap[cpoint]; k < Ap[cpoint + 1]; ++k)
        if (Aj[k] == Nf[i]) return -Ax[k];
    return 0.0;
}

// row i of Q := identity
PAMG_AIR_HD void q_identity_row(int i, int N, double *Q, int ldq)
{
    for (int k = 0; k < N; ++k) Q[k * ldq + i] = k == i ? 1.0 : 0.0;
}

// Step j of QR, by the lane that owns column j: the reflector v[0, N - j) and tau.  false: the column is skipped (normx < 1e-12)
PAMG_AIR_HD bool qr_head(int j, int N, const double *R, int ld, double *v, double *tau)
{
    double normx = 0.0;
    for (int i = j; i < N; ++i) {
        const double t = R[j * ld + i];
        normx += t * t;
    }
    normx = std::sqrt(normx);
    if (normx < 1e-12) return false;
    normx *= -1 * signof(R[j * ld + j]);
    const double scale = R[j * ld + j] - normx;
    *tau = -scale / normx;
    v[0] = 1.0;
    for (int i = 1; i < N - j; ++i) v[i] = R[j * ld + j + i] / scale;
    return true;
}

// R := H R on column k (k >= j)
PAMG_AIR_HD void qr_col(int j, int k, int N, double *R, int ld, const double *v, double tau)
{
    double vtR = 0.0;
    for (int i = 0; i < N - j; ++i) vtR += v[i] * R[k * ld + j + i];
    for (int i = 0; i < N - j; ++i) R[k * ld + j + i] -= tau * v[i] * vtR;
}

// Q := Q H on row i
PAMG_AIR_HD void qr_row(int j, int i, int N, double *Q, int ldq, const double *v, double tau)
{
    double Qv = 0.0;
    for (int k = 0; k < N - j; ++k) Qv += v[k] * Q[(k + j) * ldq + i];
    for (int k = 0; k < N - j; ++k) Q[(k + j) * ldq + i] -= tau * v[k] * Qv;
}

// rhs[i] = sum_k b[k] Q(k, i), ascending k
PAMG_AIR_HD double rhs_entry(int i, int N, const double *b, const double *Q, int ldq)
{
    double s = 0.0;
    for (int k = 0; k < N; ++k) s += b[k] * Q[i * ldq + k];
    return s;
}

// upper_tri_solve: x_i = 0 where |R_ii| < 1e-12
PAMG_AIR_HD void back_substitute(int N, const double *R, int ld, const double *rhs, double *x)
{
    for (int i = N - 1; i >= 0; --i) {
        double temp = rhs[i];
        for (int j = i + 1; j < N; ++j) temp -= R[j * ld + i] * x[j];
        if (std::fabs(R[i * ld + i]) < 1e-12) x[i] = 0.0;
        else x[i] = temp / R[i * ld + i];
    }
}

// The local solve of one C-row by one lane: R [N * ld], Q [N * ldq], v / b / rhs [N] are work space, x [N] receives the row of R
PAMG_AIR_HD void solve_serial(int N, const int *Nf, int cpoint, const int *Ap, const int *Aj, const double *Ax, double *R, int ld, double *Q, int ldq,
                              double *v, double *b, double *rhs, double *x)
{
    for (int j = 0; j < N; ++j) {
        gather_column(j, N, Nf, Ap, Aj, Ax, R, ld);
        b[j] = gather_rhs(j, Nf, Ap, Aj, Ax, cpoint);
        q_identity_row(j, N, Q, ldq);
    }
    for (int j = 0; j < N; ++j) {
        double tau = 0.0;
        if (!qr_head(j, N, R, ld, v, &tau)) continue;
        for (int k = j; k < N; ++k) qr_col(j, k, N, R, ld, v, tau);
        for (int i = 0; i < N; ++i) qr_row(j, i, N, Q, ldq, v, tau);
    }
    for (int i = 0; i < N; ++i) rhs[i] = rhs_entry(i, N, b, Q, ldq);
    back_substitute(N, R, ld, rhs, x);
}

}  // namespace air
}  // namespace pamg
