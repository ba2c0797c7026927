// pamg_classical.h -- the per-row arithmetic of the classical (Ruge-Stuben) AMG setup, shared by the kernels of pamg_classical.hip
// and the host replay tests/classical_emul.cpp (lanes as loops), as pamg_dense_pinv.h is shared by the Schwarz setup.
//
//   strength_row      amg_core::classical_strength_of_connection_abs / _min (ruge_stuben.h:64-204) followed by what strength.py:237-240
//                     does to the result: magnitudes, the row scaled by the reciprocal of its largest entry, exact zeros dropped
//   mis_node          one synchronous round of amg_core::maximal_independent_set_parallel (graph.h:140-203) for one node
//   interp_count_row  rs_direct_interpolation_pass1 == rs_classical_interpolation_pass1 (ruge_stuben.h:777-796, :1083-1103)
//   direct_row        rs_direct_interpolation_pass2 (:832-907)
//   remove_ff_row     remove_strong_FF_connections (:1133-1181)
//   classical_*       rs_classical_interpolation_pass2 (:1239-1383), split so that the inner denominator, which depends on (i, k) only, is
//                     computed once per strong F-neighbour k and not once per (j, k) pair
//
// Every sum runs serially in stored order, so with -ffp-contract=off the results are the reference's bit for bit.
// PRECONDITION of the interpolation routines: no row of A or S holds a column twice.  The searches keep the reference's rule (first
// stored entry, or the last one in the modified search for a_kj and a_kk), but with a duplicated column the reference's a_kk would
// depend on j and the inner denominator could not be shared.  Rows need not be sorted.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define PAMG_CLS_HD __host__ __device__ __forceinline__
#else
#define PAMG_CLS_HD inline
#endif

namespace pamg {
namespace cls {

constexpr int F_NODE = 0, C_NODE = 1;                       // ruge_stuben.h:15-16
constexpr double DMIN = 2.2250738585072014e-308;            // numeric_limits<double>::min()
constexpr int NCLASS = 5;                                   // lane-group widths 8 / 16 / 32 / 64 by the row's strong-entry count, and the rows beyond 64
constexpr int MAX_STAGED = 64;
PAMG_CLS_HD int size_class(int n) { return n <= 8 ? 0 : n <= 16 ? 1 : n <= 32 ? 2 : n <= 64 ? 3 : 4; }
// what a strong entry (i, col) is to an F-row i
enum : unsigned char { K_NONE = 0, K_C = 1, K_F = 2 };

PAMG_CLS_HD double signof(double a) { return a < 0.0 ? -1.0 : 1.0; }            // linalg.h:20: zero counts as positive
PAMG_CLS_HD double dmax(double a, double b) { return a < b ? b : a; }           // std::max

// Row i of the strength matrix.  Sj == nullptr: count only.  Returns the number of entries the row keeps.
template <bool MIN>
PAMG_CLS_HD int strength_row(int i, double theta, const int *Ap, const int *Aj, const double *Ax, int *Sj, double *Sx)
{
    const int r0 = Ap[i], r1 = Ap[i + 1];
    double mx = MIN ? 0.0 : DMIN;
    for (int p = r0; p < r1; ++p)
        if (Aj[p] != i) mx = dmax(mx, MIN ? -Ax[p] : std::fabs(Ax[p]));
    const double threshold = theta * mx;
    double big = DMIN;                                      // maximum_row_value (ruge_stuben.h:238) over the entries that were kept
    for (int p = r0; p < r1; ++p)
        if (Aj[p] == i || (MIN ? -Ax[p] : std::fabs(Ax[p])) >= threshold) big = dmax(big, std::fabs(Ax[p]));
    const double r = 1.0 / big;
    int w = 0;
    for (int p = r0; p < r1; ++p)
        if (Aj[p] == i || (MIN ? -Ax[p] : std::fabs(Ax[p])) >= threshold) {
            const double s = std::fabs(Ax[p]) * r;
            if (s != 0.0) {                                 // eliminate_zeros
                if (Sj) { Sj[w] = Aj[p]; Sx[w] = s; }
                ++w;
            }
        }
    return w;
}

// The state of node i after one synchronous round, from the states `prev` of the round before.  The graph is the union of the two
// patterns (Tp may be null); self loops are skipped.  A node that stays active returns `active`.
PAMG_CLS_HD int mis_node(int i, const int *Gp, const int *Gj, const int *Tp, const int *Tj, const double *y, const int *prev, int active, int C,
                         int F)
{
    const double yi = y[i];
    bool blocked = false;
    for (int pass = 0; pass < 2; ++pass) {
        const int *P = pass ? Tp : Gp, *J = pass ? Tj : Gj;
        if (!P) continue;
        for (int p = P[i]; p < P[i + 1]; ++p) {
            const int j = J[p];
            if (j == i) continue;
            const int xj = prev[j];
            if (xj == C) return F;                          // a neighbour is in the set
            if (xj == active) {
                const double yj = y[j];
                if (yj > yi || (yj == yi && j > i)) blocked = true;
            }
        }
    }
    return blocked ? active : C;
}

PAMG_CLS_HD int interp_count_row(int i, const int *Sp, const int *Sj, const int *splitting)
{
    if (splitting[i] == C_NODE) return 1;
    int n = 0;
    for (int p = Sp[i]; p < Sp[i + 1]; ++p)
        if (splitting[Sj[p]] == C_NODE && Sj[p] != i) ++n;
    return n;
}

// Row i of P by direct interpolation; map = exclusive scan of splitting (the coarse number of a C-point)
PAMG_CLS_HD void direct_row(int i, const int *Ap, const int *Aj, const double *Ax, const int *Sp, const int *Sj, const double *Sx,
                            const int *splitting, const int *Pp, const int *map, int *Pj, double *Px)
{
    if (splitting[i] == C_NODE) { Pj[Pp[i]] = map[i]; Px[Pp[i]] = 1.0; return; }
    double sum_strong_pos = 0.0, sum_strong_neg = 0.0;
    for (int p = Sp[i]; p < Sp[i + 1]; ++p)
        if (splitting[Sj[p]] == C_NODE && Sj[p] != i) {
            if (Sx[p] < 0) sum_strong_neg += Sx[p];
            else sum_strong_pos += Sx[p];
        }
    double sum_all_pos = 0.0, sum_all_neg = 0.0, diag = 0.0;
    for (int p = Ap[i]; p < Ap[i + 1]; ++p) {
        if (Aj[p] == i) diag += Ax[p];
        else if (Ax[p] < 0) sum_all_neg += Ax[p];
        else sum_all_pos += Ax[p];
    }
    const double alpha = sum_all_neg / sum_strong_neg;
    double beta = sum_all_pos / sum_strong_pos;
    if (sum_strong_pos == 0) { diag += sum_all_pos; beta = 0.0; }
    const double neg_coeff = -alpha / diag, pos_coeff = -beta / diag;
    int w = Pp[i];
    for (int p = Sp[i]; p < Sp[i + 1]; ++p)
        if (splitting[Sj[p]] == C_NODE && Sj[p] != i) {
            Pj[w] = map[Sj[p]];
            Px[w] = (Sx[p] < 0 ? neg_coeff : pos_coeff) * Sx[p];
            ++w;
        }
}

// Zero the strong F-F entries of row `row` whose two ends share no strong C-point
PAMG_CLS_HD void remove_ff_row(int row, const int *Sp, const int *Sj, double *Sx, const int *splitting)
{
    if (splitting[row] != F_NODE) return;
    for (int jj = Sp[row]; jj < Sp[row + 1]; ++jj) {
        const int j = Sj[jj];
        if (splitting[j] != F_NODE) continue;
        bool dependence = false;
        for (int ii = Sp[row]; ii < Sp[row + 1] && !dependence; ++ii) {
            const int c = Sj[ii];
            if (splitting[c] != C_NODE) continue;
            for (int kk = Sp[j]; kk < Sp[j + 1]; ++kk)
                if (Sj[kk] == c) { dependence = true; break; }
        }
        if (!dependence) Sx[jj] = 0.0;
    }
}

// ---- classical interpolation, F-row i.  Its strong entries are "staged": col[t], val[t], kind[t] for t in [0, ns)
PAMG_CLS_HD unsigned char strong_kind(int i, int col, const int *splitting)
{
    if (splitting[col] == C_NODE) return K_C;
    return (splitting[col] == F_NODE && col != i) ? K_F : K_NONE;
}

// a_ii + the weak connections: the whole row of A minus the strong off-diagonal entries
PAMG_CLS_HD double classical_denominator(int i, const int *Ap, const double *Ax, const int *Sp, const int *Sj, const double *Sx)
{
    double d = 0.0;
    for (int p = Ap[i]; p < Ap[i + 1]; ++p) d += Ax[p];
    for (int p = Sp[i]; p < Sp[i + 1]; ++p)
        if (Sj[p] != i) d -= Sx[p];
    return d;
}

// For the strong F-neighbour k: a_kk (modified form only) and the sum of a_kl over the row's strong C-neighbours l, in the row's stored order
PAMG_CLS_HD void classical_inner(int ns, const int *col, const unsigned char *kind, int k, const int *Ap, const int *Aj, const double *Ax,
                                 bool modified, double *inner, double *akk)
{
    const int r0 = Ap[k], r1 = Ap[k + 1];
    double a_kk = 0.0;
    if (modified)
        for (int p = r0; p < r1; ++p)
            if (Aj[p] == k) a_kk = Ax[p];
    double den = 0.0;
    for (int t = 0; t < ns; ++t) {
        if (kind[t] != K_C) continue;
        const int l = col[t];
        for (int p = r0; p < r1; ++p)
            if (Aj[p] == l) {
                const double a_kl = Ax[p];
                if (!modified || signof(a_kl) != signof(a_kk)) den += a_kl;
                break;
            }
    }
    *inner = den;
    *akk = a_kk;
}

// The weight of the strong C-neighbour at staged position t: -(a_ij + sum_k a_ik a_kj / inner_k) / denominator, k in stored order
PAMG_CLS_HD double classical_weight(int ns, const int *col, const double *val, const unsigned char *kind, const double *inner, const double *akk,
                                    int t, const int *Ap, const int *Aj, const double *Ax, bool modified, double denominator)
{
    const int j = col[t];
    double numerator = val[t];
    for (int u = 0; u < ns; ++u) {
        if (kind[u] != K_F) continue;
        const int k = col[u];
        const double a_ik = val[u];
        double a_kj = 0.0;
        for (int p = Ap[k]; p < Ap[k + 1]; ++p)
            if (Aj[p] == j) {
                a_kj = Ax[p];
                if (!modified) break;                       // the reference's modified search walks on (:1303-1310): the last stored entry
            }
        if (modified && signof(a_kj) == signof(akk[u])) a_kj = 0.0;
        if (std::fabs(a_kj) > 1e-15 * std::fabs(a_ik)) numerator += a_ik * a_kj / inner[u];
    }
    return -numerator / denominator;
}

// position of staged entry t among the row's strong C-neighbours (its offset in the row of P)
PAMG_CLS_HD int c_rank(const unsigned char *kind, int t)
{
    int r = 0;
    for (int u = 0; u < t; ++u) r += kind[u] == K_C;
    return r;
}

}  // namespace cls
}  // namespace pamg
