// pamg_dtri_plan.h -- host plan of the DENSE BLOCK-TRIANGULAR form of a symmetric Gauss-Seidel sweep from zero (f64, scalar CSR, every row
// with its diagonal).  Plain C++: included by pamg_dtri.hip and by tests/dtri_emul.cpp.
//
// The symmetric sweep from x = 0 is the fixed linear operator x = S b, S = (D+U)^-1 D (D+L)^-1.  The rows, in sweep order, are cut into
// nb = ceil(n / B) contiguous blocks [lo_k, hi_k).  With Wf_k = tril(A_kk)^-1 and Wb_k = triu(A_kk)^-1 kept as dense packed triangles:
//
//     forward :  for k = 0 .. nb-1 :  t_k = b_k - A[k, cols < lo_k] y          (sparse phase: the off-block slice Lo)
//                                     y_k = Wf_k t_k                           (dense phase)
//     backward:  for k = nb-1 .. 0 :  t_k = (D y)_k - A[k, cols >= hi_k] z     (off-block slice Uo)
//                                     z_k = Wb_k t_k
//
// The dependency chain of the sweep is 2 nb block steps of bulk parallel work.  The price is memory: two triangles of B (B + 2) / 2 values per block.
//
// Layout of a packed triangle of m rows: row-major, LOCAL row i holds its i + 1 values W[i][0..i] in an even number of slots (16-byte loads), so
// rows 2p and 2p + 1 both take 2p + 2 slots: row i starts at dtri_row_off(i).  The backward triangle is stored in REVERSED local order (local
// row i' = global row hi - 1 - i', local column likewise), which makes it a lower triangle too: one kernel serves both.
//
// Growth guard: the planner declines where a block's inverse is large, by the per-row factor the merged planner bounds (pamg_lanem_plan.h,
// `growth_cap`): sum_j |W_ij| |a_jj| (1 for a diagonal block; <= 1 per term on diagonally dominant operators), at the cap its callers pass.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define PAMG_DTRI_HD __host__ __device__ __forceinline__
#else
#define PAMG_DTRI_HD inline
#endif

namespace pamg {

constexpr double DTRI_GROWTH_CAP = 1e3;          // the bound build_lanem_plan is called with (pamg_lane.hip)
constexpr int DTRI_BLOCK_ROWS = 2048;            // default block size (profiles/r17_microbench_dtri_scan.json)
constexpr int DTRI_MAX_BLOCK_ROWS = 8192;

enum : int { DTRI_OK = 0, DTRI_E_SHAPE = 1, DTRI_E_DIAGONAL = 2, DTRI_E_GROWTH = 3, DTRI_E_NONFINITE = 4 };

// first slot of local row i of a packed triangle, and the slots of a triangle of m rows
PAMG_DTRI_HD int64_t dtri_row_off(int64_t i) { const int64_t p = i >> 1; return (i & 1) ? 2 * (p + 1) * (p + 1) : 2 * p * (p + 1); }
inline int64_t dtri_tri_slots(int64_t m) { return dtri_row_off(m); }

struct DtriPlan {
    int n = 0, B = 0, nb = 0;
    std::vector<int> Lp, Lj, Up, Uj;             // the off-block slices as CSR over all n rows: columns < lo(row) / columns >= hi(row)
    std::vector<double> Lx, Ux;
    std::vector<double> diag;
    std::vector<int64_t> woff;                   // [nb + 1] first slot of block k's triangle (the same for Wf and Wb)
    int lo(int k) const { return k * B; }
    int hi(int k) const { return (int)std::min<int64_t>((int64_t)(k + 1) * B, n); }
    int64_t off_block_entries() const { return (int64_t)Lj.size() + (int64_t)Uj.size(); }
};

// Partition, slices and bookkeeping.  DTRI_E_DIAGONAL: a row without exactly one stored diagonal entry, or a zero / non-finite diagonal value;
// DTRI_E_NONFINITE (a status of its own, not DTRI_E_DIAGONAL): a stored off-diagonal value, in a block or off it, is NaN or infinite -- a dense
// triangle multiplies its stored zeros by such a value and spreads it over rows the sequential sweep leaves finite, and the growth guard sees
// in-block values only; DTRI_E_SHAPE: nothing to plan.  The first offending row in row order decides the status.  (The growth guard needs the
// inverses: dtri_host_growth here, a kernel on the device.)
inline int build_dtri_plan(int n, const int *Ap, const int *Aj, const double *Ax, int B, DtriPlan &P)
{
    if (n < 1 || B < 1) return DTRI_E_SHAPE;
    P = DtriPlan();
    P.n = n; P.B = B; P.nb = (n + B - 1) / B;
    P.diag.assign((size_t)n, 0.0);
    P.Lp.assign((size_t)n + 1, 0);
    P.Up.assign((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) {
        const int lo = (i / B) * B, hi = (int)std::min<int64_t>((int64_t)lo + B, n);
        int nd = 0, cl = 0, cu = 0;
        bool finite = true;
        for (int p = Ap[i]; p < Ap[i + 1]; ++p) {
            const int j = Aj[p];
            if (j < 0 || j >= n) return DTRI_E_SHAPE;
            if (j == i) { ++nd; P.diag[(size_t)i] = Ax[p]; }
            else finite = finite && std::isfinite(Ax[p]);
            cl += j < lo; cu += j >= hi;
        }
        const double d = P.diag[(size_t)i];
        if (nd != 1 || !(d != 0.0) || !std::isfinite(d)) return DTRI_E_DIAGONAL;
        if (!finite) return DTRI_E_NONFINITE;
        P.Lp[(size_t)i + 1] = P.Lp[(size_t)i] + cl;
        P.Up[(size_t)i + 1] = P.Up[(size_t)i] + cu;
    }
    P.Lj.resize((size_t)P.Lp[(size_t)n]); P.Lx.resize((size_t)P.Lp[(size_t)n]);
    P.Uj.resize((size_t)P.Up[(size_t)n]); P.Ux.resize((size_t)P.Up[(size_t)n]);
    for (int i = 0; i < n; ++i) {
        const int lo = (i / B) * B, hi = (int)std::min<int64_t>((int64_t)lo + B, n);
        int ql = P.Lp[(size_t)i], qu = P.Up[(size_t)i];
        for (int p = Ap[i]; p < Ap[i + 1]; ++p) {
            const int j = Aj[p];
            if (j < lo) { P.Lj[(size_t)ql] = j; P.Lx[(size_t)ql] = Ax[p]; ++ql; }
            else if (j >= hi) { P.Uj[(size_t)qu] = j; P.Ux[(size_t)qu] = Ax[p]; ++qu; }
        }
    }
    P.woff.assign((size_t)P.nb + 1, 0);
    for (int k = 0; k < P.nb; ++k) P.woff[(size_t)k + 1] = P.woff[(size_t)k] + dtri_tri_slots(P.hi(k) - P.lo(k));
    return DTRI_OK;
}

// Reference inverse of one block: W (dtri_tri_slots(m) values, the padding slots zero) = tril(A_kk)^-1 (dir 0) or triu(A_kk)^-1 in reversed
// local order (dir 1).  Column by column, rows in order: W[i][j] = (delta_ij - sum_{j <= c < i} T[i][c] W[c][j]) / T[i][i] over the sparse
// in-block row -- the recurrence, and the order of its additions, of the device kernel.
inline void dtri_host_inverse(const DtriPlan &P, const int *Ap, const int *Aj, const double *Ax, int k, int dir, double *W)
{
    const int lo = P.lo(k), hi = P.hi(k), m = hi - lo;
    for (int64_t q = 0; q < dtri_tri_slots(m); ++q) W[q] = 0.0;
    for (int j = 0; j < m; ++j)
        for (int i = j; i < m; ++i) {
            const int gi = dir ? hi - 1 - i : lo + i;
            double s = i == j ? 1.0 : 0.0;
            for (int p = Ap[gi]; p < Ap[gi + 1]; ++p) {
                const int gc = Aj[p];
                if (gc < lo || gc >= hi) continue;
                const int c = dir ? hi - 1 - gc : gc - lo;
                if (c >= i || c < j) continue;
                s = s - Ax[p] * W[dtri_row_off(c) + j];
            }
            W[dtri_row_off(i) + j] = s / P.diag[(size_t)gi];
        }
}

// the guard's figure of one block: max_i sum_j |W_ij| |a_jj| (infinity where a value is not finite)
inline double dtri_host_growth(const DtriPlan &P, int k, int dir, const double *W)
{
    const int lo = P.lo(k), hi = P.hi(k), m = hi - lo;
    double g = 0.0;
    for (int i = 0; i < m; ++i) {
        double s = 0.0;
        for (int j = 0; j <= i; ++j) s += std::fabs(W[dtri_row_off(i) + j]) * std::fabs(P.diag[(size_t)(dir ? hi - 1 - j : lo + j)]);
        if (!std::isfinite(s)) s = INFINITY;
        g = std::max(g, s);
    }
    return g;
}

// Host replay of the launch sequence (the CPU test; the device kernels compute the same phases with lane-parallel row sums).
// acc = false: x = S b;  acc = true: x += S b.  Wf / Wb: the triangles of all blocks at P.woff.
inline void dtri_host_apply(const DtriPlan &P, const double *Wf, const double *Wb, const double *b, double *x, bool acc)
{
    const int n = P.n;
    std::vector<double> t((size_t)P.B), y((size_t)n, 0.0), dy((size_t)n, 0.0), z((size_t)n, 0.0);
    for (int k = 0; k < P.nb; ++k) {
        const int lo = P.lo(k), m = P.hi(k) - lo;
        for (int l = 0; l < m; ++l) {
            double s = 0.0;
            for (int p = P.Lp[(size_t)(lo + l)]; p < P.Lp[(size_t)(lo + l) + 1]; ++p) s += P.Lx[(size_t)p] * y[(size_t)P.Lj[(size_t)p]];
            t[(size_t)l] = b[lo + l] - s;
        }
        const double *W = Wf + P.woff[(size_t)k];
        for (int l = 0; l < m; ++l) {
            double s = 0.0;
            for (int j = 0; j <= l; ++j) s += W[dtri_row_off(l) + j] * t[(size_t)j];
            y[(size_t)(lo + l)] = s;
            dy[(size_t)(lo + l)] = P.diag[(size_t)(lo + l)] * s;
        }
    }
    for (int k = P.nb - 1; k >= 0; --k) {
        const int hi = P.hi(k), m = hi - P.lo(k);
        for (int l = 0; l < m; ++l) {
            const int g = hi - 1 - l;
            double s = 0.0;
            for (int p = P.Up[(size_t)g]; p < P.Up[(size_t)g + 1]; ++p) s += P.Ux[(size_t)p] * z[(size_t)P.Uj[(size_t)p]];
            t[(size_t)l] = dy[(size_t)g] - s;
        }
        const double *W = Wb + P.woff[(size_t)k];
        for (int l = 0; l < m; ++l) {
            const int g = hi - 1 - l;
            double s = 0.0;
            for (int j = 0; j <= l; ++j) s += W[dtri_row_off(l) + j] * t[(size_t)j];
            z[(size_t)g] = s;
            x[g] = acc ? x[g] + s : s;
        }
    }
}

}  // namespace pamg
