// pamg_energy.h -- the per-element arithmetic of energy-minimisation prolongation smoothing (CG, GMRES), shared by the kernels of
// pamg_energy.hip and the host replays tests/energy_emul.cpp and tests/energy_gmres_emul.cpp (lanes, groups and workgroups as loops), as pamg_air.h is shared by the AIR
// setup.  Blocks are row-major: A r x m, B (the operand, T or P) m x c, S r x c; the candidates Bc are [n_bcol * c] x K row-major.
//
//   imm_entry      element (a, d) of the block S(i, col) of incomplete_mat_mult_bsr (smoothed_aggregation.h:970-1042): the contributions
//                  in the order of A's stored row i, within it of B's stored row Aj[jj] (every match counts, no sorting assumed), within
//                  a block in gemm's 'F','T','F' order (linalg.h:466-492), which for one element is cc ascending.  The 1 x 1 shortcut
//                  *Sk += Ax * Bx is the same expression.  The operand's values come through a functor, so that the CG driver reads the
//                  new search direction without storing it first
//   ub_entry       element (a, v) of row i of U @ Bc in the order of SciPy's bsr_matvecs: blocks in stored order, cc ascending, from 0.0
//   update_entry   element (a, d) of Update = UB_i (BtBinv_i Bc_j^H) as the two gemm calls of satisfy_constraints_helper compute it
//                  (smoothed_aggregation.h:760-764): C[d, k] = sum_k2 BtBinv_i[k, k2] Bc_j[d, k2], Update[a, d] = sum_k UB_i[a, k] C[d, k],
//                  both from 0.0, ascending
//   lane_partial,  the fixed summation tree of the driver's two inner products: one partial per block row (stored order), RED_PER
//   tree_fold      consecutive partials per lane, RED_LANES lanes folded by halving, then the chunk sums the same way by one workgroup.
//                  Its shape depends on the number of block rows alone
//
// Every sum runs serially in the reference's order, so with -ffp-contract=off the first three are the reference's bit for bit.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PAMG_EN_HD __host__ __device__ inline          // (inline: pamg_rootnode.hip includes this header too)
#else
#define PAMG_EN_HD inline
#endif

namespace pamg {
namespace energy {

constexpr int MAX_BLOCK = 6;                                // rows / columns of a block
constexpr int MAX_NULLDIM = 6;                              // candidates
constexpr int RED_LANES = 256, RED_PER = 4, RED_CHUNK = RED_LANES * RED_PER;

// lanes per block row, from the mean number of stored elements per row of the pattern
inline int group_width(int64_t elements, int n)
{
    const int64_t mean = n ? elements / n : 0;
    return mean <= 8 ? 8 : mean <= 16 ? 16 : mean <= 32 ? 32 : 64;
}

// the operand's stored values: value (cc, d) of the stored block kk
struct StoredBlocks {
    const double *Bx;
    int m, c;
    PAMG_EN_HD double operator()(int kk, int /*brow*/, int cc, int d) const { return Bx[((int64_t)kk * m + cc) * c + d]; }
};

// the CG search direction of this iteration, P = Z + beta P_old with Z = Dinv R (P = Z in the first), formed where it is read
struct Direction {
    const double *R, *Pold, *Dinv, *beta;                   // beta: device-side scalar
    int m, c, first;
    PAMG_EN_HD double operator()(int kk, int brow, int cc, int d) const
    {
        const int64_t e = ((int64_t)kk * m + cc) * c + d;
        const double z = R[e] * Dinv[(int64_t)brow * m + cc];
        if (first) return z;
        const double bp = *beta * Pold[e];
        return z + bp;
    }
};

template <class BV>
PAMG_EN_HD double imm_entry(double acc, int i, int col, int a, int d, const int *Ap, const int *Aj, const double *Ax, const int *Bp,
                            const int *Bj, BV bval, int r, int m)
{
    for (int jj = Ap[i]; jj < Ap[i + 1]; ++jj) {
        const int j = Aj[jj];
        const double *Ab = Ax + ((int64_t)jj * r + a) * m;
        for (int kk = Bp[j]; kk < Bp[j + 1]; ++kk) {
            if (Bj[kk] != col) continue;
            for (int cc = 0; cc < m; ++cc) {
                const double t = Ab[cc] * bval(kk, j, cc, d);
                acc += t;
            }
        }
    }
    return acc;
}

PAMG_EN_HD double ub_entry(int i, int a, int v, const int *Sp, const int *Sj, const double *Sx, const double *Bc, int r, int c, int K)
{
    double s = 0.0;
    for (int p = Sp[i]; p < Sp[i + 1]; ++p) {
        const double *blk = Sx + ((int64_t)p * r + a) * c;
        const double *bj = Bc + (int64_t)Sj[p] * c * K;
        for (int cc = 0; cc < c; ++cc) {
            const double t = blk[cc] * bj[cc * K + v];
            s += t;
        }
    }
    return s;
}

// UBi: the r x K row of U @ Bc, BtBinv_i: K x K, col: the block column
PAMG_EN_HD double update_entry(const double *UBi, const double *BtBinv_i, const double *Bc, int col, int a, int d, int c, int K)
{
    const double *bt = Bc + ((int64_t)col * c + d) * K;
    double upd = 0.0;
    for (int k = 0; k < K; ++k) {
        double cdk = 0.0;
        for (int k2 = 0; k2 < K; ++k2) {
            const double t = BtBinv_i[k * K + k2] * bt[k2];
            cdk += t;
        }
        const double t = UBi[a * K + k] * cdk;
        upd += t;
    }
    return upd;
}

// ---- what one lane of a group of gw lanes does for block row i: it owns the elements lane, lane + gw, ... of the row's stored blocks
// (element e of the row: block Sp[i] + e / (r c), entry (a, d) = ((e % (r c)) / c, e % c)).  Between two of these phases the group
// meets at a barrier; the replay runs each phase for every lane in turn.

// the row of A B on the pattern: from Sin (incomplete_mat_mult_bsr accumulates) or, Sin == nullptr, from 0.0; negate: R = -(A T)
template <class BV>
PAMG_EN_HD void imm_lane(int lane, int gw, int i, const int *Ap, const int *Aj, const double *Ax, const int *Bp, const int *Bj, BV bval,
                         const int *Sp, const int *Sj, const double *Sin, double *Sout, bool negate, int r, int m, int c)
{
    const int rc = r * c, len = (Sp[i + 1] - Sp[i]) * rc;
    for (int e = lane; e < len; e += gw) {
        const int p = Sp[i] + e / rc, a = (e % rc) / c, d = e % c;
        const int64_t at = (int64_t)Sp[i] * rc + e;
        const double v = imm_entry(Sin ? Sin[at] : 0.0, i, Sj[p], a, d, Ap, Aj, Ax, Bp, Bj, bval, r, m);
        Sout[at] = negate ? -v : v;
    }
}

// the row of the new search direction, stored
PAMG_EN_HD void pnew_lane(int lane, int gw, int i, const int *Sp, const Direction &dir, double *Pnew, int r, int c)
{
    const int rc = r * c, len = (Sp[i + 1] - Sp[i]) * rc;
    for (int e = lane; e < len; e += gw) Pnew[(int64_t)Sp[i] * rc + e] = dir(Sp[i] + e / rc, i, (e % rc) / c, e % c);
}

// UBi [r * K] = row i of S @ Bc
PAMG_EN_HD void ub_lane(int lane, int gw, int i, const int *Sp, const int *Sj, const double *Sx, const double *Bc, double *UBi, int r, int c,
                        int K)
{
    for (int q = lane; q < r * K; q += gw) UBi[q] = ub_entry(i, q / K, q % K, Sp, Sj, Sx, Bc, r, c, K);
}

// Sx -= UBi (BtBinv_i Bc_j^H) on the row's stored blocks
PAMG_EN_HD void project_lane(int lane, int gw, int i, const int *Sp, const int *Sj, double *Sx, const double *UBi, const double *BtBinv,
                             const double *Bc, int r, int c, int K)
{
    const int rc = r * c, len = (Sp[i + 1] - Sp[i]) * rc;
    const double *bi = BtBinv + (int64_t)i * K * K;
    for (int e = lane; e < len; e += gw) {
        const int p = Sp[i] + e / rc, a = (e % rc) / c, d = e % c;
        const double upd = update_entry(UBi, bi, Bc, Sj[p], a, d, c, K);
        Sx[(int64_t)Sp[i] * rc + e] -= upd;
    }
}

// T += alpha P, C-point rows reset to the injection's (T = I_F T + P_I), R -= alpha AP
PAMG_EN_HD void update_lane(int lane, int gw, int i, const int *Sp, double *T, double *R, const double *P, const double *AP, double alpha,
                            const unsigned char *cmask, const double *PI, int r, int c)
{
    const int rc = r * c, len = (Sp[i + 1] - Sp[i]) * rc;
    for (int e = lane; e < len; e += gw) {
        const int64_t at = (int64_t)Sp[i] * rc + e;
        const double ap = alpha * P[at];
        double t = T[at] + ap;
        if (cmask && cmask[(int64_t)i * r + (e % rc) / c]) t = PI[at];
        T[at] = t;
        const double aap = alpha * AP[at];
        R[at] = R[at] - aap;
    }
}

// <X, Y> over the stored elements e0 .. e1 of one block row, in stored order from 0.0
PAMG_EN_HD double row_dot(const double *X, const double *Y, int64_t e0, int64_t e1)
{
    double s = 0.0;
    for (int64_t e = e0; e < e1; ++e) {
        const double t = X[e] * Y[e];
        s += t;
    }
    return s;
}

// <R, Dinv R> over block row i (Z = Dinv R is rounded first, like scale_rows), and the number of its blocks with a non-zero entry
PAMG_EN_HD double row_rz(const double *R, const double *Dinv, int i, int p0, int p1, int r, int c, int *nonzero_blocks)
{
    double s = 0.0;
    int nzb = 0;
    for (int p = p0; p < p1; ++p) {
        bool any = false;
        for (int a = 0; a < r; ++a)
            for (int d = 0; d < c; ++d) {
                const double x = R[((int64_t)p * r + a) * c + d];
                const double z = x * Dinv[(int64_t)i * r + a];
                const double t = x * z;
                s += t;
                any |= x != 0.0;
            }
        nzb += any;
    }
    *nonzero_blocks = nzb;
    return s;
}

// lane t of the chunk that starts at base: RED_PER consecutive values, ascending, from 0.0
PAMG_EN_HD double lane_partial(const double *v, int64_t n, int64_t base, int t)
{
    double s = 0.0;
    for (int q = 0; q < RED_PER; ++q) {
        const int64_t idx = base + (int64_t)t * RED_PER + q;
        if (idx < n) s += v[idx];
    }
    return s;
}

// lane t of the last level: the values t, t + RED_LANES, ... ascending, from 0.0
PAMG_EN_HD double lane_strided(const double *v, int64_t n, int t)
{
    double s = 0.0;
    for (int64_t idx = t; idx < n; idx += RED_LANES) s += v[idx];
    return s;
}

// the halving fold of RED_LANES lane values, as one workgroup does it between barriers (host form; the kernels run the same steps)
inline double tree_fold(double *lane)
{
    for (int s = RED_LANES / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; ++t) lane[t] = lane[t] + lane[t + s];
    return lane[0];
}

inline int64_t chunks(int64_t n) { return (n + RED_CHUNK - 1) / RED_CHUNK; }

// what the loop of cg_prolongation_smoothing does at its head (smooth.py:381-392) with the reduced values: 2 = `resid > tol` fails
// (resid: the stored size of R, zero blocks dropped as SciPy's subtraction drops them), 1 = newsum < tol, 0 = go on
PAMG_EN_HD int cg_stop(double resid, double newsum, double tol) { return !(resid > tol) ? 2 : (newsum < tol ? 1 : 0); }

// ---- GMRES (gmres_prolongation_smoothing, smooth.py:648-872).  Local to a block row it is the CG driver's arithmetic with the row
// weights applied where scale_rows applies them (on the product, before the projection); the element-wise updates are the
// reference's expressions; the Frobenius inner products go through the tree above; the Hessenberg column, the rotations and g are one
// function that a single lane runs on the device and the replay calls as it is.
constexpr int GMRES_MAXITER = 32, GMRES_LD = GMRES_MAXITER + 1;

// the row of Dinv (A V) on the pattern from 0.0 (negate: Dinv (-(A T)), the initial residual), not yet projected
template <class BV>
PAMG_EN_HD void imm_scaled_lane(int lane, int gw, int i, const int *Ap, const int *Aj, const double *Ax, BV bval, const int *Sp, const int *Sj,
                                const double *Dinv, double *Sout, bool negate, int r, int c)
{
    const int rc = r * c, len = (Sp[i + 1] - Sp[i]) * rc;
    for (int e = lane; e < len; e += gw) {
        const int p = Sp[i] + e / rc, a = (e % rc) / c, d = e % c;
        double v = imm_entry(0.0, i, Sj[p], a, d, Ap, Aj, Ax, Sp, Sj, bval, r, r);
        if (negate) v *= -1.0;
        Sout[(int64_t)Sp[i] * rc + e] = v * Dinv[(int64_t)i * r + a];
    }
}

// W -= h V (modified Gram-Schmidt: h was taken on the W that comes in)
PAMG_EN_HD void mgs_lane(int lane, int gw, int i, const int *Sp, double *W, const double *V, double h, int r, int c)
{
    const int rc = r * c, len = (Sp[i + 1] - Sp[i]) * rc;
    for (int e = lane; e < len; e += gw) {
        const int64_t at = (int64_t)Sp[i] * rc + e;
        const double hv = h * V[at];
        W[at] = W[at] - hv;
    }
}

// V = s V: the first basis vector (s = 1.0 / normr) and the normalisation (s = 1.0 / H[i+1, i])
PAMG_EN_HD void scale_lane(int lane, int gw, int i, const int *Sp, double *V, double s, int r, int c)
{
    const int rc = r * c, len = (Sp[i + 1] - Sp[i]) * rc;
    for (int e = lane; e < len; e += gw) {
        const int64_t at = (int64_t)Sp[i] * rc + e;
        V[at] = s * V[at];
    }
}

// T = T + y[j] V_j for j ascending (V_j = V + j * stride), then the C-point rows reset to the injection's (T = I_F T + P_I)
PAMG_EN_HD void combine_lane(int lane, int gw, int i, const int *Sp, double *T, const double *V, int64_t stride, const double *y, int ny,
                             const unsigned char *cmask, const double *PI, int r, int c)
{
    const int rc = r * c, len = (Sp[i + 1] - Sp[i]) * rc;
    for (int e = lane; e < len; e += gw) {
        const int64_t at = (int64_t)Sp[i] * rc + e;
        double t = T[at];
        for (int j = 0; j < ny; ++j) {
            const double yv = y[j] * V[(int64_t)j * stride + at];
            t = t + yv;
        }
        if (cmask && cmask[(int64_t)i * r + (e % rc) / c]) t = PI[at];
        T[at] = t;
    }
}

// the Krylov side's scalars: H as the reference holds it (row-major, leading dimension GMRES_LD), the rotations, g, the normr history
struct GmresState {
    double H[GMRES_LD * GMRES_LD], g[GMRES_LD], normr[GMRES_LD], Qc[GMRES_MAXITER], Qs[GMRES_MAXITER];
    double h;                                               // the coefficient of the next Gram-Schmidt pass
    double scale;                                           // what the newest basis vector is multiplied by, if `scaled`
    int scaled, nq, iterations, stop;
};

// after the initial residual: total = <R, R>.  g[0] = normr; V_0 = (1.0 / normr) R if normr > 0.0; the loop's head
PAMG_EN_HD void gmres_start(GmresState &S, double total, int maxiter, double tol)
{
    const double normr = std::sqrt(total);
    S.g[0] = normr;
    S.normr[0] = normr;
    S.scaled = normr > 0.0;
    S.scale = S.scaled ? 1.0 / normr : 0.0;
    S.nq = 0;
    S.iterations = 0;
    S.stop = !(0 < maxiter && normr > tol && S.scaled);
}

// H[j, i] = <V_j, W>: kept, and handed to the pass that subtracts with it
PAMG_EN_HD void gmres_coefficient(GmresState &S, int j, int i, double total)
{
    S.H[j * GMRES_LD + i] = total;
    S.h = total;
}

// the end of iteration i (smooth.py:816-854): total = <W, W> after the last Gram-Schmidt pass
PAMG_EN_HD void gmres_column(GmresState &S, int i, double total, int maxiter, double tol)
{
    double *H = S.H;
    const int L = GMRES_LD;
    H[(i + 1) * L + i] = std::sqrt(total);
    S.scaled = H[(i + 1) * L + i] != 0.0;                   // the breakdown check
    S.scale = S.scaled ? 1.0 / H[(i + 1) * L + i] : 0.0;
    for (int j = 0; j < S.nq && j < i; ++j) {               // apply_givens(Q, H[:, i], i)
        const double v0 = H[j * L + i], v1 = H[(j + 1) * L + i];
        const double a0 = S.Qc[j] * v0, a1 = S.Qs[j] * v1, b0 = -S.Qs[j] * v0, b1 = S.Qc[j] * v1;
        H[j * L + i] = a0 + a1;
        H[(j + 1) * L + i] = b0 + b1;
    }
    if (H[(i + 1) * L + i] != 0.0) {
        const double h1 = H[i * L + i], h2 = H[(i + 1) * L + i];
        const double h1_mag = std::fabs(h1), h2_mag = std::fabs(h2);
        double mu, tau;
        if (h1_mag < h2_mag) {
            mu = h1 / h2;
            tau = mu / std::fabs(mu);
        } else {
            mu = h2 / h1;
            tau = mu / std::fabs(mu);
        }
        const double q1 = h1_mag * h1_mag, q2 = h2_mag * h2_mag;
        const double denom = std::sqrt(q1 + q2);
        const double c = h1_mag / denom;
        const double st = h2_mag * tau;
        const double s = st / denom;
        S.Qc[S.nq] = c;
        S.Qs[S.nq] = s;
        ++S.nq;
        const double g0 = S.g[i], g1 = S.g[i + 1];
        const double a0 = c * g0, a1 = s * g1, b0 = -s * g0, b1 = c * g1;
        S.g[i] = a0 + a1;
        S.g[i + 1] = b0 + b1;
        const double c0 = c * h1, c1 = s * h2;
        H[i * L + i] = c0 + c1;
        H[(i + 1) * L + i] = 0.0;
    }
    const double normr = std::fabs(S.g[i + 1]);
    S.normr[i + 1] = normr;
    S.iterations = i + 1;
    S.stop = !(i + 1 < maxiter && normr > tol);
}

// y = H[0:k, 0:k]^-1 g[0:k] for the upper triangular H the rotations leave (what la.solve's LU without a row exchange comes to):
// back substitution, column by column
inline void gmres_solve(const GmresState &S, int k, double *y)
{
    for (int j = 0; j < k; ++j) y[j] = S.g[j];
    for (int j = k - 1; j >= 0; --j) {
        y[j] = y[j] / S.H[j * GMRES_LD + j];
        for (int q = 0; q < j; ++q) {
            const double t = y[j] * S.H[q * GMRES_LD + j];
            y[q] = y[q] - t;
        }
    }
}

}  // namespace energy
}  // namespace pamg
