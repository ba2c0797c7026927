// pamg_dense_pinv.h -- the per-lane arithmetic of the Schwarz setup (pamg_schwarz_setup.hip): membership search of the
// block extraction and the one-sided (Hestenes) Jacobi SVD behind the batched pseudo-inverse of variable-size blocks.
//
// Everything here is plain scalar C++ that compiles for the host and for the device, so that a host program can replay
// the kernels with the lanes of a group as a loop (tests/schwarz_setup_emul.cpp).  What a kernel adds is the lane
// mapping: a group of W lanes (W = 8 / 16 / 32 / 64, the size class of the block) owns one m x m block, lane i owns row i
// of U and of V, a column dot product is the butterfly sum `butterfly_offsets` describes.
//
// The method:  B V = U Sigma.  U starts as B, V as I; every sweep visits the column pairs (j, k), j < k, in cyclic order
// and rotates the pair in U and V until u_j . u_k is at rounding level.  Afterwards sigma_j = |u_j|, a singular value
// with sigma_j <= rank_tol * sigma_max counts as zero (LAPACK gelss' rule, which the reference's schwarz_parameters
// relies on), and  pinv(B) = sum over the kept j of  v_j u_j^T / sigma_j^2.
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

#if defined(__HIPCC__)
#define PAMG_DP_HD __host__ __device__ inline
#else
#define PAMG_DP_HD inline
#endif

namespace pamg {
namespace dpinv {

constexpr int MAX_M = 64;          // largest block the device path takes
constexpr int SWEEP_CAP = 60;      // Jacobi sweeps before a block counts as not converged
constexpr int NCLASS = 4;

// size class of an m x m block: its group is 8 << class lanes wide
PAMG_DP_HD int size_class(int m) { return m <= 8 ? 0 : (m <= 16 ? 1 : (m <= 32 ? 2 : 3)); }
PAMG_DP_HD int class_width(int c) { return 8 << c; }

// position of `col` in the sorted list S[0..m), or -1
PAMG_DP_HD int member(const int *S, int m, int col)
{
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (S[mid] < col) lo = mid + 1;
        else hi = mid;
    }
    return (lo < m && S[lo] == col) ? lo : -1;
}

// amg_core::extract_subblocks walks a sorted row with a cursor into the subdomain list that moves past a member once it is
// matched: of several stored entries with one column the FIRST is copied.  In a sorted row they are neighbours.
PAMG_DP_HD bool first_stored(const int *Aj, int row_begin, int k) { return k == row_begin || Aj[k - 1] != Aj[k]; }

// where entry k of row `row_begin..` lands in the m x m block of a subdomain (column position), or -1: not copied
PAMG_DP_HD int extract_target(const int *Aj, int row_begin, int k, const int *S, int m)
{
    if (!first_stored(Aj, row_begin, k)) return -1;
    return member(S, m, Aj[k]);
}

template <typename T>
struct Rotation {
    T c, s;
    bool on;        // false: the pair counts as orthogonal, nothing is applied
};

// relative size of u_j . u_k below which a pair is left alone
template <typename T>
PAMG_DP_HD T pair_tolerance(int m) { return std::sqrt((T)m) * std::numeric_limits<T>::epsilon(); }

// squared column norm below which a column is rounding noise of a rank-deficient block (fro2 = |B|_F^2, which rotations keep):
// such a column is far below every rank tolerance in use and is dropped anyway; rotating against it never settles
template <typename T>
PAMG_DP_HD T noise_floor2(int m, T fro2)
{
    const T e = std::numeric_limits<T>::epsilon();
    return ((T)m * e) * e * fro2;
}

// the rotation of columns j, k from aa = u_j . u_j, bb = u_k . u_k, d = u_j . u_k
template <typename T>
PAMG_DP_HD Rotation<T> rotation(T aa, T bb, T d, T tol, T floor2)
{
    Rotation<T> r;
    r.c = T(1);
    r.s = T(0);
    r.on = false;
    if (aa <= floor2 || bb <= floor2) return r;
    const T nd = std::fabs(d);
    if (nd <= tol * (std::sqrt(aa) * std::sqrt(bb))) return r;
    const T zeta = (bb - aa) / (T(2) * d);
    const T t = (zeta < T(0) ? T(-1) : T(1)) / (std::fabs(zeta) + std::sqrt(T(1) + zeta * zeta));
    r.c = T(1) / std::sqrt(T(1) + t * t);
    r.s = r.c * t;
    r.on = true;
    return r;
}

// one row of the pair: (xj, xk) <- (c xj - s xk, s xj + c xk), separate multiplies and adds
template <typename T>
PAMG_DP_HD void rotate(T &xj, T &xk, T c, T s)
{
    const T a = xj, b = xk;
    xj = c * a - s * b;
    xk = s * a + c * b;
}

// a singular value is kept when it is above rank_tol * sigma_max (gelss: S(i) > rcond * S(1))
template <typename T>
PAMG_DP_HD bool kept(T sigma, T sigma_max, T rank_tol) { return sigma > rank_tol * sigma_max; }

// the cross-lane sum of a group of W lanes: for off = W/2, W/4, ..., 1 every lane adds the value of lane ^ off.  All lanes
// end with the same sum; a host replay that walks the same offsets gets the device's bits.
template <int W, typename F>
PAMG_DP_HD void butterfly_offsets(F &&step)
{
    for (int off = W / 2; off > 0; off >>= 1) step(off);
}

}  // namespace dpinv
}  // namespace pamg
