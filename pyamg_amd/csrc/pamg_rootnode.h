// pamg_rootnode.h -- the per-lane arithmetic of the root-node setup pieces (pamg_rootnode.hip): amg_core::calc_BtB
// (smoothed_aggregation.h:829-907), the pseudo-inverse behind compute_BtBinv and scale_T (util/linalg.py:556-617) and the block
// product of scale_T (util/utils.py:1345-1381).  Plain scalar C++ for the host and the device: tests/rootnode_emul.cpp replays the
// kernels with the lanes as a loop.  Everything is float64; the build compiles with -ffp-contract=off, so a product is rounded before
// it is added.
#pragma once
#include <cstdint>

#include "pamg_jacobi_svd.h"

#if defined(__HIPCC__)
#define PAMG_RN_HD __host__ __device__ inline
#else
#define PAMG_RN_HD inline
#endif

namespace pamg {
namespace rootnode {

constexpr int MAX_BLOCK = 6;            // columns per block of the pattern, and the square blocks of T
constexpr int MAX_NULLDIM = 6;
constexpr int MAX_TRI = MAX_NULLDIM * (MAX_NULLDIM + 1) / 2;

PAMG_RN_HD int tri_count(int K) { return K * (K + 1) / 2; }

// entry t of the upper triangle in the reference's order of Bsq's columns: (0,0) (0,1) .. (0,K-1) (1,1) ..
PAMG_RN_HD void tri_entry(int K, int t, int *i, int *j)
{
    int row = 0, left = t;
    while (left >= K - row) {
        left -= K - row;
        ++row;
    }
    *i = row;
    *j = row + left;
}

// where one product conj(B[k, i]) * B[k, j] comes from: the caller's Bsq (amg_core.calc_BtB's argument) ...
struct Squares {
    const double *b;
    int cols;
    PAMG_RN_HD double operator()(int64_t k, int t, int, int) const { return b[k * cols + t]; }
};
// ... or B itself: one rounded product, the value Bsq would hold
struct Candidates {
    const double *B;
    int K;
    PAMG_RN_HD double operator()(int64_t k, int, int i, int j) const { return B[k * K + i] * B[k * K + j]; }
};

// entry (i, j) of BtB of one node: the pattern row's stored blocks in stored order, the columns of a block ascending -- the reference's
// one accumulator per entry, so the sum is the reference's bit for bit whatever the row holds (unsorted, a column twice, nothing)
template <class Product>
PAMG_RN_HD double btb_entry(const Product &prod, int t, int i, int j, const int *Sp, const int *Sj, int node, int cols_per_block)
{
    double acc = 0.0;
    for (int p = Sp[node]; p < Sp[node + 1]; ++p) {
        const int64_t k0 = (int64_t)Sj[p] * cols_per_block;
        for (int64_t k = k0; k < k0 + cols_per_block; ++k) acc += prod(k, t, i, j);
    }
    return acc;
}

// the lane of entry t of a node's group: BtB is real and symmetric, the entry goes to both places of the column-major block
template <class Product>
PAMG_RN_HD void btb_lane(const Product &prod, int K, int t, const int *Sp, const int *Sj, int node, int cols_per_block, double *BtB)
{
    int i, j;
    tri_entry(K, t, &i, &j);
    const double v = btb_entry(prod, t, i, j, Sp, Sj, node, cols_per_block);
    double *blk = BtB + (int64_t)node * K * K;
    blk[i * K + j] = v;
    blk[j * K + i] = v;
}

// pinv_array on one n x n block, in place, by one lane.  `a` is row-major (what a[kk] is in Python).  n == 1: the reference's rule,
// reciprocal and zero stays zero (linalg.py:590-596).  n > 1: the one-sided Jacobi SVD, a singular value kept when it is above
// rank_tol * sigma_max (gelss' cond), X = sum over the kept k of v_k u_k^T / sigma_k: LAPACK's result to rounding.
PAMG_RN_HD void pinv_block(double *a, int n, double rank_tol)
{
    if (n == 1) {
        a[0] = a[0] == 0.0 ? 0.0 : 1.0 / a[0];
        return;
    }
    JacobiSvd<double, MAX_BLOCK> sv;
    sv.n = n;
    double in[MAX_BLOCK * MAX_BLOCK];
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) in[c * n + r] = a[r * n + c];
    sv.run(in);
    double smax = 0.0;
    for (int k = 0; k < n; ++k) smax = sv.S[k] > smax ? sv.S[k] : smax;
    double w[MAX_BLOCK];
    for (int k = 0; k < n; ++k) w[k] = sv.S[k] > rank_tol * smax ? 1.0 / sv.S[k] : 0.0;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            double acc = 0.0;
            for (int k = 0; k < n; ++k) acc += (sv.V[k * n + r] * w[k]) * sv.U[k * n + c];
            a[r * n + c] = acc;
        }
}

// util/params.py set_tol for float64
PAMG_RN_HD double rank_tol_f64() { return 1e6 * 2.220446049250313e-16; }

// D = P_I.T @ T for an aggregate whose root row holds one block: SciPy's product with the identity block, 0.0 + 1.0 * t (a negative
// zero comes out positive)
PAMG_RN_HD void gather_root_block(const double *Tx, int64_t pos, int bs, double *D)
{
    for (int q = 0; q < bs * bs; ++q) D[q] = 0.0 + Tx[pos * bs * bs + q];
}

// element e of (T @ D) + the injection: a stored block (i, a) of T times the one block of D's row a, in the order of SciPy's gemm (from
// 0.0, k ascending); a root row gets the injected identity instead
PAMG_RN_HD double scale_element(int64_t e, int bs, const int *Tj, const double *Tx, const double *D, const unsigned char *is_root,
                                const int *row_of)
{
    const int bb = bs * bs;
    const int64_t p = e / bb;
    const int r = (int)(e % bb) / bs, c = (int)(e % bb) % bs;
    if (is_root[row_of[p]]) return r == c ? 1.0 : 0.0;
    const double *t = Tx + p * bb + r * bs, *d = D + (int64_t)Tj[p] * bb + c;
    double dot = 0.0;
    for (int k = 0; k < bs; ++k) dot += t[k] * d[k * bs];
    return dot;
}

// filter_operator's `A @ B - Bf`: one element, the product row already summed
PAMG_RN_HD double constraint_defect(double ab, double bf) { return ab - bf; }

}  // namespace rootnode
}  // namespace pamg
