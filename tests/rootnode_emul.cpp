// rootnode_emul.cpp -- host replay of pyamg_amd/csrc/pamg_rootnode.hip: the same per-lane functions (pamg_rootnode.h, and pamg_energy.h for
// filter_operator's projection), the lanes of a group as a loop, a workgroup barrier as the end of that loop.  Built by
// tests/test_rootnode_host.py with the host compiler and -ffp-contract=off; the arguments are those of the C entry points.
// Returns 0, -1 for bad arguments, -2 for what the device path does not take.
#include <cstdint>
#include <vector>

#include "../pyamg_amd/csrc/pamg_energy.h"
#include "../pyamg_amd/csrc/pamg_rootnode.h"

using namespace pamg;

namespace {

constexpr int GW = 8;          // the group width of the replay; the results do not depend on it

bool pattern_ok(int n, int ncol, const int *Sp, const int *Sj)
{
    if (n < 0 || Sp[0] != 0) return false;
    for (int i = 0; i < n; ++i) if (Sp[i + 1] < Sp[i]) return false;
    for (int p = 0; p < Sp[n]; ++p) if (Sj[p] < 0 || Sj[p] >= ncol) return false;
    return true;
}

}  // namespace

extern "C" {

int rn_calc_BtB(int K, int n, int cpb, const double *b, int b_size, int BsqCols, double *x, const int *Sp, const int *Sj)
{
    if (K < 1 || cpb < 1) return -1;
    if (K > rootnode::MAX_NULLDIM || cpb > rootnode::MAX_BLOCK) return -2;
    if (BsqCols != rootnode::tri_count(K) || b_size % (BsqCols * cpb) || !pattern_ok(n, b_size / (BsqCols * cpb), Sp, Sj)) return -1;
    const rootnode::Squares prod{b, BsqCols};
    for (int node = 0; node < n; ++node)
        for (int lane = 0; lane < rootnode::tri_count(K); ++lane) rootnode::btb_lane(prod, K, lane, Sp, Sj, node, cpb, x);
    return 0;
}

// BtB (may be null) <- the blocks before the inversion, as calc_BtB leaves them
int rn_compute_BtBinv(int K, int n, int cpb, const double *B, int64_t B_size, const int *Sp, const int *Sj, double *BtB, double *BtBinv)
{
    if (K < 1 || cpb < 1) return -1;
    if (K > rootnode::MAX_NULLDIM || cpb > rootnode::MAX_BLOCK) return -2;
    if (B_size % (K * cpb) || !pattern_ok(n, (int)(B_size / (K * cpb)), Sp, Sj)) return -1;
    const rootnode::Candidates prod{B, K};
    for (int node = 0; node < n; ++node)
        for (int lane = 0; lane < rootnode::tri_count(K); ++lane) rootnode::btb_lane(prod, K, lane, Sp, Sj, node, cpb, BtBinv);
    if (BtB) for (int64_t q = 0; q < (int64_t)n * K * K; ++q) BtB[q] = BtBinv[q];
    for (int node = 0; node < n; ++node) {
        double *a = BtBinv + (int64_t)node * K * K;
        for (int r = 0; r < K; ++r)
            for (int c = r + 1; c < K; ++c) {
                const double up = a[r * K + c];
                a[r * K + c] = a[c * K + r];
                a[c * K + r] = up;
            }
        rootnode::pinv_block(a, K, rootnode::rank_tol_f64());
    }
    return 0;
}

int rn_filter_constraints(int r, int c, int n, int K, const double *B, int B_size, const double *Bf, const double *BtBinv, const int *Sp,
                          const int *Sj, double *Sx)
{
    if (r < 1 || c < 1 || K < 1) return -1;
    if (r > rootnode::MAX_BLOCK || c > rootnode::MAX_BLOCK || K > rootnode::MAX_NULLDIM) return -2;
    if (B_size % (c * K) || !pattern_ok(n, B_size / (c * K), Sp, Sj)) return -1;
    double ub[rootnode::MAX_BLOCK * rootnode::MAX_NULLDIM];
    for (int row = 0; row < n; ++row) {
        for (int lane = 0; lane < GW; ++lane) {
            energy::ub_lane(lane, GW, row, Sp, Sj, Sx, B, ub, r, c, K);
            for (int q = lane; q < r * K; q += GW) ub[q] = rootnode::constraint_defect(ub[q], Bf[(int64_t)row * r * K + q]);
        }
        for (int lane = 0; lane < GW; ++lane) energy::project_lane(lane, GW, row, Sp, Sj, Sx, ub, BtBinv, B, r, c, K);
    }
    return 0;
}

int rn_scale_T(int n, int n_bcol, int bs, const int *Tp, const int *Tj, double *Tx, const int *Cnodes)
{
    if (bs < 1 || n < 0 || n_bcol < 0) return -1;
    if (bs > rootnode::MAX_BLOCK) return -2;
    if (!pattern_ok(n, n_bcol, Tp, Tj)) return -1;
    std::vector<unsigned char> is_root((size_t)n, 0);
    for (int a = 0; a < n_bcol; ++a) {
        const int r = Cnodes[a];
        if (r < 0 || r >= n || is_root[r]) return -1;
        if (Tp[r + 1] - Tp[r] != 1 || Tj[Tp[r]] != a) return -2;
        is_root[r] = 1;
    }
    const int64_t nnz = Tp[n], E = nnz * bs * bs;
    std::vector<int> row_of((size_t)nnz);
    for (int i = 0; i < n; ++i)
        for (int p = Tp[i]; p < Tp[i + 1]; ++p) row_of[p] = i;
    std::vector<double> D((size_t)n_bcol * bs * bs), out((size_t)E);
    for (int a = 0; a < n_bcol; ++a) {
        double *d = D.data() + (int64_t)a * bs * bs;
        rootnode::gather_root_block(Tx, Tp[Cnodes[a]], bs, d);
        rootnode::pinv_block(d, bs, rootnode::rank_tol_f64());
    }
    for (int64_t e = 0; e < E; ++e) out[e] = rootnode::scale_element(e, bs, Tj, Tx, D.data(), is_root.data(), row_of.data());
    for (int64_t e = 0; e < E; ++e) Tx[e] = out[e];
    return 0;
}

}  // extern "C"
