// Host replay of pyamg_amd/csrc/pamg_energy.hip: the same per-lane phases (pamg_energy.h), the lanes of a group as loops, a phase run
// for every lane before the next (the workgroup barrier), the reduction tree lane by lane.  gw = 0 takes the group width the device
// would take; gw = 1 is the single-lane run the group boundaries are checked against.  Built by tests/test_energy_host.py with
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC
// and, with -DENE_MAIN, as a program of its own for the sanitizers.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../pyamg_amd/csrc/pamg_energy.h"

using namespace pamg;

namespace {

int width(int gw, int64_t elements, int n) { return gw > 0 ? gw : energy::group_width(elements, n); }

// the two-level tree of reduce_chunks_kernel / reduce_final_kernel
double tree_sum(const std::vector<double> &row)
{
    const int64_t n = (int64_t)row.size(), nchunks = energy::chunks(n);
    std::vector<double> chunk((size_t)nchunks), lane(energy::RED_LANES);
    for (int64_t b = 0; b < nchunks; ++b) {
        for (int t = 0; t < energy::RED_LANES; ++t) lane[t] = energy::lane_partial(row.data(), n, b * energy::RED_CHUNK, t);
        chunk[(size_t)b] = energy::tree_fold(lane.data());
    }
    for (int t = 0; t < energy::RED_LANES; ++t) lane[t] = energy::lane_strided(chunk.data(), nchunks, t);
    return energy::tree_fold(lane.data());
}

void project_row(int gw, int i, const int *Sp, const int *Sj, double *Sx, const double *Bc, const double *BtBinv, int r, int c, int K)
{
    double ub[energy::MAX_BLOCK * energy::MAX_NULLDIM];
    for (int lane = 0; lane < gw; ++lane) energy::ub_lane(lane, gw, i, Sp, Sj, Sx, Bc, ub, r, c, K);
    for (int lane = 0; lane < gw; ++lane) energy::project_lane(lane, gw, i, Sp, Sj, Sx, ub, BtBinv, Bc, r, c, K);
}

}  // namespace

extern "C" {

int ene_imm(int gw, const int *Ap, const int *Aj, const double *Ax, const int *Bp, const int *Bj, const double *Bx, const int *Sp, const int *Sj,
            double *Sx, int n, int r, int m, int c)
{
    if (r > energy::MAX_BLOCK || m > energy::MAX_BLOCK || c > energy::MAX_BLOCK) return 2;
    gw = width(gw, (int64_t)Sp[n] * r * c, n);
    for (int i = 0; i < n; ++i)
        for (int lane = 0; lane < gw; ++lane)
            energy::imm_lane(lane, gw, i, Ap, Aj, Ax, Bp, Bj, energy::StoredBlocks{Bx, m, c}, Sp, Sj, Sx, Sx, false, r, m, c);
    return 0;
}

// UB == nullptr: U @ B here as well (satisfy_constraints); 0, or 2 for a shape the device path does not take
int ene_constraints(int gw, int r, int c, int n, int K, const double *Bc, const double *UB, const double *BtBinv, const int *Sp, const int *Sj,
                    double *Sx)
{
    if (r > energy::MAX_BLOCK || c > energy::MAX_BLOCK || K > energy::MAX_NULLDIM) return 2;
    gw = width(gw, (int64_t)Sp[n] * r * c, n);
    for (int i = 0; i < n; ++i) {
        if (!UB) { project_row(gw, i, Sp, Sj, Sx, Bc, BtBinv, r, c, K); continue; }
        for (int lane = 0; lane < gw; ++lane) energy::project_lane(lane, gw, i, Sp, Sj, Sx, UB + (int64_t)i * r * K, BtBinv, Bc, r, c, K);
    }
    return 0;
}

int ene_cg(int gw, int n, int nbc, int r, int c, int K, const int *Ap, const int *Aj, const double *Ax, const int *Sp, const int *Sj, double *T,
           const double *Bc, const double *BtBinv, const double *Dinv, const unsigned char *cmask, const double *PI, int maxiter, double tol,
           int *iterations, double *newsums, int *n_newsums)
{
    (void)nbc;
    if (r > energy::MAX_BLOCK || c > energy::MAX_BLOCK || K > energy::MAX_NULLDIM) return 2;
    *iterations = 0;
    *n_newsums = 0;
    const int64_t E = (int64_t)Sp[n] * r * c;
    if (n == 0 || E == 0 || maxiter == 0) return 0;
    gw = width(gw, E, n);
    std::vector<double> R((size_t)E), P0((size_t)E), P1((size_t)E), AP((size_t)E), rowsum((size_t)n);
    std::vector<int> nzb((size_t)n);
    double *P[2] = {P0.data(), P1.data()};
    for (int i = 0; i < n; ++i) {                            // cg_init_kernel
        for (int lane = 0; lane < gw; ++lane)
            energy::imm_lane(lane, gw, i, Ap, Aj, Ax, Sp, Sj, energy::StoredBlocks{T, r, c}, Sp, Sj, nullptr, R.data(), true, r, r, c);
        project_row(gw, i, Sp, Sj, R.data(), Bc, BtBinv, r, c, K);
        rowsum[(size_t)i] = energy::row_rz(R.data(), Dinv, i, Sp[i], Sp[i + 1], r, c, &nzb[(size_t)i]);
    }
    const double bs = (double)r * c, resid0 = (double)Sp[n] * bs;
    double newsum = 0.0, oldsum = 0.0, beta = 0.0;
    int it = 0, cur = 0;
    for (; it < maxiter; ++it) {
        const double total = tree_sum(rowsum);               // reduce_final_kernel, what = 0
        long long cnt = 0;
        for (int v : nzb) cnt += v;
        const int stop = energy::cg_stop(it == 0 ? resid0 : (double)cnt * bs, total, tol);
        if (stop != 2) {
            newsum = total;
            newsums[(*n_newsums)++] = total;
        }
        if (stop) break;
        if (it > 0) beta = total / oldsum;
        oldsum = total;
        const energy::Direction dir{R.data(), P[cur], Dinv, &beta, r, c, it == 0 ? 1 : 0};
        double *Pn = P[cur ^ 1];
        for (int i = 0; i < n; ++i) {                        // cg_direction_kernel
            for (int lane = 0; lane < gw; ++lane) {
                energy::pnew_lane(lane, gw, i, Sp, dir, Pn, r, c);
                energy::imm_lane(lane, gw, i, Ap, Aj, Ax, Sp, Sj, dir, Sp, Sj, nullptr, AP.data(), false, r, r, c);
            }
            project_row(gw, i, Sp, Sj, AP.data(), Bc, BtBinv, r, c, K);
            rowsum[(size_t)i] = energy::row_dot(Pn, AP.data(), (int64_t)Sp[i] * r * c, (int64_t)Sp[i + 1] * r * c);
        }
        const double alpha = newsum / tree_sum(rowsum);      // reduce_final_kernel, what = 1
        for (int i = 0; i < n; ++i) {                        // cg_update_kernel
            for (int lane = 0; lane < gw; ++lane) energy::update_lane(lane, gw, i, Sp, T, R.data(), Pn, AP.data(), alpha, cmask, PI, r, c);
            rowsum[(size_t)i] = energy::row_rz(R.data(), Dinv, i, Sp[i], Sp[i + 1], r, c, &nzb[(size_t)i]);
        }
        cur ^= 1;
    }
    *iterations = it;
    return 0;
}

}  // extern "C"

#ifdef ENE_MAIN
// A 9 x 7 five-point operator in 2 x 2 blocks, a block-diagonal tentative T of 2 x 3 blocks on 3-node aggregates, the pattern A's
// structure times T's; every routine once, group widths 1 and the device's, with and without C-point rows.
int main()
{
    const int nx = 9, ny = 7, n = nx * ny, r = 2, c = 3, K = 3, nagg = (n + 2) / 3;
    std::vector<int> Ap(1, 0), Aj;
    std::vector<double> Ax;
    for (int i = 0; i < n; ++i) {
        const int x = i % nx, y = i / nx;
        const int nb[5] = {y > 0 ? i - nx : -1, x > 0 ? i - 1 : -1, i, x < nx - 1 ? i + 1 : -1, y < ny - 1 ? i + nx : -1};
        for (int q = 0; q < 5; ++q) {
            if (nb[q] < 0) continue;
            Aj.push_back(nb[q]);
            const double d = nb[q] == i ? 4.0 : -1.0;
            const double blk[4] = {d, 0.1 * (q + 1), 0.1 * (q + 1), d * 0.9};
            Ax.insert(Ax.end(), blk, blk + 4);
        }
        Ap.push_back((int)Aj.size());
    }
    std::vector<int> Sp(1, 0), Sj;
    for (int i = 0; i < n; ++i) {
        std::vector<char> seen((size_t)nagg, 0);
        for (int p = Ap[i]; p < Ap[i + 1]; ++p) seen[(size_t)(Aj[p] / 3)] = 1;
        for (int a = 0; a < nagg; ++a) if (seen[(size_t)a]) Sj.push_back(a);
        Sp.push_back((int)Sj.size());
    }
    const int nnz = Sp[n], E = nnz * r * c;
    std::vector<double> T0((size_t)E, 0.0), Bc((size_t)nagg * c * K), BtBinv((size_t)n * K * K, 0.0), Dinv((size_t)n * r), PI((size_t)E, 0.0);
    std::vector<unsigned char> cmask((size_t)n * r, 0);
    for (int i = 0; i < n; ++i)
        for (int p = Sp[i]; p < Sp[i + 1]; ++p)
            if (Sj[p] == i / 3)
                for (int q = 0; q < r * c; ++q) T0[(size_t)p * r * c + q] = 0.5 + 0.01 * ((i + q) % 7);
    for (size_t q = 0; q < Bc.size(); ++q) Bc[q] = 1.0 + 0.03 * (double)(q % 11);
    for (int i = 0; i < n; ++i) for (int k = 0; k < K; ++k) BtBinv[((size_t)i * K + k) * K + k] = 0.2 / (1 + k);
    for (size_t q = 0; q < Dinv.size(); ++q) Dinv[q] = 1.0 / (8.0 + (double)(q % 3));
    for (int i = 0; i < n; i += 3) {                         // every third node a C point: identity-like injection in its own block
        cmask[(size_t)i * r] = cmask[(size_t)i * r + 1] = 1;
        for (int p = Sp[i]; p < Sp[i + 1]; ++p) if (Sj[p] == i / 3) { PI[(size_t)p * r * c] = 1.0; PI[(size_t)p * r * c + c + 1] = 1.0; }
    }
    double check = 0.0;
    for (int gw : {1, 0}) {
        std::vector<double> S((size_t)E, 0.25);
        if (ene_imm(gw, Ap.data(), Aj.data(), Ax.data(), Sp.data(), Sj.data(), T0.data(), Sp.data(), Sj.data(), S.data(), n, r, r, c)) return 1;
        if (ene_constraints(gw, r, c, n, K, Bc.data(), nullptr, BtBinv.data(), Sp.data(), Sj.data(), S.data())) return 1;
        std::vector<double> UB((size_t)n * r * K, 0.125);
        if (ene_constraints(gw, r, c, n, K, Bc.data(), UB.data(), BtBinv.data(), Sp.data(), Sj.data(), S.data())) return 1;
        for (double v : S) check += v;
        for (int rooted = 0; rooted < 2; ++rooted) {
            std::vector<double> T(T0), sums(4);
            int its = 0, ns = 0;
            if (ene_cg(gw, n, nagg, r, c, K, Ap.data(), Aj.data(), Ax.data(), Sp.data(), Sj.data(), T.data(), Bc.data(), BtBinv.data(), Dinv.data(),
                       rooted ? cmask.data() : nullptr, rooted ? PI.data() : nullptr, 4, 1e-12, &its, sums.data(), &ns)) return 1;
            if (its != 4 || ns != 4) { std::printf("iterations %d sums %d\n", its, ns); return 1; }
            for (double v : T) check += v;
        }
    }
    if (!(check == check)) { std::printf("nan\n"); return 1; }
    std::printf("%.17g\nok\n", check);
    return 0;
}
#endif
