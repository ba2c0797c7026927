// Host replay of the GMRES driver of pyamg_amd/csrc/pamg_energy.hip (pamg_energy_gmres_f64): the same per-lane phases and the same
// Krylov-side step functions (pamg_energy.h), the lanes of a group as loops, a phase run for every lane before the next (the workgroup
// barrier), the reduction tree lane by lane.  gw = 0 takes the group width the device would take.  Built by
// tests/test_energy_gmres_host.py with
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC
// and, with -DEGE_MAIN, as a program of its own for the sanitizers.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../pyamg_amd/csrc/pamg_energy.h"

using namespace pamg;

namespace {

// the two-level tree of reduce_chunks_kernel / gmres_step_kernel
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

struct Problem {
    int gw, n, r, c, K;
    const int *Ap, *Aj;
    const double *Ax;
    const int *Sp, *Sj;
    const double *Bc, *BtBinv, *Dinv;
};

// gmres_product_kernel
void product(const Problem &P, const double *In, double *Out, const double *With, bool negate, std::vector<double> &rowsum)
{
    double ub[energy::MAX_BLOCK * energy::MAX_NULLDIM];
    for (int i = 0; i < P.n; ++i) {
        for (int lane = 0; lane < P.gw; ++lane)
            energy::imm_scaled_lane(lane, P.gw, i, P.Ap, P.Aj, P.Ax, energy::StoredBlocks{In, P.r, P.c}, P.Sp, P.Sj, P.Dinv, Out, negate, P.r, P.c);
        for (int lane = 0; lane < P.gw; ++lane) energy::ub_lane(lane, P.gw, i, P.Sp, P.Sj, Out, P.Bc, ub, P.r, P.c, P.K);
        for (int lane = 0; lane < P.gw; ++lane) energy::project_lane(lane, P.gw, i, P.Sp, P.Sj, Out, ub, P.BtBinv, P.Bc, P.r, P.c, P.K);
        rowsum[(size_t)i] = energy::row_dot(With, Out, (int64_t)P.Sp[i] * P.r * P.c, (int64_t)P.Sp[i + 1] * P.r * P.c);
    }
}

}  // namespace

extern "C" {

// 0, or 2 for what the device path does not take.  normrs: room for maxiter + 1 values; H: (maxiter + 1)^2 values or NULL
int ege_gmres(int gw, int n, int nbc, int r, int c, int K, const int *Ap, const int *Aj, const double *Ax, const int *Sp, const int *Sj, double *T,
              const double *Bc, const double *BtBinv, const double *Dinv, const unsigned char *cmask, const double *PI, int maxiter, double tol,
              int *iterations, double *normrs, int *n_normrs, double *H)
{
    (void)nbc;
    if (r > energy::MAX_BLOCK || c > energy::MAX_BLOCK || K > energy::MAX_NULLDIM || maxiter > energy::GMRES_MAXITER) return 2;
    *iterations = 0;
    *n_normrs = 0;
    const int64_t E = (int64_t)Sp[n] * r * c;
    if (n == 0 || E == 0) return 0;
    if (gw <= 0) gw = energy::group_width(E, n);
    const Problem P{gw, n, r, c, K, Ap, Aj, Ax, Sp, Sj, Bc, BtBinv, Dinv};
    std::vector<double> V((size_t)E * (size_t)(maxiter + 1)), rowsum((size_t)n);
    std::vector<energy::GmresState> state(1);               // (value-initialised: the hipMemset of the driver)
    energy::GmresState &S = state[0];
    auto basis = [&](int j) { return V.data() + (int64_t)j * E; };
    auto scale = [&](double *X) {                           // gmres_scale_kernel
        if (!S.scaled) return;
        for (int i = 0; i < n; ++i)
            for (int lane = 0; lane < gw; ++lane) energy::scale_lane(lane, gw, i, Sp, X, S.scale, r, c);
    };
    product(P, T, basis(0), basis(0), true, rowsum);
    energy::gmres_start(S, tree_sum(rowsum), maxiter, tol);
    scale(basis(0));
    for (int i = 0; i < maxiter; ++i) {
        if (S.stop) break;
        double *W = basis(i + 1);
        product(P, basis(i), W, basis(0), false, rowsum);
        energy::gmres_coefficient(S, 0, i, tree_sum(rowsum));
        for (int j = 0; j <= i; ++j) {                       // gmres_mgs_kernel
            const double *Next = j < i ? basis(j + 1) : W;
            for (int q = 0; q < n; ++q) {
                for (int lane = 0; lane < gw; ++lane) energy::mgs_lane(lane, gw, q, Sp, W, basis(j), S.h, r, c);
                rowsum[(size_t)q] = energy::row_dot(Next, W, (int64_t)Sp[q] * r * c, (int64_t)Sp[q + 1] * r * c);
            }
            if (j < i) energy::gmres_coefficient(S, j + 1, i, tree_sum(rowsum));
            else energy::gmres_column(S, i, tree_sum(rowsum), maxiter, tol);
        }
        scale(W);
    }
    const int its = S.iterations;
    double y[energy::GMRES_MAXITER] = {0.0};
    if (its > 0) energy::gmres_solve(S, its, y);
    if (its > 0 || cmask)                                    // gmres_combine_kernel
        for (int i = 0; i < n; ++i)
            for (int lane = 0; lane < gw; ++lane) energy::combine_lane(lane, gw, i, Sp, T, V.data(), E, y, its, cmask, PI, r, c);
    for (int q = 0; q <= its; ++q) normrs[q] = S.normr[q];
    if (H)
        for (int a = 0; a <= maxiter; ++a)
            for (int b = 0; b <= maxiter; ++b) H[a * (maxiter + 1) + b] = S.H[a * energy::GMRES_LD + b];
    *iterations = its;
    *n_normrs = its + 1;
    return 0;
}

}  // extern "C"

#ifdef EGE_MAIN
// An 11 x 9 first-order upwind convection-diffusion operator in 2 x 2 blocks (not symmetric), a block-diagonal tentative T of 2 x 3
// blocks on 3-node aggregates, the pattern A's structure times T's: GMRES with group widths 1 and the device's, with and without
// C-point rows, then the paths that leave early -- a tolerance above the initial norm, maxiter 0, and a residual that is zero (the
// breakdown's neighbour: nothing to normalise).
int main()
{
    const int nx = 11, ny = 9, n = nx * ny, r = 2, c = 3, K = 3, nagg = (n + 2) / 3;
    std::vector<int> Ap(1, 0), Aj;
    std::vector<double> Ax;
    for (int i = 0; i < n; ++i) {
        const int x = i % nx, y = i / nx;
        const int nb[5] = {y > 0 ? i - nx : -1, x > 0 ? i - 1 : -1, i, x < nx - 1 ? i + 1 : -1, y < ny - 1 ? i + nx : -1};
        const double w[5] = {-0.01 - 0.59, -0.01 - 0.81, 0.04 + 1.4, -0.01, -0.01};       // diffusion 0.01, flow from the lower left
        for (int q = 0; q < 5; ++q) {
            if (nb[q] < 0) continue;
            Aj.push_back(nb[q]);
            const double blk[4] = {w[q], 0.02 * (q + 1), -0.01 * (q + 1), w[q] * 0.9};
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
    for (size_t q = 0; q < Dinv.size(); ++q) Dinv[q] = 1.0 / (2.8 + (double)(q % 3));
    for (int i = 0; i < n; i += 3) {                         // every third node a C point: identity-like injection in its own block
        cmask[(size_t)i * r] = cmask[(size_t)i * r + 1] = 1;
        for (int p = Sp[i]; p < Sp[i + 1]; ++p) if (Sj[p] == i / 3) { PI[(size_t)p * r * c] = 1.0; PI[(size_t)p * r * c + c + 1] = 1.0; }
    }
    auto run = [&](int gw, bool rooted, const std::vector<double> &Tin, int maxiter, double tol, std::vector<double> &T, std::vector<double> &nr,
                   int &its) {
        T = Tin;
        nr.assign((size_t)maxiter + 1, -1.0);
        std::vector<double> H((size_t)(maxiter + 1) * (size_t)(maxiter + 1));
        int ns = 0;
        const int rc = ege_gmres(gw, n, nagg, r, c, K, Ap.data(), Aj.data(), Ax.data(), Sp.data(), Sj.data(), T.data(), Bc.data(), BtBinv.data(),
                                 Dinv.data(), rooted ? cmask.data() : nullptr, rooted ? PI.data() : nullptr, maxiter, tol, &its, nr.data(), &ns,
                                 H.data());
        nr.resize((size_t)ns);
        return rc;
    };
    double check = 0.0;
    std::vector<double> T, nr, T1, nr1;
    int its = 0;
    for (int rooted = 0; rooted < 2; ++rooted) {
        if (run(1, rooted, T0, 4, 1e-12, T1, nr1, its) || its != 4 || nr1.size() != 5) { std::printf("gw 1: iterations %d\n", its); return 1; }
        if (run(0, rooted, T0, 4, 1e-12, T, nr, its) || its != 4 || T != T1 || nr != nr1) { std::printf("the group width moved a bit\n"); return 1; }
        for (size_t q = 1; q < nr.size(); ++q) if (!(nr[q] < nr[q - 1])) { std::printf("normr does not fall\n"); return 1; }
        for (double v : T) check += v;
        if (run(0, rooted, T0, 32, 1e-12, T, nr, its) || its < 4) { std::printf("maxiter 32: iterations %d\n", its); return 1; }
        for (double v : T) check += v;
    }
    if (run(0, 1, T0, 4, 1e300, T, nr, its) || its != 0 || nr.size() != 1) { std::printf("tol above the norm: iterations %d\n", its); return 1; }
    for (int i = 0; i < n; ++i)                              // T unchanged on F rows, the injection on C rows
        for (int e = Sp[i] * r * c; e < Sp[i + 1] * r * c; ++e) {
            const int a = (e % (r * c)) / c;
            if (T[(size_t)e] != (cmask[(size_t)i * r + a] ? PI[(size_t)e] : T0[(size_t)e])) { std::printf("no iteration: T moved\n"); return 1; }
        }
    if (run(0, 0, T0, 0, 1e-12, T, nr, its) || its != 0 || T != T0) { std::printf("maxiter 0\n"); return 1; }
    const std::vector<double> Z((size_t)E, 0.0);             // T = 0: R = 0, normr = 0.0, no basis vector, no iteration
    if (run(0, 0, Z, 4, 0.0, T, nr, its) || its != 0 || nr.size() != 1 || nr[0] != 0.0 || T != Z) { std::printf("zero residual\n"); return 1; }
    if (run(0, 0, T0, 33, 1e-12, T, nr, its) != 2) { std::printf("maxiter 33 was taken\n"); return 1; }
    // the breakdown branch itself, on the step function: a column whose remainder is exactly zero leaves no rotation and normr = 0.0
    std::vector<energy::GmresState> st(1);
    energy::gmres_start(st[0], 4.0, 4, 1e-12);
    energy::gmres_coefficient(st[0], 0, 0, 0.75);
    energy::gmres_column(st[0], 0, 0.0, 4, 1e-12);
    if (st[0].scaled || st[0].nq != 0 || st[0].normr[1] != 0.0 || !st[0].stop || st[0].iterations != 1 || st[0].H[0] != 0.75 || st[0].g[0] != 2.0) {
        std::printf("breakdown\n");
        return 1;
    }
    double y[1];
    energy::gmres_solve(st[0], 1, y);
    check += y[0];
    if (!(check == check)) { std::printf("nan\n"); return 1; }
    std::printf("%.17g\nok\n", check);
    return 0;
}
#endif
