// Host replay of pyamg_amd/csrc/pamg_evolution.hip: the same per-row / per-entry arithmetic (pamg_evolution.h), the lanes of a group, the
// groups of a workgroup and the workgroups of a grid as loops.  Built by tests/test_evolution_host.py with
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC
// and, with -DEVE_MAIN, as a program of its own for the sanitizers.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../pyamg_amd/csrc/pamg_evolution.h"

using namespace pamg;

namespace {
constexpr int BLK = 256, GW = 16, HBLK = 64, GRID = 3;      // a small grid, so that the grid-stride loops are taken
}

extern "C" {

void eve_imm(int n, const int *Ap, const int *Aj, const double *Ax, const int *Bp, const int *Bj, const double *Bx, const int *Sp, const int *Sj,
             double *Sx)
{
    for (int block = 0; block < GRID; ++block)
        for (int t = 0; t < BLK; ++t) {
            const int lane = t % GW;
            for (int64_t row = ((int64_t)block * BLK + t) / GW; row < n; row += (int64_t)GRID * (BLK / GW)) {
                const int r1 = Sp[row + 1];
                for (int p = Sp[row] + lane; p < r1; p += GW) Sx[p] = evo::inner(Ap, Aj, Ax, Bp, Bj, Bx, (int)row, Sj[p]);
            }
        }
}

// 0, or 2 for a NullDim the device path does not take (PAMG_E_UNSUPPORTED)
int eve_helper(double *Sx, const int *Sp, const int *Sj, int nrows, const double *B, const double *DB, const double *BDB, int NullDim, double tol)
{
    if (NullDim < 1 || NullDim > evo::MAX_NULLDIM) return 2;
    for (int block = 0; block < GRID; ++block)
        for (int t = 0; t < HBLK; ++t)
            for (int64_t i = (int64_t)block * HBLK + t; i < nrows; i += (int64_t)GRID * HBLK) {
                switch (NullDim) {
                case 1: evo::helper_row<2>((int)i, Sx, Sp, Sj, nrows, B, DB, BDB, tol); break;
                case 2: evo::helper_row<3>((int)i, Sx, Sp, Sj, nrows, B, DB, BDB, tol); break;
                case 3: evo::helper_row<4>((int)i, Sx, Sp, Sj, nrows, B, DB, BDB, tol); break;
                case 4: evo::helper_row<5>((int)i, Sx, Sp, Sj, nrows, B, DB, BDB, tol); break;
                case 5: evo::helper_row<6>((int)i, Sx, Sp, Sj, nrows, B, DB, BDB, tol); break;
                default: evo::helper_row<7>((int)i, Sx, Sp, Sj, nrows, B, DB, BDB, tol); break;
                }
            }
    return 0;
}

void eve_distance(int relative, int n, double epsilon, const int *Sp, const int *Sj, double *Sx)
{
    for (int block = 0; block < GRID; ++block)
        for (int t = 0; t < BLK; ++t)
            for (int64_t i = (int64_t)block * BLK + t; i < n; i += (int64_t)GRID * BLK) {
                if (relative) evo::distance_row<true>((int)i, epsilon, Sp, Sj, Sx);
                else evo::distance_row<false>((int)i, epsilon, Sp, Sj, Sx);
            }
}

void eve_min_blocks(int n_blocks, int blocksize, const double *Sx, double *Tx)
{
    for (int64_t i = 0; i < n_blocks; ++i) Tx[i] = evo::block_min(Sx + i * blocksize, blocksize);
}

void eve_vector(double *Sx, const int *Sp, const int *Sj, int n, const double *d, const double *b)
{
    for (int block = 0; block < GRID; ++block)
        for (int t = 0; t < BLK; ++t) {
            const int lane = t % GW;
            for (int64_t row = ((int64_t)block * BLK + t) / GW; row < n; row += (int64_t)GRID * (BLK / GW)) {
                const int r1 = Sp[row + 1];
                for (int p = Sp[row] + lane; p < r1; p += GW) Sx[p] = evo::vector_entry(Sx[p], d[row], b[row], b[Sj[p]]);
            }
        }
}

}  // extern "C"

#ifdef EVE_MAIN
// Two fixture-like cases through every routine: a 9 x 7 five-point operator (product, one candidate, filters) and the same grid with
// six candidates, one of which vanishes, and rows shortened below NullDim (helper: the singular system and the all-strong shortcut).
int main()
{
    const int nx = 9, ny = 7, n = nx * ny;
    std::vector<int> Ap(1, 0), Aj;
    std::vector<double> Ax;
    for (int i = 0; i < n; ++i) {
        const int x = i % nx, y = i / nx;
        if (y > 0) { Aj.push_back(i - nx); Ax.push_back(-0.21); }
        if (x > 0) { Aj.push_back(i - 1); Ax.push_back(-0.27); }
        if (i != 5) { Aj.push_back(i); Ax.push_back(0.5 + 0.01 * (i % 5)); }
        if (x < nx - 1) { Aj.push_back(i + 1); Ax.push_back(-0.23); }
        if (y < ny - 1) { Aj.push_back(i + nx); Ax.push_back(-0.29); }
        Ap.push_back((int)Aj.size());
    }
    const int nnz = Ap[n];
    // the CSC form of the same matrix
    std::vector<int> Bp(n + 1, 0), Bj(nnz);
    std::vector<double> Bx(nnz);
    for (int p = 0; p < nnz; ++p) ++Bp[Aj[p] + 1];
    for (int i = 0; i < n; ++i) Bp[i + 1] += Bp[i];
    std::vector<int> fill(Bp.begin(), Bp.end() - 1);
    for (int i = 0; i < n; ++i) for (int p = Ap[i]; p < Ap[i + 1]; ++p) { Bj[fill[Aj[p]]] = i; Bx[fill[Aj[p]]++] = Ax[p]; }
    std::vector<double> Sx(nnz, -1.0);
    eve_imm(n, Ap.data(), Aj.data(), Ax.data(), Bp.data(), Bj.data(), Bx.data(), Ap.data(), Aj.data(), Sx.data());
    double check = 0.0;
    for (double v : Sx) check += v;
    std::vector<double> d(n, 0.0), b(n, 1.0), V(Sx);
    for (int i = 0; i < n; ++i) { b[i] = 1.0 + 0.1 * (i % 3); for (int p = Ap[i]; p < Ap[i + 1]; ++p) if (Aj[p] == i) d[i] = Sx[p]; }
    eve_vector(V.data(), Ap.data(), Aj.data(), n, d.data(), b.data());
    eve_distance(1, n, 2.0, Ap.data(), Aj.data(), V.data());
    eve_distance(0, n, 4.0, Ap.data(), Aj.data(), V.data());
    std::vector<double> T(nnz / 4);
    eve_min_blocks(nnz / 4, 4, V.data(), T.data());
    for (double v : T) check += v < 1e300 ? v : 0.0;
    for (int K = 1; K <= 6; ++K) {
        const int cols = K * (K + 1) / 2;
        std::vector<double> B((size_t)n * K), DB((size_t)n * K), BDB((size_t)n * cols), H(Sx);
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < K; ++k) {
                const double v = k == K - 1 && K > 1 ? 0.0 : (k == 0 ? 1.0 : 0.3 * k + 0.01 * ((i * (k + 1)) % 7));     // the last candidate vanishes
                B[(size_t)i * K + k] = v;
                DB[(size_t)k * n + i] = v;
            }
        for (int i = 0; i < n; ++i) {
            int c = 0;
            for (int a = 0; a < K; ++a) for (int e = a; e < K; ++e) BDB[(size_t)i * cols + c++] = 2.0 * (B[(size_t)i * K + a] * B[(size_t)i * K + e]);
        }
        if (eve_helper(H.data(), Ap.data(), Aj.data(), n, B.data(), DB.data(), BDB.data(), K, 2.220446049250313e-10) != 0) return 1;
        for (double v : H) check += v;
    }
    if (!(check == check)) { std::printf("nan\n"); return 1; }
    std::printf("%.17g\nok\n", check);
    return 0;
}
#endif
