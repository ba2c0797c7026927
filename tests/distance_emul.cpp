// Host replay of pyamg_amd/csrc/pamg_distance.hip: the same per-row / per-entry arithmetic (pamg_distance.h), the lanes of a group, the
// groups of a workgroup and the workgroups of a grid as loops, the block of vectors interleaved as on the device.  Built by
// tests/test_distance_host.py with
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC
// and, with -DDSE_MAIN, as a program of its own for the sanitizers.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../pyamg_amd/csrc/pamg_distance.h"

using namespace pamg;

namespace {
constexpr int BLK = 256, GW = 16, GN = 8, GN_ROW = 7, GRID = 3;        // a small grid, so that the grid-stride loops are taken

void records(bool to_records, int n, int R, const double *src, double *dst)
{
    const int64_t total = (int64_t)n * R;
    for (int block = 0; block < GRID; ++block)
        for (int th = 0; th < BLK; ++th)
            for (int64_t t = (int64_t)block * BLK + th; t < total; t += (int64_t)GRID * BLK) {
                const int64_t i = t / R, r = t - i * R;
                if (to_records) dst[t] = src[r * n + i];
                else dst[r * n + i] = src[t];
            }
}

// k sweeps between the two buffers; returns the one that holds the result
double *sweeps(int n, int R, int k, double omega, const int *Ap, const int *Aj, const double *Ax, double *a, double *b)
{
    const int64_t total = (int64_t)n * R;
    for (int s = 0; s < k; ++s) {
        for (int block = 0; block < GRID; ++block)
            for (int th = 0; th < BLK; ++th)
                for (int64_t t = (int64_t)block * BLK + th; t < total; t += (int64_t)GRID * BLK) {
                    const int i = (int)(t / R), r = (int)(t - (int64_t)i * R);
                    b[t] = dst::relax_value(i, r, R, Ap, Aj, Ax, a, omega);
                }
        std::swap(a, b);
    }
    return a;
}

void measure(bool filter, int measure_, int n, int R, double epsilon, const int *Ap, const int *Aj, const double *Ax, const double *X, double *Dx)
{
    const int G = (int64_t)Ap[n] <= (int64_t)GN_ROW * n ? GN : GW;           // lanes per row, as the launch chooses them
    for (int block = 0; block < GRID; ++block)
        for (int g = 0; g < BLK / G; ++g)
            for (int64_t row = (int64_t)block * (BLK / G) + g; row < n; row += (int64_t)GRID * (BLK / G)) {
                const int r1 = Ap[row + 1];
                for (int lane = 0; lane < G; ++lane)
                    for (int p = Ap[row] + lane; p < r1; p += G) Dx[p] = dst::measure_entry(measure_, R, (int)row, Aj[p], Ax[p], X);
                if (!filter) continue;
                double mn[GW];
                for (int lane = 0; lane < G; ++lane) mn[lane] = dst::row_min((int)row, Ap[row] + lane, r1, G, Aj, Dx);
                for (int m = G / 2; m; m >>= 1) {                           // the butterfly of the group
                    double nx[GW];
                    for (int lane = 0; lane < G; ++lane) nx[lane] = dst::dmin(mn[lane], mn[lane ^ m]);
                    std::copy(nx, nx + G, mn);
                }
                for (int lane = 0; lane < G; ++lane) {
                    const double threshold = epsilon * mn[lane];
                    for (int p = Ap[row] + lane; p < r1; p += G) Dx[p] = dst::tail(Dx[p], threshold);
                }
            }
}

bool known(int m) { return m >= 0 && m <= 3; }
}  // namespace

extern "C" {

// 0, 1 for a bad argument (PAMG_E_ARG), 2 for what the device path does not take (PAMG_E_UNSUPPORTED)
int dse_relaxation_vectors(const int *Ap, const int *Aj, const double *Ax, double *X, int n, int R, int k, double omega)
{
    if (n < 0 || R < 1 || k < 0) return 1;
    if (R > dst::MAX_R) return 2;
    std::vector<double> a((size_t)n * R), b((size_t)n * R);
    records(true, n, R, X, a.data());
    records(false, n, R, sweeps(n, R, k, omega, Ap, Aj, Ax, a.data(), b.data()), X);
    return 0;
}

int dse_distance_measure(int measure_, const int *Ap, const int *Aj, const double *Ax, const double *X, int n, int R, double *Dx)
{
    if (n < 0 || R < 1 || !known(measure_)) return 1;
    if (R > dst::MAX_R) return 2;
    std::vector<double> a((size_t)n * R);
    records(true, n, R, X, a.data());
    measure(false, measure_, n, R, 0.0, Ap, Aj, Ax, a.data(), Dx);
    return 0;
}

int dse_distance_strength(int measure_, const int *Ap, const int *Aj, const double *Ax, double *X, int n, int R, int k, double omega, double epsilon,
                          double *Dx)
{
    if (n < 0 || R < 1 || k < 0 || !known(measure_)) return 1;
    if (R > dst::MAX_R) return 2;
    std::vector<double> a((size_t)n * R), b((size_t)n * R);
    records(true, n, R, X, a.data());
    const double *x = sweeps(n, R, k, omega, Ap, Aj, Ax, a.data(), b.data());
    measure(true, measure_, n, R, epsilon, Ap, Aj, Ax, x, Dx);
    records(false, n, R, x, X);
    return 0;
}

int dse_vertex_distance(const int *Ap, const int *Aj, const double *V, int n, int dim, double *Cx)
{
    if (n < 0 || dim < 1) return 1;
    if (dim > dst::MAX_DIM) return 2;
    for (int block = 0; block < GRID; ++block)
        for (int g = 0; g < BLK / GW; ++g)
            for (int64_t row = (int64_t)block * (BLK / GW) + g; row < n; row += (int64_t)GRID * (BLK / GW))
                for (int lane = 0; lane < GW; ++lane)
                    for (int p = Ap[row] + lane; p < Ap[row + 1]; p += GW) Cx[p] = dst::vertex_entry((int)row, Aj[p], dim, V);
    return 0;
}

}  // extern "C"

#ifdef DSE_MAIN
// An 11 x 9 five-point operator with a row without a diagonal, a stored zero diagonal, a stored zero beside it and an empty row,
// through every routine: every measure, R on both sides of eight and at the cap, odd and even numbers of sweeps.
int main()
{
    const int nx = 11, ny = 9, n = nx * ny;
    std::vector<int> Ap(1, 0), Aj;
    std::vector<double> Ax;
    for (int i = 0; i < n; ++i) {
        const int x = i % nx, y = i / nx;
        if (i != 40) {
            if (y > 0) { Aj.push_back(i - nx); Ax.push_back(-0.21); }
            if (x > 0) { Aj.push_back(i - 1); Ax.push_back(i == 17 ? 0.0 : -0.27); }
            if (i != 5) { Aj.push_back(i); Ax.push_back(i == 23 ? 0.0 : 0.5 + 0.01 * (i % 5)); }
            if (x < nx - 1) { Aj.push_back(i + 1); Ax.push_back(-0.23); }
            if (y < ny - 1) { Aj.push_back(i + nx); Ax.push_back(-0.29); }
        }
        Ap.push_back((int)Aj.size());
    }
    const int nnz = Ap[n];
    double check = 0.0;
    const int Rs[] = {1, 5, 7, 8, 9, 17, 32};
    for (int R : Rs)
        for (int k = 1; k <= 3; ++k)
            for (int m = 0; m < 4; ++m) {
                std::vector<double> X((size_t)n * R), Dx(nnz, -1.0), D2(nnz, -1.0);
                unsigned s = 12345u + (unsigned)(R * 7 + k);
                for (double &v : X) { s = s * 1664525u + 1013904223u; v = (double)(s >> 8) / 16777216.0 - 0.5; }
                std::vector<double> Y(X);
                if (dse_distance_strength(m, Ap.data(), Aj.data(), Ax.data(), X.data(), n, R, k, 0.5, 2.0, Dx.data()) != 0) return 1;
                if (dse_relaxation_vectors(Ap.data(), Aj.data(), Ax.data(), Y.data(), n, R, k, 0.5) != 0) return 1;
                if (X != Y) { std::printf("the chain relaxes differently\n"); return 1; }
                if (dse_distance_measure(m, Ap.data(), Aj.data(), Ax.data(), Y.data(), n, R, D2.data()) != 0) return 1;
                for (int p = 0; p < nnz; ++p) {
                    if (Dx[p] != 0.0 && Dx[p] != D2[p]) { std::printf("the filter changed a value\n"); return 1; }
                    check += Dx[p];
                }
            }
    if (dse_relaxation_vectors(Ap.data(), Aj.data(), Ax.data(), nullptr, n, 33, 1, 0.5) != 2) return 1;
    for (int dim = 1; dim <= 8; ++dim) {
        std::vector<double> V((size_t)n * dim), Cx(nnz, -1.0);
        for (int i = 0; i < n; ++i) for (int d = 0; d < dim; ++d) V[(size_t)i * dim + d] = i == 31 ? 0.25 : 0.1 * ((i * (d + 3)) % 13);
        if (dse_vertex_distance(Ap.data(), Aj.data(), V.data(), n, dim, Cx.data()) != 0) return 1;
        for (double v : Cx) { if (v < 1e-6) return 1; check += v; }
    }
    if (!(check == check)) { std::printf("nan\n"); return 1; }
    std::printf("%.17g\nok\n", check);
    return 0;
}
#endif
