// classical_emul.cpp -- host replay of pyamg_amd/csrc/pamg_classical.hip through the per-row arithmetic of pamg_classical.h: the lanes of
// a launch, the lanes of a group and the rounds of the MIS as loops, in the kernels' phase structure (count / scan / fill; two state
// buffers per round; stage / inner denominators / weights per F-row).  Built by tests/test_classical_host.py with
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC
#include "../pyamg_amd/csrc/pamg_classical.h"

#include <vector>

using namespace pamg;

namespace {

void scan(int n, const int *cnt, int *ptr)
{
    long long run = 0;
    for (int i = 0; i < n; ++i) { ptr[i] = (int)run; run += cnt[i]; }
    ptr[n] = (int)run;
}

template <bool MIN>
void strength(int n, double theta, const int *Ap, const int *Aj, const double *Ax, int *Sp, int *Sj, double *Sx)
{
    std::vector<int> cnt((size_t)n);
    for (int i = 0; i < n; ++i) cnt[(size_t)i] = cls::strength_row<MIN>(i, theta, Ap, Aj, Ax, nullptr, nullptr);
    scan(n, cnt.data(), Sp);
    for (int i = 0; i < n; ++i) cls::strength_row<MIN>(i, theta, Ap, Aj, Ax, Sj + Sp[i], Sx + Sp[i]);
}

// synchronous rounds over two buffers; 0 = ok, 8 = more than n rounds
int mis_rounds(int n, const int *Gp, const int *Gj, const int *Tp, const int *Tj, const double *y, int *x, int active, int C, int F, int *rounds)
{
    std::vector<int> a(x, x + n), b((size_t)n);
    int nr = 0;
    bool done = n == 0;
    while (!done) {
        if (nr == n) return 8;
        bool flag = false;
        for (int i = 0; i < n; ++i) {
            int s = a[(size_t)i];
            if (s == active) {
                s = cls::mis_node(i, Gp, Gj, Tp, Tj, y, a.data(), active, C, F);
                flag = flag || s == active;
            }
            b[(size_t)i] = s;
        }
        a.swap(b);
        ++nr;
        done = !flag;
    }
    for (int i = 0; i < n; ++i) x[i] = a[(size_t)i];
    *rounds = nr;
    return 0;
}

}  // namespace

extern "C" {

void cle_strength(int min_norm, int n, double theta, const int *Ap, const int *Aj, const double *Ax, int *Sp, int *Sj, double *Sx)
{
    if (min_norm) strength<true>(n, theta, Ap, Aj, Ax, Sp, Sj, Sx);
    else strength<false>(n, theta, Ap, Aj, Ax, Sp, Sj, Sx);
}

// 2 = the pattern is not symmetric (what the device refuses)
int cle_mis(int n, const int *Gp, const int *Gj, int active, int C, int F, int *x, const double *y, int *rounds)
{
    for (int i = 0; i < n; ++i)
        for (int p = Gp[i]; p < Gp[i + 1]; ++p) {
            const int j = Gj[p];
            bool found = j == i;
            for (int q = Gp[j]; q < Gp[j + 1] && !found; ++q) found = Gj[q] == i;
            if (!found) return 2;
        }
    return mis_rounds(n, Gp, Gj, nullptr, nullptr, y, x, active, C, F, rounds);
}

int cle_pmis(int n, const int *Sp, const int *Sj, const double *rnd, int *splitting, int *rounds)
{
    std::vector<int> deg((size_t)n, 0), Tp((size_t)n + 1), cur((size_t)n, 0);
    for (int i = 0; i < n; ++i)
        for (int p = Sp[i]; p < Sp[i + 1]; ++p)
            if (Sj[p] != i) ++deg[(size_t)Sj[p]];
    scan(n, deg.data(), Tp.data());
    std::vector<int> Tj((size_t)Tp[(size_t)n] + 1);
    for (int i = n - 1; i >= 0; --i)                        // any order inside a transposed row: the device's is not reproducible either
        for (int p = Sp[i]; p < Sp[i + 1]; ++p)
            if (Sj[p] != i) Tj[(size_t)(Tp[(size_t)Sj[p]] + cur[(size_t)Sj[p]]++)] = i;
    std::vector<double> y((size_t)n);
    for (int i = 0; i < n; ++i) { y[(size_t)i] = (double)deg[(size_t)i] + rnd[i]; splitting[i] = -1; }
    const int rc = mis_rounds(n, Sp, Sj, Tp.data(), Tj.data(), y.data(), splitting, -1, cls::C_NODE, cls::F_NODE, rounds);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) {
        bool any = deg[(size_t)i] > 0;
        for (int p = Sp[i]; p < Sp[i + 1] && !any; ++p) any = Sj[p] != i;
        if (!any) splitting[i] = cls::F_NODE;
    }
    return 0;
}

void cle_interp_pass1(int n, const int *Sp, const int *Sj, const int *splitting, int *Pp)
{
    std::vector<int> cnt((size_t)n);
    for (int i = 0; i < n; ++i) cnt[(size_t)i] = cls::interp_count_row(i, Sp, Sj, splitting);
    scan(n, cnt.data(), Pp);
}

void cle_direct_pass2(int n, const int *Ap, const int *Aj, const double *Ax, const int *Sp, const int *Sj, const double *Sx, const int *splitting,
                      const int *Pp, int *Pj, double *Px)
{
    std::vector<int> map((size_t)n + 1);
    scan(n, splitting, map.data());
    for (int i = 0; i < n; ++i) cls::direct_row(i, Ap, Aj, Ax, Sp, Sj, Sx, splitting, Pp, map.data(), Pj, Px);
}

void cle_remove_ff(int n, const int *Sp, const int *Sj, double *Sx, const int *splitting)
{
    for (int i = 0; i < n; ++i) cls::remove_ff_row(i, Sp, Sj, Sx, splitting);
}

// classes[c] receives the number of F-rows of size class c (8 / 16 / 32 / 64 / longer)
void cle_classical_pass2(int n, const int *Ap, const int *Aj, const double *Ax, const int *Sp, const int *Sj, const double *Sx, const int *splitting,
                         const int *Pp, int *Pj, double *Px, int modified, int *classes)
{
    std::vector<int> map((size_t)n + 1);
    scan(n, splitting, map.data());
    std::vector<double> den((size_t)n, 0.0);
    for (int i = 0; i < n; ++i) {                           // classical_prologue_kernel
        if (splitting[i] == cls::C_NODE) { Pj[Pp[i]] = map[(size_t)i]; Px[Pp[i]] = 1.0; }
        else den[(size_t)i] = cls::classical_denominator(i, Ap, Ax, Sp, Sj, Sx);
    }
    static const int widths[cls::NCLASS] = {8, 16, 32, 64, 64};
    for (int c = 0; c < cls::NCLASS; ++c) {
        classes[c] = 0;
        const int W = widths[c];
        for (int i = 0; i < n; ++i) {                       // classical_rows_kernel<W>: the groups one after another
            const int s0 = Sp[i], ns = Sp[i + 1] - s0;
            if (splitting[i] == cls::C_NODE || ns == 0 || cls::size_class(ns) != c) continue;
            ++classes[c];
            std::vector<int> col((size_t)ns);
            std::vector<double> val((size_t)ns), inner((size_t)ns, 0.0), akk((size_t)ns, 0.0);
            std::vector<unsigned char> kind((size_t)ns);
            for (int lane = 0; lane < W; ++lane)
                for (int t = lane; t < ns; t += W) {
                    col[(size_t)t] = Sj[s0 + t]; val[(size_t)t] = Sx[s0 + t];
                    kind[(size_t)t] = cls::strong_kind(i, Sj[s0 + t], splitting);
                }
            for (int lane = 0; lane < W; ++lane)
                for (int t = lane; t < ns; t += W)
                    if (kind[(size_t)t] == cls::K_F)
                        cls::classical_inner(ns, col.data(), kind.data(), col[(size_t)t], Ap, Aj, Ax, modified != 0, &inner[(size_t)t], &akk[(size_t)t]);
            for (int lane = 0; lane < W; ++lane)
                for (int t = lane; t < ns; t += W)
                    if (kind[(size_t)t] == cls::K_C) {
                        const int w = Pp[i] + cls::c_rank(kind.data(), t);
                        Pj[w] = map[(size_t)col[(size_t)t]];
                        Px[w] = cls::classical_weight(ns, col.data(), val.data(), kind.data(), inner.data(), akk.data(), t, Ap, Aj, Ax, modified != 0,
                                                      den[(size_t)i]);
                    }
        }
    }
}

}  // extern "C"

#ifdef CLE_MAIN
// the replay as a program of its own, for a build with -fsanitize=address,undefined: a 7 x 6 five-point grid with one long row, through every
// entry point
#include <cstdio>
int main()
{
    const int nx = 7, ny = 6, n = nx * ny;
    std::vector<int> Ap{0}, Aj;
    std::vector<double> Ax;
    for (int i = 0; i < n; ++i) {
        const int x = i % nx, y = i / nx;
        if (i == 20) { for (int j = n - 1; j >= 0; --j) { Aj.push_back(j); Ax.push_back(j == i ? 50.0 : -1.0); } }     // a hub row, stored backwards
        else {
            if (y + 1 < ny) { Aj.push_back(i + nx); Ax.push_back(-1.0); }
            if (x + 1 < nx) { Aj.push_back(i + 1); Ax.push_back(i % 5 ? -1.0 : 0.5); }
            Aj.push_back(i); Ax.push_back(4.0);
            if (x > 0) { Aj.push_back(i - 1); Ax.push_back(-1.0); }
            if (y > 0) { Aj.push_back(i - nx); Ax.push_back(-1.0); }
            if (i != 20) { Aj.push_back(20); Ax.push_back(-1.0); }
        }
        Ap.push_back((int)Aj.size());
    }
    // (column 20 appears twice in the rows next to the hub: drop the grid copy so that no row holds a column twice)
    std::vector<int> Bp{0}, Bj;
    std::vector<double> Bx;
    for (int i = 0; i < n; ++i) {
        for (int p = Ap[(size_t)i]; p < Ap[(size_t)i + 1]; ++p) {
            bool dup = false;
            for (int q = Bp[(size_t)i]; q < (int)Bj.size(); ++q) dup = dup || Bj[(size_t)q] == Aj[(size_t)p];
            if (!dup) { Bj.push_back(Aj[(size_t)p]); Bx.push_back(Ax[(size_t)p]); }
        }
        Bp.push_back((int)Bj.size());
    }
    const size_t nnz = Bj.size();
    for (int mn = 0; mn < 2; ++mn) {
        std::vector<int> Sp((size_t)n + 1), Sj(nnz);
        std::vector<double> Sx(nnz);
        cle_strength(mn, n, 0.25, Bp.data(), Bj.data(), Bx.data(), Sp.data(), Sj.data(), Sx.data());
        std::vector<double> rnd((size_t)n);
        for (int i = 0; i < n; ++i) rnd[(size_t)i] = (double)((i * 37) % 11) / 11.0;
        std::vector<int> split((size_t)n);
        int rounds = 0;
        if (cle_pmis(n, Sp.data(), Sj.data(), rnd.data(), split.data(), &rounds) || rounds < 1 || rounds > n) return 1;
        split[20] = 0;                                       // the hub as an F-row
        // the values of A on the pattern of S
        Sj.resize((size_t)Sp[(size_t)n]); Sx.resize((size_t)Sp[(size_t)n]);
        for (int i = 0; i < n; ++i)
            for (int p = Sp[(size_t)i]; p < Sp[(size_t)i + 1]; ++p)
                for (int q = Bp[(size_t)i]; q < Bp[(size_t)i + 1]; ++q)
                    if (Bj[(size_t)q] == Sj[(size_t)p]) Sx[(size_t)p] = Bx[(size_t)q];
        std::vector<int> Pp((size_t)n + 1);
        cle_interp_pass1(n, Sp.data(), Sj.data(), split.data(), Pp.data());
        std::vector<int> Pj((size_t)Pp[(size_t)n]);
        std::vector<double> Px((size_t)Pp[(size_t)n]);
        int classes[5];
        cle_direct_pass2(n, Bp.data(), Bj.data(), Bx.data(), Sp.data(), Sj.data(), Sx.data(), split.data(), Pp.data(), Pj.data(), Px.data());
        for (int modified = 0; modified < 2; ++modified)
            cle_classical_pass2(n, Bp.data(), Bj.data(), Bx.data(), Sp.data(), Sj.data(), Sx.data(), split.data(), Pp.data(), Pj.data(), Px.data(),
                                modified, classes);
        std::vector<double> Fx(Sx);
        cle_remove_ff(n, Sp.data(), Sj.data(), Fx.data(), split.data());
        // MIS on the symmetrised pattern
        std::vector<std::vector<int>> adj((size_t)n);
        for (int i = 0; i < n; ++i)
            for (int p = Sp[(size_t)i]; p < Sp[(size_t)i + 1]; ++p) { adj[(size_t)i].push_back(Sj[(size_t)p]); adj[(size_t)Sj[(size_t)p]].push_back(i); }
        std::vector<int> Gp{0}, Gj;
        for (int i = 0; i < n; ++i) { for (int j : adj[(size_t)i]) Gj.push_back(j); Gp.push_back((int)Gj.size()); }
        std::vector<int> x((size_t)n, -1);
        std::vector<double> y((size_t)n, 1.0);
        if (cle_mis(n, Gp.data(), Gj.data(), -1, 1, 0, x.data(), y.data(), &rounds)) return 2;
        for (int i = 0; i < n; ++i) if (x[(size_t)i] != 0 && x[(size_t)i] != 1) return 3;
    }
    std::printf("ok\n");
    return 0;
}
#endif
