// lloyd_emul.cpp -- host replay of pyamg_amd/csrc/pamg_lloyd.hip through the rules of pamg_lloyd.h: the lanes of a launch and the rounds as
// loops, in the kernels' phase structure (synchronous distance rounds over two buffers, in-place stamp rounds, pointer jumping, labels;
// boundary, the same three steps, the centre update).  The edges are visited from the LAST to the first, the opposite of the reference's
// sweep: the result may not depend on it.  The entries have the signatures of the C ABI (include/pyamg_amd.h) and its checks.  Built by
// tests/test_lloyd_host.py with
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC
#include "../pyamg_amd/csrc/pamg_lloyd.h"

#include <algorithm>
#include <cstdio>
#include <vector>

using namespace pamg;
using lloyd::stamp_t;

namespace {

constexpr int E_NOCONV = -8;

struct Work {
    int n = 0, nc = 0;
    long long nnz = 0;
    std::vector<int> row, q, first;
    const int *Aj = nullptr;
    const double *Ax = nullptr;
    std::vector<double> d[2];
    std::vector<stamp_t> key, dmax;
    int *c = nullptr, *m = nullptr, *p = nullptr;
    int cur = 0, dist_rounds = 0, stamp_rounds = 0;

    void setup(int n_, const int *Ap, const int *Aj_, const double *Ax_, int *c_, int nc_, int *m_, int *p_)
    {
        n = n_; nc = nc_; nnz = Ap[n]; Aj = Aj_; Ax = Ax_; c = c_; m = m_; p = p_;
        row.assign((size_t)nnz + 1, 0);
        for (long long e = 0; e < nnz; ++e) row[(size_t)e] = lloyd::row_of_entry(n, Ap, e);
        d[0].assign((size_t)n, 0.0); d[1].assign((size_t)n, 0.0);
        key.assign((size_t)n, 0); q.assign((size_t)n, 0); dmax.assign((size_t)nc + 1, 0); first.assign((size_t)nc + 1, 0);
    }

    int bellman_ford()
    {
        int nr = 0;
        for (bool changed = true; changed; ++nr) {          // distances: synchronous rounds
            if (nr == n) return E_NOCONV;
            changed = false;
            const std::vector<double> &prev = d[cur];
            std::vector<double> &next = d[cur ^ 1];
            next = prev;
            for (long long e = nnz - 1; e >= 0; --e) {
                const int j = Aj[e];
                double cand;
                if (lloyd::relaxes(prev[(size_t)row[(size_t)e]], Ax[e], prev[(size_t)j], &cand)) {
                    if (lloyd::bits_of(cand) < lloyd::bits_of(next[(size_t)j])) next[(size_t)j] = cand;    // the atomic min on the bits
                    changed = true;
                }
            }
            cur ^= 1;
        }
        dist_rounds += nr;
        const std::vector<double> &dd = d[cur];
        for (int i = 0; i < n; ++i) key[(size_t)i] = dd[(size_t)i] == 0.0 ? lloyd::SOURCE_STAMP : lloyd::NO_STAMP;
        nr = 0;
        for (bool changed = true; changed; ++nr) {          // stamps: in-place rounds
            if (nr == n) return E_NOCONV;
            changed = false;
            for (long long e = nnz - 1; e >= 0; --e) {
                const int i = row[(size_t)e], j = Aj[e];
                if (!lloyd::tight(dd[(size_t)i], Ax[e], dd[(size_t)j])) continue;
                const stamp_t ki = key[(size_t)i];
                if (ki == lloyd::NO_STAMP) continue;
                const stamp_t cand = lloyd::stamp_of(ki, i);
                if (key[(size_t)j] > cand) { key[(size_t)j] = cand; changed = true; }
            }
        }
        stamp_rounds += nr;
        for (int j = 0; j < n; ++j) q[(size_t)j] = lloyd::was_written(key[(size_t)j]) ? lloyd::writer_of(key[(size_t)j]) : j;
        for (bool changed = true; changed;) {               // labels: pointer jumping
            changed = false;
            for (int j = n - 1; j >= 0; --j) {
                const int a = q[(size_t)j], b = q[(size_t)a];
                if (b != a) { q[(size_t)j] = b; changed = true; }
            }
        }
        for (int j = 0; j < n; ++j)
            if (lloyd::was_written(key[(size_t)j])) { p[j] = lloyd::writer_of(key[(size_t)j]); m[j] = m[q[(size_t)j]]; }
        return 0;
    }

    int most_interior(int *nmoved)
    {
        std::vector<double> &dd = d[cur];
        std::fill(dd.begin(), dd.end(), lloyd::infinity());
        for (long long e = nnz - 1; e >= 0; --e) {
            const int i = row[(size_t)e];
            if (lloyd::is_boundary_edge(m[i], m[Aj[e]])) dd[(size_t)i] = 0.0;
        }
        if (int st = bellman_ford()) return st;
        const std::vector<double> &df = d[cur];
        *nmoved = 0;
        for (int a = 0; a < nc; ++a) { dmax[(size_t)a] = 0ull; first[(size_t)a] = lloyd::NO_NODE; }
        for (int i = n - 1; i >= 0; --i)
            if (m[i] >= 0) dmax[(size_t)m[i]] = std::max(dmax[(size_t)m[i]], lloyd::bits_of(df[(size_t)i]));
        for (int i = n - 1; i >= 0; --i)
            if (m[i] >= 0 && lloyd::bits_of(df[(size_t)i]) == dmax[(size_t)m[i]]) first[(size_t)m[i]] = std::min(first[(size_t)m[i]], i);
        for (int a = 0; a < nc; ++a)
            if (lloyd::centre_moves(df[(size_t)c[a]], lloyd::dist_of(dmax[(size_t)a]), first[(size_t)a])) { c[a] = first[(size_t)a]; ++*nmoved; }
        return 0;
    }
};

// check_pattern of pamg_host_call.h, with values
int check_graph(int n, const int *Ap, int Ap_size, const int *Aj, int Aj_size, const double *Ax, int Ax_size, const int *c, int c_size)
{
    if (n < 0 || !Ap || Ap_size < n + 1 || Ap[0] != 0) return lloyd::BAD_ARG;
    for (int i = 0; i < n; ++i) if (Ap[i + 1] < Ap[i]) return lloyd::BAD_ARG;
    const long long nnz = Ap[n];
    if (nnz > Aj_size || (nnz && !Aj) || nnz > Ax_size || (nnz && !Ax)) return lloyd::BAD_ARG;
    for (long long e = 0; e < nnz; ++e) if (Aj[e] < 0 || Aj[e] >= n) return lloyd::BAD_ARG;
    if (c_size < 0 || (c_size && !c)) return lloyd::BAD_ARG;
    if (int st = lloyd::check_centres(n, c, c_size)) return st;
    return lloyd::check_weights(n, nnz, Ax);
}

}  // namespace

extern "C" {

int lle_bellman_ford(int n, const int *Ap, int Ap_size, const int *Aj, int Aj_size, const double *Ax, int Ax_size, const int *c, int c_size,
                     double *d, int d_size, int *m, int m_size, int *p, int p_size, int *info)
{
    if (n < 0 || d_size < n || m_size < n || p_size < n || (n && (!d || !m || !p))) return lloyd::BAD_ARG;
    if (int st = check_graph(n, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, c, c_size)) return st;
    if (int st = lloyd::check_start(n, d)) return st;
    if (info) info[0] = info[1] = 0;
    if (n == 0) return 0;
    std::vector<int> hc(c, c + c_size), hm(m, m + n), hp(p, p + n);
    Work w;
    w.setup(n, Ap, Aj, Ax, hc.data(), c_size, hm.data(), hp.data());
    std::copy(d, d + n, w.d[0].begin());
    if (int st = w.bellman_ford()) return st;
    std::copy(w.d[w.cur].begin(), w.d[w.cur].end(), d); std::copy(hm.begin(), hm.end(), m); std::copy(hp.begin(), hp.end(), p);
    if (info) { info[0] = w.dist_rounds; info[1] = w.stamp_rounds; }
    return 0;
}

int lle_most_interior_nodes(int n, const int *Ap, int Ap_size, const int *Aj, int Aj_size, const double *Ax, int Ax_size, int *c, int c_size,
                            double *d, int d_size, int *m, int m_size, int *p, int p_size, int *info)
{
    if (n < 0 || d_size < n || m_size < n || p_size < n || (n && (!d || !m || !p))) return lloyd::BAD_ARG;
    if (int st = check_graph(n, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, c, c_size)) return st;
    if (int st = lloyd::check_labels(n, m, c_size)) return st;
    if (info) info[0] = info[1] = info[2] = 0;
    if (n == 0) return 0;
    std::vector<int> hc(c, c + c_size), hm(m, m + n), hp(p, p + n);
    Work w;
    w.setup(n, Ap, Aj, Ax, hc.data(), c_size, hm.data(), hp.data());
    int nmoved = 0;
    if (int st = w.most_interior(&nmoved)) return st;
    std::copy(w.d[w.cur].begin(), w.d[w.cur].end(), d); std::copy(hm.begin(), hm.end(), m); std::copy(hp.begin(), hp.end(), p);
    std::copy(hc.begin(), hc.end(), c);
    if (info) { info[0] = w.dist_rounds; info[1] = w.stamp_rounds; info[2] = nmoved; }
    return 0;
}

int lle_lloyd_cluster(int n, const int *Ap, int Ap_size, const int *Aj, int Aj_size, const double *Ax, int Ax_size, int *c, int c_size,
                      int maxiter, int *clusters, int clusters_size, int *info)
{
    if (n < 0 || clusters_size < n || (n && !clusters)) return lloyd::BAD_ARG;
    if (int st = check_graph(n, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, c, c_size)) return st;
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (n == 0) return 0;
    std::vector<int> hc(c, c + c_size), hm((size_t)n, -1), hp((size_t)n, -1);
    int it = 0, nmoved = 0;
    Work w;
    w.setup(n, Ap, Aj, Ax, hc.data(), c_size, hm.data(), hp.data());
    if (maxiter <= 0)
        for (int a = 0; a < c_size; ++a) hm[(size_t)c[a]] = a;
    for (bool changed = true; changed && it < maxiter; ++it) {
        std::fill(w.d[w.cur].begin(), w.d[w.cur].end(), lloyd::infinity());
        std::fill(hm.begin(), hm.end(), -1); std::fill(hp.begin(), hp.end(), -1);
        for (int a = 0; a < c_size; ++a) {                  // two clusters can share a centre after an update: the largest index stays
            w.d[w.cur][(size_t)hc[(size_t)a]] = 0.0;
            hm[(size_t)hc[(size_t)a]] = std::max(hm[(size_t)hc[(size_t)a]], a);
        }
        if (int st = w.bellman_ford()) return st;
        if (int st = w.most_interior(&nmoved)) return st;
        changed = nmoved > 0;
    }
    std::copy(hm.begin(), hm.end(), clusters); std::copy(hc.begin(), hc.end(), c);
    if (info) { info[0] = it; info[1] = w.dist_rounds; info[2] = w.stamp_rounds; info[3] = nmoved; }
    return 0;
}

}  // extern "C"

#ifdef LLE_MAIN
// the replay as a program of its own, for a sanitizer build: a 7 x 5 grid with unit weights, a graph with a row of 70 entries and
// unreached nodes, and the refusals
int main()
{
    const int nx = 7, ny = 5, n = nx * ny;
    std::vector<int> Ap(1, 0), Aj;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            if (y) Aj.push_back((y - 1) * nx + x);
            if (x) Aj.push_back(y * nx + x - 1);
            Aj.push_back(y * nx + x);
            if (x + 1 < nx) Aj.push_back(y * nx + x + 1);
            if (y + 1 < ny) Aj.push_back((y + 1) * nx + x);
            Ap.push_back((int)Aj.size());
        }
    std::vector<double> Ax(Aj.size(), 1.0);
    std::vector<int> c = {3, 17, 30}, cl((size_t)n);
    int info[4];
    if (lle_lloyd_cluster(n, Ap.data(), n + 1, Aj.data(), (int)Aj.size(), Ax.data(), (int)Ax.size(), c.data(), 3, 5, cl.data(), n, info)) return 1;
    for (int i = 0; i < n; ++i) if (cl[(size_t)i] < 0 || cl[(size_t)i] > 2) return 2;
    if (info[0] < 1 || info[1] < 2 * info[0] || info[2] < 2 * info[0]) return 3;
    // a hub of 70 entries, three unreached nodes
    const int nh = 80;
    std::vector<int> Hp(1, 0), Hj;
    for (int i = 0; i < nh; ++i) {
        if (i == 0) for (int j = 1; j <= 70; ++j) Hj.push_back(j);
        else if (i <= 70) Hj.push_back(i % 70 + 1);
        Hp.push_back((int)Hj.size());
    }
    std::vector<double> Hx(Hj.size(), 2.0), d((size_t)nh, lloyd::infinity());
    std::vector<int> hc = {0}, m((size_t)nh, -1), p((size_t)nh, -1);
    d[0] = 0.0; m[0] = 0;
    if (lle_bellman_ford(nh, Hp.data(), nh + 1, Hj.data(), (int)Hj.size(), Hx.data(), (int)Hx.size(), hc.data(), 1, d.data(), nh, m.data(), nh,
                         p.data(), nh, info)) return 4;
    for (int i = 1; i <= 70; ++i) if (d[(size_t)i] != 2.0 || m[(size_t)i] != 0 || p[(size_t)i] != 0) return 5;
    for (int i = 71; i < nh; ++i) if (d[(size_t)i] != lloyd::infinity() || m[(size_t)i] != -1 || p[(size_t)i] != -1) return 6;
    int moved[3];
    if (lle_most_interior_nodes(nh, Hp.data(), nh + 1, Hj.data(), (int)Hj.size(), Hx.data(), (int)Hx.size(), hc.data(), 1, d.data(), nh, m.data(),
                                nh, p.data(), nh, moved)) return 7;
    // refusals: a real weight, an explicit zero, a repeated centre, a centre out of range
    Hx[3] = 0.5;
    if (lle_bellman_ford(nh, Hp.data(), nh + 1, Hj.data(), (int)Hj.size(), Hx.data(), (int)Hx.size(), hc.data(), 1, d.data(), nh, m.data(), nh,
                         p.data(), nh, info) != lloyd::UNSUPPORTED) return 8;
    Hx[3] = 0.0;
    if (lle_lloyd_cluster(nh, Hp.data(), nh + 1, Hj.data(), (int)Hj.size(), Hx.data(), (int)Hx.size(), hc.data(), 1, 5, m.data(), nh, info) !=
        lloyd::UNSUPPORTED) return 9;
    Hx[3] = 2.0;
    std::vector<int> twice = {4, 4}, far = {nh};
    if (lle_lloyd_cluster(nh, Hp.data(), nh + 1, Hj.data(), (int)Hj.size(), Hx.data(), (int)Hx.size(), twice.data(), 2, 5, m.data(), nh, info) !=
        lloyd::UNSUPPORTED) return 10;
    if (lle_lloyd_cluster(nh, Hp.data(), nh + 1, Hj.data(), (int)Hj.size(), Hx.data(), (int)Hx.size(), far.data(), 1, 5, m.data(), nh, info) !=
        lloyd::BAD_ARG) return 11;
    std::printf("ok\n");
    return 0;
}
#endif
