// Host replay of pyamg_amd/csrc/pamg_schwarz_setup.hip: the same per-lane arithmetic (pamg_dense_pinv.h), the lanes of a
// group -- and the groups of a wave -- as loops.  A wave holds 64 / W groups of W lanes; the groups of a wave share the
// bounds of the pair loop and the sweep loop exactly like the kernel, so the replay also checks that a group is not
// disturbed by a neighbour that is larger, slower or absent.  Cross-lane sums walk the kernel's butterfly offsets.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC schwarz_setup_emul.cpp -o schwarz_setup_emul.so
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -DSSE_MAIN schwarz_setup_emul.cpp -o sse   (stand-alone)
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../pyamg_amd/csrc/pamg_dense_pinv.h"

using namespace pamg;

namespace {

// the plan kernel: block pointer (64-bit), largest m, the subdomains of every size class in their own order
struct Plan {
    std::vector<long long> tp;
    std::vector<int> list[dpinv::NCLASS];
    int maxm = 0;
    bool bad = false;
};

Plan make_plan(int nsub, const int *Sp)
{
    Plan p;
    p.tp.assign((size_t)nsub + 1, 0);
    long long run = 0;
    for (int d = 0; d < nsub; ++d) {
        const int m = Sp[d + 1] - Sp[d];
        p.tp[d] = run;
        if (m < 0 || Sp[d] < 0) { p.bad = true; continue; }
        run += (long long)m * m;
        p.maxm = std::max(p.maxm, m);
        if (m > 0 && m <= dpinv::MAX_M) p.list[dpinv::size_class(m)].push_back(d);
    }
    p.tp[nsub] = run;
    return p;
}

template <typename T, int W>
int extract_class(const std::vector<int> &list, const int *Sp, const int *Sj, const long long *Tp, int nrows, const int *Ap, const int *Aj,
                  const T *Ax, T *Tx)
{
    int bad = 0;
    for (int d : list) {
        int S[W];
        const int m = Sp[d + 1] - Sp[d];
        for (int l = 0; l < m; ++l) S[l] = Sj[Sp[d] + l];
        T *blk = Tx + Tp[d];
        for (int r = 0; r < m; ++r) {
            const int row = S[r];
            if (row < 0 || row >= nrows) { bad = 1; continue; }
            const int a0 = Ap[row], a1 = Ap[row + 1];
            for (int l = 0; l < W; ++l)                       // the lanes of the group
                for (int k = a0 + l; k < a1; k += W) {
                    const int c = dpinv::extract_target(Aj, a0, k, S, m);
                    if (c >= 0) blk[r * m + c] = Ax[k];
                }
        }
    }
    return bad;
}

template <typename T, int W>
void group_sum(T *v)        // v[W]: every lane ends with the sum
{
    dpinv::butterfly_offsets<W>([&](int off) {
        T t[W];
        for (int l = 0; l < W; ++l) t[l] = v[l] + v[l ^ off];
        for (int l = 0; l < W; ++l) v[l] = t[l];
    });
}

struct Info { long long sweeps = 0, trunc = 0, noconv = 0; };

// one wave: groups g = 0 .. NG-1 own the blocks list[first + g]
template <typename T, int W>
void pinv_wave(const int *list, int count, long long first, const int *Sp, const long long *Tp, T *Tx, T rank_tol, int sweep_cap, Info &info,
               int *rank_out)
{
    constexpr int NG = 64 / W;
    static thread_local std::vector<T> sU, sV;
    sU.assign((size_t)NG * W * W, T(0));
    sV.assign((size_t)NG * W * W, T(0));
    int d[NG], m[NG];
    T *U[NG], *V[NG], *blk[NG], fro2[NG], tol[NG], floor2[NG];
    bool live[NG];
    int mw = 0;
    for (int g = 0; g < NG; ++g) {
        d[g] = first + g < count ? list[first + g] : -1;
        m[g] = d[g] >= 0 ? Sp[d[g] + 1] - Sp[d[g]] : 0;
        U[g] = sU.data() + (size_t)g * W * W;
        V[g] = sV.data() + (size_t)g * W * W;
        blk[g] = d[g] >= 0 ? Tx + Tp[d[g]] : nullptr;
        for (int i = 0; i < W; ++i) V[g][i * W + i] = T(1);
        for (int e = 0; e < m[g] * m[g]; ++e) U[g][(e % m[g]) * W + e / m[g]] = blk[g][e];
        T part[W];
        for (int i = 0; i < W; ++i) {
            part[i] = T(0);
            if (i < m[g]) for (int j = 0; j < m[g]; ++j) part[i] += U[g][j * W + i] * U[g][j * W + i];
        }
        group_sum<T, W>(part);
        fro2[g] = part[0];
        tol[g] = dpinv::pair_tolerance<T>(m[g] > 0 ? m[g] : 1);
        floor2[g] = dpinv::noise_floor2<T>(m[g], fro2[g]);
        live[g] = m[g] > 1;
        mw = std::max(mw, m[g]);
    }
    int sweeps = 0;
    auto any_live = [&] { for (int g = 0; g < NG; ++g) if (live[g]) return true; return false; };
    while (any_live() && sweeps < sweep_cap) {
        int rotated[NG] = {};
        for (int j = 0; j + 1 < mw; ++j)
            for (int k = j + 1; k < mw; ++k)
                for (int g = 0; g < NG; ++g) {
                    const bool mine = live[g] && k < m[g];
                    T aa[W], bb[W], dd[W];
                    for (int i = 0; i < W; ++i) {
                        T uj = T(0), uk = T(0);
                        if (mine && i < m[g]) { uj = U[g][j * W + i]; uk = U[g][k * W + i]; }
                        aa[i] = uj * uj; bb[i] = uk * uk; dd[i] = uj * uk;
                    }
                    group_sum<T, W>(aa); group_sum<T, W>(bb); group_sum<T, W>(dd);
                    if (!mine) continue;
                    const dpinv::Rotation<T> r = dpinv::rotation(aa[0], bb[0], dd[0], tol[g], floor2[g]);
                    if (!r.on) continue;
                    ++rotated[g];
                    for (int i = 0; i < m[g]; ++i) {
                        dpinv::rotate(U[g][j * W + i], U[g][k * W + i], r.c, r.s);
                        dpinv::rotate(V[g][j * W + i], V[g][k * W + i], r.c, r.s);
                    }
                }
        ++sweeps;
        for (int g = 0; g < NG; ++g) {
            if (live[g] && rotated[g] == 0) live[g] = false;
            if (live[g] && sweeps >= sweep_cap) ++info.noconv;
        }
    }
    for (int g = 0; g < NG; ++g) {
        if (d[g] < 0) continue;
        const int mg = m[g];
        T sig[W] = {}, smax = T(0);
        for (int j = 0; j < mg; ++j) {
            T part[W];
            for (int i = 0; i < W; ++i) { const T u = i < mg ? U[g][j * W + i] : T(0); part[i] = u * u; }
            group_sum<T, W>(part);
            sig[j] = std::sqrt(part[0]);
            smax = std::fmax(smax, sig[j]);
        }
        int nkept = 0;
        for (int j = 0; j < mg; ++j) {
            const bool keep = dpinv::kept(sig[j], smax, rank_tol);
            const T w = keep ? T(1) / sig[j] : T(0);
            nkept += keep ? 1 : 0;
            for (int i = 0; i < mg; ++i) {
                U[g][j * W + i] = U[g][j * W + i] * w;
                V[g][j * W + i] = V[g][j * W + i] * w;
            }
        }
        for (int i = 0; i < mg; ++i)
            for (int c = 0; c < mg; ++c) {
                T acc = T(0);
                for (int j = 0; j < mg; ++j) acc += V[g][j * W + i] * U[g][j * W + c];
                blk[g][i * mg + c] = acc;
            }
        if (nkept < mg) ++info.trunc;
        if (rank_out) rank_out[d[g]] = nkept;
        info.sweeps = std::max<long long>(info.sweeps, mg > 1 ? sweeps : 0);
    }
}

template <typename T, int W>
void pinv_class(const std::vector<int> &list, const int *Sp, const long long *Tp, T *Tx, T rank_tol, int sweep_cap, Info &info, int *rank_out)
{
    constexpr int NG = 64 / W;
    for (long long first = 0; first < (long long)list.size(); first += NG)
        pinv_wave<T, W>(list.data(), (int)list.size(), first, Sp, Tp, Tx, rank_tol, sweep_cap, info, rank_out);
}

// 0 ok, 1 bad argument, 2 unsupported (a subdomain above 64 rows / more than 2^31 - 1 entries), 3 not converged
template <typename T>
int blocks(int nrows, const int *Ap, const int *Aj, const T *Ax, int nsub, const int *Sp, const int *Sj, int *Tp, T *Tx, long long Tx_capacity,
           double rank_tol, int invert, int sweep_cap, long long *info4, int *rank_out)
{
    const Plan p = make_plan(nsub, Sp);
    info4[0] = p.tp[nsub]; info4[1] = p.maxm; info4[2] = info4[3] = 0;
    if (p.bad) return 1;
    if (p.maxm > dpinv::MAX_M || p.tp[nsub] > 2147483647LL) return 2;
    if (p.tp[nsub] > Tx_capacity) return 1;
    for (int d = 0; d <= nsub; ++d) Tp[d] = (int)p.tp[d];
    std::fill(Tx, Tx + p.tp[nsub], T(0));
    int bad = 0;
    bad |= extract_class<T, 8>(p.list[0], Sp, Sj, p.tp.data(), nrows, Ap, Aj, Ax, Tx);
    bad |= extract_class<T, 16>(p.list[1], Sp, Sj, p.tp.data(), nrows, Ap, Aj, Ax, Tx);
    bad |= extract_class<T, 32>(p.list[2], Sp, Sj, p.tp.data(), nrows, Ap, Aj, Ax, Tx);
    bad |= extract_class<T, 64>(p.list[3], Sp, Sj, p.tp.data(), nrows, Ap, Aj, Ax, Tx);
    if (bad) return 1;
    if (!invert) return 0;
    Info info;
    pinv_class<T, 8>(p.list[0], Sp, p.tp.data(), Tx, (T)rank_tol, sweep_cap, info, rank_out);
    pinv_class<T, 16>(p.list[1], Sp, p.tp.data(), Tx, (T)rank_tol, sweep_cap, info, rank_out);
    pinv_class<T, 32>(p.list[2], Sp, p.tp.data(), Tx, (T)rank_tol, sweep_cap, info, rank_out);
    pinv_class<T, 64>(p.list[3], Sp, p.tp.data(), Tx, (T)rank_tol, sweep_cap, info, rank_out);
    info4[2] = info.sweeps; info4[3] = info.trunc;
    return info.noconv ? 3 : 0;
}

}  // namespace

extern "C" {

int sse_blocks_f64(int nrows, const int *Ap, const int *Aj, const double *Ax, int nsub, const int *Sp, const int *Sj, int *Tp, double *Tx,
                   long long Tx_capacity, double rank_tol, int invert, int sweep_cap, long long *info4, int *rank_out)
{
    return blocks<double>(nrows, Ap, Aj, Ax, nsub, Sp, Sj, Tp, Tx, Tx_capacity, rank_tol, invert, sweep_cap, info4, rank_out);
}

int sse_blocks_f32(int nrows, const int *Ap, const int *Aj, const float *Ax, int nsub, const int *Sp, const int *Sj, int *Tp, float *Tx,
                   long long Tx_capacity, double rank_tol, int invert, int sweep_cap, long long *info4, int *rank_out)
{
    return blocks<float>(nrows, Ap, Aj, Ax, nsub, Sp, Sj, Tp, Tx, Tx_capacity, rank_tol, invert, sweep_cap, info4, rank_out);
}

int sse_sweep_cap(void) { return dpinv::SWEEP_CAP; }
int sse_max_m(void) { return dpinv::MAX_M; }

}  // extern "C"

#ifdef SSE_MAIN
// stand-alone run for the sanitizers: disconnected Neumann chains of every size-class edge (singular blocks), the same
// plus 0.1 I, a 65-row subdomain (refused), a sweep cap of 1 (reported)
template <typename T>
int chains(double shift, double rank_tol)
{
    const int len[] = {1, 2, 8, 9, 16, 17, 32, 33, 64};
    std::vector<int> Ap{0}, Aj, Sp{0}, Sj;
    std::vector<T> Ax;
    int n = 0;
    for (int L : len) {
        for (int i = 0; i < L; ++i) {
            const int deg = (i > 0) + (i + 1 < L);
            if (i > 0) { Aj.push_back(n + i - 1); Ax.push_back(T(-1)); }
            Aj.push_back(n + i); Ax.push_back((T)(deg + shift));
            if (i + 1 < L) { Aj.push_back(n + i + 1); Ax.push_back(T(-1)); }
            Ap.push_back((int)Aj.size());
            Sj.push_back(n + i);
        }
        n += L;
        Sp.push_back((int)Sj.size());
    }
    const int nsub = (int)Sp.size() - 1;
    long long total = 0;
    for (int L : len) total += (long long)L * L;
    std::vector<int> Tp((size_t)nsub + 1), rank((size_t)nsub, -1);
    std::vector<T> Tx((size_t)total);
    long long info[4];
    int rc = blocks<T>(n, Ap.data(), Aj.data(), Ax.data(), nsub, Sp.data(), Sj.data(), Tp.data(), Tx.data(), total, rank_tol, 1, dpinv::SWEEP_CAP, info, rank.data());
    std::printf("shift %.1f: rc %d total %lld maxm %lld sweeps %lld truncated %lld\n", shift, rc, info[0], info[1], info[2], info[3]);
    if (rc != 0 || info[0] != total || info[1] != 64) return 1;
    for (int d = 0; d < nsub; ++d) if (rank[d] != (shift == 0.0 ? len[d] - 1 : len[d])) return 1;
    if (info[3] != (shift == 0.0 ? nsub : 0)) return 1;
    rc = blocks<T>(n, Ap.data(), Aj.data(), Ax.data(), nsub, Sp.data(), Sj.data(), Tp.data(), Tx.data(), total, rank_tol, 1, 1, info, rank.data());
    if (rc != 3) return 1;
    return 0;
}

int main()
{
    if (chains<double>(0.0, 1e6 * 2.220446049250313e-16) || chains<double>(0.1, 1e6 * 2.220446049250313e-16)) return 1;
    if (chains<float>(0.0, 1e3 * 1.1920929e-07) || chains<float>(0.1, 1e3 * 1.1920929e-07)) return 1;
    const int Ap[2] = {0, 0}, Sp[2] = {0, 65};
    std::vector<int> Sj(65, 0), Tp(2);
    long long info[4];
    double tx = 7.0;
    if (blocks<double>(1, Ap, nullptr, (const double *)nullptr, 1, Sp, Sj.data(), Tp.data(), &tx, 1, 0.0, 1, 60, info, nullptr) != 2 || tx != 7.0) return 1;
    std::puts("ok");
    return 0;
}
#endif
