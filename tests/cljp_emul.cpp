// cljp_emul.cpp -- host replay of pyamg_amd/csrc/pamg_cljp.hip through the rules of pamg_cljp.h: the lanes of a launch, the lanes of a
// group, the rounds of a colour and the passes of the selection as loops, in the kernels' phase structure (two state buffers per round
// and per selection; P5 / apply / P6 by size class / apply; integer decrement counters).  Built by tests/test_cljp_host.py with
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC
#include "../pyamg_amd/csrc/pamg_cljp.h"

#include <vector>

using namespace pamg;

namespace {

void scan(int n, const int *cnt, int *ptr)
{
    long long run = 0;
    for (int i = 0; i < n; ++i) { ptr[i] = (int)run; run += cnt[i]; }
    ptr[n] = (int)run;
}

// the off-diagonal transposed pattern, rows filled from the last row up: any order inside a transposed row, the device's is not
// reproducible either
void transpose(int n, const int *Sp, const int *Sj, std::vector<int> &deg, std::vector<int> &Tp, std::vector<int> &Tj)
{
    deg.assign((size_t)n, 0); Tp.assign((size_t)n + 1, 0);
    std::vector<int> cur((size_t)n, 0);
    for (int i = 0; i < n; ++i)
        for (int p = Sp[i]; p < Sp[i + 1]; ++p)
            if (Sj[p] != i) ++deg[(size_t)Sj[p]];
    scan(n, deg.data(), Tp.data());
    Tj.assign((size_t)Tp[(size_t)n] + 1, 0);
    for (int i = n - 1; i >= 0; --i)
        for (int p = Sp[i]; p < Sp[i + 1]; ++p)
            if (Sj[p] != i) Tj[(size_t)(Tp[(size_t)Sj[p]] + cur[(size_t)Sj[p]]++)] = i;
}

// colouring(): 0 = ok, 8 = more than n rounds for a colour or more than n colours
int colouring(int n, const int *Tp, const int *Tj, std::vector<int> &x, int *ncolors, int *rounds, int *deepest)
{
    std::vector<int> a((size_t)n, cljp::UNDECIDED), b((size_t)n);
    int K = 0, total = 0;
    *deepest = 0;
    for (;;) {
        if (K == n) return 8;
        int nr = 0;
        bool done = false;
        while (!done) {
            if (nr == n) return 8;
            bool flag = false;
            for (int i = 0; i < n; ++i) {                   // colour_round_kernel
                int s = a[(size_t)i];
                if (s == cljp::UNDECIDED) {
                    s = cljp::colour_node(i, Tp, Tj, a.data(), K);
                    flag = flag || s == cljp::UNDECIDED;
                }
                b[(size_t)i] = s;
            }
            a.swap(b);
            ++nr;
            done = !flag;
        }
        total += nr;
        if (nr > *deepest) *deepest = nr;
        ++K;
        bool more = false;
        for (int i = 0; i < n; ++i)                         // colour_next_kernel
            if (a[(size_t)i] == cljp::OUT) { a[(size_t)i] = cljp::UNDECIDED; more = true; }
        if (!more) break;
    }
    x = a;
    *ncolors = K;
    *rounds = total;
    return 0;
}

}  // namespace

extern "C" {

// info: colours, rounds, the most rounds one colour took
int cje_vertex_coloring_mis(int n, const int *Ap, const int *Aj, int *x, int *info)
{
    info[0] = info[1] = info[2] = 0;
    if (n == 0) return 0;
    std::vector<int> deg, Tp, Tj, col;
    transpose(n, Ap, Aj, deg, Tp, Tj);
    const int rc = colouring(n, Tp.data(), Tj.data(), col, &info[0], &info[1], &info[2]);
    if (rc) return rc;
    for (int i = 0; i < n; ++i) x[i] = col[(size_t)i];
    return 0;
}

// info: passes, colours, colouring rounds, nodes selected, then what the replay alone can tell: [4] the most rounds one colour took,
// [5] rows of the looping class that staged an entry, [6] passes in which two adjacent nodes were selected together, [7] edges removed by
// P6, [8 .. 12] rows per size class
int cje_cljp(int n, const int *Sp, const int *Sj, int colorflag, int *splitting, int *info)
{
    for (int k = 0; k < 13; ++k) info[k] = 0;
    if (n == 0) return 0;
    const int nnz = Sp[n];
    std::vector<int> deg, Tp, Tj;
    transpose(n, Sp, Sj, deg, Tp, Tj);
    std::vector<double> w((size_t)n);
    if (colorflag == 1) {
        std::vector<int> col;
        const int rc = colouring(n, Tp.data(), Tj.data(), col, &info[1], &info[2], &info[4]);
        if (rc) return rc;
        for (int i = 0; i < n; ++i) w[(size_t)i] = cljp::initial_weight(cljp::colour_weight(col[(size_t)i], info[1]), deg[(size_t)i]);
    } else {
        std::vector<double> rnd((size_t)n);
        cljp::random_weights(n, rnd.data());
        for (int i = 0; i < n; ++i) w[(size_t)i] = cljp::initial_weight(rnd[(size_t)i], deg[(size_t)i]);
    }
    std::vector<int> a((size_t)n, cljp::U_NODE), b((size_t)n), cnt((size_t)n, 0), selpass((size_t)n, 0);
    std::vector<unsigned char> mark((size_t)nnz + 1, 1);
    static const int widths[cljp::NCLASS] = {8, 16, 32, 64, 64};
    for (int i = 0; i < n; ++i)
        if (Sp[i + 1] > Sp[i]) ++info[8 + cljp::size_class(Sp[i + 1] - Sp[i])];
    auto apply = [&](std::vector<int> &st) {                // cljp_apply_kernel; returns the U nodes that remain
        int u = 0;
        for (int i = 0; i < n; ++i) {
            if (cnt[(size_t)i]) { st[(size_t)i] = cljp::apply_node(st[(size_t)i], cnt[(size_t)i], &w[(size_t)i]); cnt[(size_t)i] = 0; }
            u += st[(size_t)i] == cljp::U_NODE;
        }
        return u;
    };
    int pass = 0;
    for (;;) {
        if (pass == n) return 8;
        ++pass;
        for (int i = 0; i < n; ++i) {                       // cljp_select_kernel: old state -> new state
            int s = a[(size_t)i];
            if (s == cljp::U_NODE && cljp::selects(i, Sp, Sj, Tp.data(), Tj.data(), w.data(), a.data())) { s = cljp::C_NODE; selpass[(size_t)i] = pass; }
            b[(size_t)i] = s;
        }
        a.swap(b);
        bool adjacent = false;
        for (int c = 0; c < n; ++c) {                       // cljp_p5_kernel
            if (selpass[(size_t)c] != pass) continue;
            for (int jj = Sp[c]; jj < Sp[c + 1]; ++jj) {
                adjacent = adjacent || (Sj[jj] != c && selpass[(size_t)Sj[jj]] == pass);
                if (cljp::p5_edge(c, jj, Sj, a.data(), mark.data())) { mark[(size_t)jj] = 0; ++cnt[(size_t)Sj[jj]]; }
            }
        }
        info[6] += adjacent;
        apply(a);
        for (int c = 0; c < cljp::NCLASS; ++c) {            // cljp_p6_kernel<W>: the groups one after another
            const int W = widths[c];
            for (int j = 0; j < n; ++j) {
                const int s0 = Sp[j], ns = Sp[j + 1] - s0;
                if (ns == 0 || cljp::size_class(ns) != c) continue;
                std::vector<int> stage((size_t)ns);
                int nst = 0;
                for (int lane = 0; lane < W; ++lane)
                    for (int t = lane; t < ns; t += W)
                        if (cljp::stages(j, Sj[s0 + t], selpass.data(), pass)) stage[(size_t)nst++] = Sj[s0 + t];
                if (!nst) continue;
                if (c == 4) ++info[5];
                for (int lane = 0; lane < W; ++lane)
                    for (int t = lane; t < ns; t += W)
                        if (cljp::p6_edge(j, s0 + t, Sp, Sj, a.data(), mark.data(), selpass.data(), pass, stage.data(), nst)) {
                            mark[(size_t)(s0 + t)] = 0;
                            ++cnt[(size_t)Sj[s0 + t]];
                            ++info[7];
                        }
            }
        }
        if (apply(a) == 0) break;
    }
    info[0] = pass;
    for (int i = 0; i < n; ++i) {
        splitting[i] = a[(size_t)i] == cljp::U_NODE ? cljp::F_NODE : a[(size_t)i];
        info[3] += splitting[i] == cljp::C_NODE;
    }
    return 0;
}

// the first `count` values of rand() after srand(the reference's seed)
void cje_rand_head(int count, int *out)
{
    srand(cljp::SEED);
    for (int i = 0; i < count; ++i) out[i] = rand();
}

}  // extern "C"

#ifdef CJE_MAIN
// the replay as a program of its own, for a build with -fsanitize=address,undefined: a 7 x 6 five-point grid with a hub row stored backwards
// and a few one-way edges, with and without colours, and the colouring alone
#include <cstdio>
int main()
{
    const int nx = 7, ny = 6, n = nx * ny;
    std::vector<int> Ap{0}, Aj;
    for (int i = 0; i < n; ++i) {
        const int x = i % nx, y = i / nx;
        if (i == 20) { for (int j = n - 1; j >= 0; --j) Aj.push_back(j); }
        else {
            if (y + 1 < ny && i + nx != 20) Aj.push_back(i + nx);
            if (x + 1 < nx && i + 1 != 20 && i % 5) Aj.push_back(i + 1);
            Aj.push_back(i);
            if (x > 0 && i - 1 != 20) Aj.push_back(i - 1);
            if (y > 0 && i - nx != 20) Aj.push_back(i - nx);
            if (i % 3) Aj.push_back(20);
        }
        Ap.push_back((int)Aj.size());
    }
    for (int colorflag = 0; colorflag < 2; ++colorflag) {
        std::vector<int> split((size_t)n, -7);
        int info[13];
        if (cje_cljp(n, Ap.data(), Aj.data(), colorflag, split.data(), info)) return 1;
        if (info[0] < 1 || info[0] > n || info[4] > n || info[3] < 1) return 2;
        for (int i = 0; i < n; ++i) if (split[(size_t)i] != 0 && split[(size_t)i] != 1) return 3;
    }
    std::vector<int> x((size_t)n, -7);
    int info[3];
    if (cje_vertex_coloring_mis(n, Ap.data(), Aj.data(), x.data(), info)) return 4;
    for (int i = 0; i < n; ++i) if (x[(size_t)i] < 0 || x[(size_t)i] >= info[0]) return 5;
    int empty = 0, none[13];
    if (cje_cljp(0, &empty, nullptr, 1, nullptr, none) != 0) return 6;
    std::printf("ok\n");
    return 0;
}
#endif
