// CPU replay of the CLUSTER layout of the merged lane-parallel Gauss-Seidel sweep (pyamg_amd/csrc/pamg_lanem_plan.h, cluster = 4 / 8): the plan is
// consumed the way c_group (pamg_lane.hip) consumes it -- group after group: the unique operands into a 512-entry buffer (early ones from the hand-off
// buffer, old ones from the snapshot / the forward iterate, b operands from b), every lane its slots from that buffer, a segmented inclusive scan over
// the lanes of a row, (b - sum) * (1 / a_ii) in the row's last lane -- and asserts what the device relies on: every visited row sits in exactly one
// group, slot indices stay below the group's unique count, a lane serves one row and a row consecutive lanes, polled operands come from EARLIER
// super-levels and smaller group numbers (deadlock freedom for any number of waves, visited in the adversarial order), gates are ancestors.
// Test infrastructure only (tests/test_lanec_plan.py).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../pyamg_amd/csrc/pamg_lanem_plan.h"
#include "../pyamg_amd/csrc/pamg_tile_plan.h"

using namespace pamg;

namespace {

struct Phase {
    const LaneMPlan *P;
    const double *xold;     // OLD operands (and the value of a row without a diagonal)
    double *xs;             // hand-off buffer
    double *y;              // the iterate that is written, or nullptr (first phase of the fused sweep)
    const double *b;
    bool xz;                // x known to be zero: OLD operands are not read
    int n;
};

// returns 0, a positive error code, or -1 (still polling; may_wait only)
int run_group(const Phase &ph, int64_t g, bool may_wait, std::vector<char> &pub, std::vector<int> &sup_pub, int64_t &rows_done)
{
    const LaneMPlan &P = *ph.P;
    const int R = P.cluster, KU = P.c_KU[(size_t)g], KS = P.c_KS[(size_t)g], nr = P.c_rows[(size_t)g];
    if (KU < 1 || KU > LANEM_KMAX || KS < 1 || KS > LANEM_KMAX || nr < 1 || nr > R) return 33;
    const int *uc = P.ucodes.data() + (size_t)P.c_uunit[(size_t)g] * 64;
    const double *sv = P.svals.data() + (size_t)P.c_sunit[(size_t)g] * 64;
    const unsigned short *si = P.sidx.data() + (size_t)P.c_sunit[(size_t)g] * 64;
    int nu = 0;
    for (int u = 0; u < KU * 64; ++u) {
        if (uc[u] & LANE_NONE) continue;
        if (u != nu) return 40;                                            // the unique operands come first, padding behind them
        if (u && !((unsigned)uc[u - 1] < (unsigned)uc[u])) return 41;      // sorted by (kind, column), no operand twice
        ++nu;
    }
    if (may_wait) {
        for (int u = 0; u < nu; ++u)
            if ((uc[u] & LANE_EARLY) && !pub[(size_t)(uc[u] & LANEM_MASK)]) return -1;     // still polling
        const int gt = P.gate[(size_t)g];
        if (gt >= 0 && !pub[(size_t)gt]) return 16;                       // every operand is there but the gate is not: the gate is not an ancestor
    }
    double lds[LANEC_UMAX];
    for (int u = 0; u < KU * 64; ++u) {
        const int c = uc[u];
        if (c & LANE_NONE) { lds[u] = 0.0; continue; }
        const int col = c & LANEM_MASK;
        if (col >= ph.n) return 42;
        if (c & LANE_EARLY) {
            if (c & LANEM_BSRC) return 18;
            if (!pub[(size_t)col]) return 12;                             // producer has a larger group number: deadlock on the device
            if (sup_pub[(size_t)col] >= P.super_of[(size_t)g]) return 19; // polled operands come from EARLIER super-levels
            lds[u] = ph.xs[(size_t)col];
        } else if (c & LANEM_BSRC) lds[u] = ph.b[col];
        else lds[u] = ph.xz ? 0.0 : ph.xold[(size_t)col];
    }
    double s[64];
    int tag[64];
    std::vector<char> used((size_t)nu, 0);
    for (int lane = 0; lane < 64; ++lane) {
        const unsigned t0 = si[lane];
        tag[lane] = (t0 & LANEC_UNUSED) ? -1 : (int)((t0 >> LANEC_ROWSHIFT) & 7u);
        if (tag[lane] >= nr) return 43;
        double acc = 0.0;
        for (int k = 0; k < KS; ++k) {
            const unsigned t = si[(size_t)k * 64 + (size_t)lane];
            const int tg = (t & LANEC_UNUSED) ? -1 : (int)((t >> LANEC_ROWSHIFT) & 7u);
            if (tg != tag[lane]) return 44;                                // a lane serves one row
            if (t & LANEC_PAD) { if (sv[(size_t)k * 64 + (size_t)lane] != 0.0) return 11; continue; }
            const int u = (int)(t & LANEC_IDX);
            if (u >= nu) return 45;                                        // slot index below the group's unique count
            const int rid = P.rid[(size_t)(g * R + tg)];
            if (rid < 0 || (rid & LANE_NODIAG)) return 17;                 // an untouched row carries no operands
            used[(size_t)u] = 1;
            const double pr = sv[(size_t)k * 64 + (size_t)lane] * lds[u];
            acc = acc + pr;
        }
        s[lane] = acc;
    }
    for (int u = 0; u < nu; ++u) if (!used[(size_t)u]) return 46;          // nothing is loaded for nothing
    int seglo[64];
    for (int lane = 0; lane < 64; ++lane) {
        seglo[lane] = (lane == 0 || tag[lane - 1] != tag[lane]) ? lane : seglo[lane - 1];
        if (lane && tag[lane] != tag[lane - 1] && tag[lane] != -1 && tag[lane] != tag[lane - 1] + 1) return 47;     // rows own consecutive lanes, in order
    }
    if (tag[0] != 0) return 47;
    for (int d = 1; d < 64; d *= 2) {
        double t[64];
        for (int lane = 0; lane < 64; ++lane) t[lane] = s[lane] + ((lane - d >= seglo[lane]) ? s[lane - d] : 0.0);
        for (int lane = 0; lane < 64; ++lane) s[lane] = t[lane];
    }
    int published = 0;
    for (int lane = 0; lane < 64; ++lane) {
        const bool tail = lane == 63 || tag[lane + 1] != tag[lane];
        if (!tail || tag[lane] < 0) continue;
        const int rid = P.rid[(size_t)(g * R + tag[lane])];
        if (rid < 0) return 48;
        const int row = rid & LANE_MASK;
        const bool upd = !(rid & LANE_NODIAG);
        double v = (ph.b[row] - s[lane]) * P.rdiag[(size_t)(g * R + tag[lane])];
        if (!upd) v = ph.xold[(size_t)row];
        if (pub[(size_t)row]) return 14;                                   // every visited row in exactly one group
        ph.xs[(size_t)row] = v; pub[(size_t)row] = 1; sup_pub[(size_t)row] = P.super_of[(size_t)g];
        if (ph.y && upd) ph.y[row] = v;
        ++rows_done; ++published;
    }
    if (published != nr) return 49;
    for (int r = nr; r < R; ++r) if (P.rid[(size_t)(g * R + r)] != -1) return 50;
    return 0;
}

int run_phase(const Phase &ph, int waves, int64_t m)
{
    const LaneMPlan &P = *ph.P;
    std::vector<char> pub((size_t)ph.n, 0);
    std::vector<int> sup_pub((size_t)ph.n, -1);
    int64_t rows_done = 0;
    for (int64_t g = 0; g + 1 < P.ngroups; ++g) {
        if (P.c_uunit[(size_t)g] + P.c_KU[(size_t)g] != P.c_uunit[(size_t)g + 1]) return 30;
        if (P.c_sunit[(size_t)g] + P.c_KS[(size_t)g] != P.c_sunit[(size_t)g + 1]) return 30;
        if (P.super_of[(size_t)g] > P.super_of[(size_t)g + 1]) return 31;
    }
    for (int s = 0; s < P.nsuper; ++s)
        for (int64_t g = P.super_grp[(size_t)s]; g < P.super_grp[(size_t)s + 1]; ++g) if (P.super_of[(size_t)g] != s) return 32;
    if (waves <= 0) {
        for (int64_t g = 0; g < P.ngroups; ++g) { const int rc = run_group(ph, g, false, pub, sup_pub, rows_done); if (rc) return rc; }
    } else {
        std::vector<int64_t> next((size_t)waves);
        for (int w = 0; w < waves; ++w) next[(size_t)w] = w;
        int64_t left = P.ngroups;
        while (left > 0) {
            bool progress = false;
            for (int w = waves - 1; w >= 0; --w) {
                int64_t &g = next[(size_t)w];
                if (g >= P.ngroups) continue;
                const int rc = run_group(ph, g, true, pub, sup_pub, rows_done);
                if (rc > 0) return rc;
                if (rc == 0) { g += waves; --left; progress = true; }
            }
            if (!progress) return 20;
        }
    }
    if (rows_done != m) return 15;
    return 0;
}

void fill_stats(const LaneMPlan &P, long long *st)
{
    st[0] = P.nsuper; st[1] = P.nlevels; st[2] = P.nrows; st[3] = P.n_sunits; st[4] = P.n_early; st[5] = P.n_old; st[6] = P.n_b; st[7] = P.n_direct;
    st[8] = P.max_len; st[9] = P.closed_by_length; st[10] = P.closed_by_growth; st[11] = P.ngroups; st[12] = P.n_uunits; st[13] = P.n_uearly;
    st[14] = P.n_uold; st[15] = P.n_ub; st[16] = P.n_early_lines; st[17] = P.n_sunits * 64;
}

int plan(int n, const int *Ap, const int *Aj, const double *Ax, int row_start, int row_stop, int row_step, int s_max, double growth_cap, int cluster,
         LaneMPlan &P, int &m)
{
    std::vector<int> vis, lvl;
    int nl = 0;
    m = 0;
    if (sweep_levels(n, Ap, Aj, row_start, row_stop, row_step, vis, lvl, m, nl)) return 1;
    if (m == 0) return 0;
    if (build_lanem_plan(n, Ap, Aj, Ax, row_start, row_step, m, nl, vis, lvl, s_max, growth_cap, P, LANEM_KMAX * 64, 1, cluster)) return 2;
    if (P.nrows != m || P.cluster != cluster) return 34;
    return 0;
}

}  // namespace

// stats[18]: 0 nsuper, 1 nlevels, 2 rows, 3 slot units, 4 early, 5 old, 6 b operands, 7 direct entries, 8 max_len, 9 / 10 closed by length / growth,
//            11 groups, 12 units of unique operands, 13 / 14 / 15 unique early / old / b operands, 16 early lines, 17 padded slots
// One directional sweep of x (the snapshot of x is taken here, as lanem_prepare_kernel does).  xz: the OLD operands are not read.
extern "C" int lanec_emul_sweep_f64(int n, const int *Ap, const int *Aj, const double *Ax, double *x, const double *b, int row_start, int row_stop,
                                    int row_step, int s_max, double growth_cap, int cluster, long long *stats, int waves, int xz)
{
    LaneMPlan P;
    int m = 0;
    const int rc = plan(n, Ap, Aj, Ax, row_start, row_stop, row_step, s_max, growth_cap, cluster, P, m);
    if (rc || m == 0) return rc;
    fill_stats(P, stats);
    std::vector<double> xs((size_t)n, 0.0), xold(x, x + n);
    Phase ph{&P, xold.data(), xs.data(), x, b, xz != 0, n};
    return run_phase(ph, waves, m);
}

// The fused symmetric sweep over all rows (gs_lanem_sym_kernel): phase 1 = the forward schedule, OLD operands from x, every row published in H_f, x
// not written; phase 2 = the backward schedule, OLD operands from H_f, x written.  stats: of the forward plan, then [18..35] of the backward plan.
extern "C" int lanec_emul_sym_f64(int n, const int *Ap, const int *Aj, const double *Ax, double *x, const double *b, int s_max, double growth_cap,
                                  int cluster, long long *stats, int waves, int xz)
{
    LaneMPlan Pf, Pb;
    int mf = 0, mb = 0;
    int rc = plan(n, Ap, Aj, Ax, 0, n, 1, s_max, growth_cap, cluster, Pf, mf);
    if (rc) return rc;
    rc = plan(n, Ap, Aj, Ax, n - 1, -1, -1, s_max, growth_cap, cluster, Pb, mb);
    if (rc) return 100 + rc;
    if (mf != n || mb != n) return 35;
    fill_stats(Pf, stats);
    fill_stats(Pb, stats + 18);
    std::vector<double> hf((size_t)n, 0.0), hb((size_t)n, 0.0);
    Phase p1{&Pf, x, hf.data(), nullptr, b, xz != 0, n};
    rc = run_phase(p1, waves, mf);
    if (rc) return rc;
    Phase p2{&Pb, hf.data(), hb.data(), x, b, false, n};
    rc = run_phase(p2, waves, mb);
    return rc ? 200 + rc : 0;
}
