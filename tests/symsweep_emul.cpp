// CPU replay of the FUSED SYMMETRIC merged sweep (gs_lanem_sym_kernel, pyamg_amd/csrc/pamg_lane.hip): the forward and the backward plan of
// pamg_lanem_plan.h are walked in ONE "launch" by W waves in workgroups of four -- phase 1, the completion barrier that counts finished groups,
// phase 2 -- under the static and the ticket assignment, waves visited in the adversarial order (last wave first, one group per visit); several
// launches in a row on the same buffers, as a solver replays them.
// The kernel's buffer discipline: forward hand-off buffers H_f[0], H_f[1] alternating by a parity word, one backward buffer H_b.  Phase 1 reads old
// operands from x, publishes in H_f[parity] (x is not written) and wipes H_b; phase 2 reads old operands from H_f[parity], polls H_b, writes x and
// wipes H_f[parity ^ 1], the buffer of the next launch.  Wipe partition: n = q G + r, group g owns [g q + min(g, r), + q + (g < r)), the first group
// of every block of B consecutive groups wipes the block's entries.
// Asserted on the way: the replay terminates; no phase-2 group starts before every phase-1 group has finished and its workgroup has passed the
// barrier; the wipes cover every entry of the wiped buffer exactly once per phase, so H_b is all sentinels when the barrier opens and the next
// launch's forward buffer is at the end; no vector is written in a phase that reads old operands from it (x in phase 1, H_f[parity] in phase 2);
// polled operands are read only once published IN THIS phase of THIS launch (every buffer starts a launch full of values that would pass for
// published ones, except the one invariant: H_f[parity] all sentinels).
// The result of every launch must be the bits of the two directional sweeps replayed one after the other (snapshot of x in front of each).
// Test infrastructure only (tests/test_symsweep_plan.py).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../pyamg_amd/csrc/pamg_lanem_plan.h"
#include "../pyamg_amd/csrc/pamg_tile_plan.h"

using namespace pamg;

namespace {

const unsigned long long SENT = 0x7FF8DEADBEEF5A5Aull;
double sentinel() { double d; std::memcpy(&d, &SENT, 8); return d; }
bool is_sent(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u == SENT; }

// one group of plan P: operands polled in H, old ones read from `old`, returns -1 while an early operand is still a sentinel; val[r] = value of row r
int group_value(const LaneMPlan &P, int64_t g, const double *H, const double *old, const double *b, bool xz, double *val, char *need_old)
{
    const int RPW = P.rpw, LPR = 64 / RPW, K = P.K[(size_t)g];
    const size_t s0 = (size_t)P.unit[(size_t)g] * 64;
    if (K < 1 || K > LANEM_KMAX) return 33;
    for (int e = 0; e < K * 64; ++e) {
        const int c = P.cols[s0 + (size_t)e];
        if (!(c & LANE_NONE) && (c & LANE_EARLY) && is_sent(H[c & LANEM_MASK])) return -1;
    }
    double lane_sum[64];
    for (int lane = 0; lane < 64; ++lane) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) {
            const size_t e = s0 + (size_t)k * 64 + (size_t)lane;
            const int c = P.cols[e];
            if (c & LANE_NONE) continue;
            const int col = c & LANEM_MASK;
            double xv;
            if (c & LANE_EARLY) xv = H[col];
            else if (c & LANEM_BSRC) xv = b[col];
            else {
                if (xz) continue;                                       // x is known to be zero: an idle slot, product + 0
                if (need_old) need_old[col] = 1;
                xv = old[col];
            }
            s = s + P.vals[e] * xv;
        }
        lane_sum[lane] = s;
    }
    for (int step = 1; step < LPR; step *= 2) {
        double t[64];
        for (int lane = 0; lane < 64; ++lane) t[lane] = lane_sum[lane] + lane_sum[lane ^ step];
        for (int lane = 0; lane < 64; ++lane) lane_sum[lane] = t[lane];
    }
    for (int r = 0; r < RPW; ++r) {
        const int rid = P.rid[(size_t)(g * RPW + r)];
        if (rid < 0) { val[r] = 0.0; continue; }
        const int row = rid & LANE_MASK;
        val[r] = (rid & LANE_NODIAG) ? old[row] : (b[row] - lane_sum[r * LPR]) * P.rdiag[(size_t)(g * RPW + r)];
    }
    return 0;
}

int make_plan(int n, const int *Ap, const int *Aj, const double *Ax, int r0, int r1, int rs, int s_max, int rpw, LaneMPlan &P)
{
    std::vector<int> vis, lvl;
    int m = 0, nl = 0;
    if (sweep_levels(n, Ap, Aj, r0, r1, rs, vis, lvl, m, nl)) return 1;
    if (m != n) return 3;
    if (build_lanem_plan(n, Ap, Aj, Ax, r0, rs, m, nl, vis, lvl, s_max, 1e3, P, LANEM_KMAX * 64, rpw)) return 2;
    return 0;
}

// a directional sweep as the two-launch path runs it: sentinel fill, snapshot, groups in order
int directional(const LaneMPlan &P, int n, double *x, const double *b)
{
    std::vector<double> H((size_t)n, sentinel()), old(x, x + n);
    double val[2];
    for (int64_t g = 0; g < P.ngroups; ++g) {
        if (group_value(P, g, H.data(), old.data(), b, false, val, nullptr)) return 40;
        for (int r = 0; r < P.rpw; ++r) {
            const int rid = P.rid[(size_t)(g * P.rpw + r)];
            if (rid < 0) continue;
            H[(size_t)(rid & LANE_MASK)] = val[r];
            if (!(rid & LANE_NODIAG)) x[rid & LANE_MASK] = val[r];
        }
    }
    return 0;
}

}  // namespace

// x: in = the iterate, out = the result of `launches` fused replays; x2: out = the same number of (forward, backward) directional replays.
// ticket != 0: groups are drawn from a counter per phase (two tickets ahead), else wave w takes groups w, w + W, ...
// stats[8]: groups fwd, groups bwd, rounds, entries wiped in phase 1, in phase 2 (per launch), old operands read in phase 1, in phase 2, waves
extern "C" int symsweep_emul_f64(int n, const int *Ap, const int *Aj, const double *Ax, double *x, double *x2, const double *b, int s_max, int rpw,
                                 int waves, int ticket, int xzero, int launches, long long *stats)
{
    LaneMPlan PF, PB;
    int rc = make_plan(n, Ap, Aj, Ax, 0, n, 1, s_max, rpw, PF);
    if (rc) return rc;
    rc = make_plan(n, Ap, Aj, Ax, n - 1, -1, -1, s_max, rpw, PB);
    if (rc) return rc;
    const LaneMPlan *P[2] = {&PF, &PB};
    const int64_t G[2] = {PF.ngroups, PB.ngroups};
    int64_t B[2];
    for (int p = 0; p < 2; ++p) { B[p] = 1; while (B[p] * n < 64 * G[p]) B[p] *= 2; }      // groups per wipe block (the launcher's rule)
    waves = (waves + 3) / 4 * 4;
    const int W = waves, NWG = W / 4;
    // the state between launches: H_f[parity] all sentinels, the other two ANYTHING (here: values that would be taken for published ones)
    std::vector<double> Hf[2] = {std::vector<double>((size_t)n, sentinel()), std::vector<double>((size_t)n, 4321.0)}, Hb((size_t)n, 12345.0);
    int parity = 0;
    std::memcpy(x2, x, (size_t)n * sizeof(double));
    long long rounds = 0, o1 = 0, o2 = 0;
    std::vector<char> tmp;
    for (int launch = 0; launch < launches; ++launch) {
        if (directional(PF, n, x2, b) || directional(PB, n, x2, b)) return 40;
        double *HF = Hf[parity].data(), *HN = Hf[parity ^ 1].data();
        for (int j = 0; j < n; ++j) if (!is_sent(HF[j])) return 30;                        // the invariant between launches
        double *H[2] = {HF, Hb.data()};                                  // where phase p publishes and polls
        double *wipe[2] = {Hb.data(), HN};                               // what phase p wipes
        std::vector<int> wiped[2] = {std::vector<int>((size_t)n, 0), std::vector<int>((size_t)n, 0)};
        std::vector<char> old_read[2] = {std::vector<char>((size_t)n, 0), std::vector<char>((size_t)n, 0)};
        std::vector<char> pub[2] = {std::vector<char>((size_t)n, 0), std::vector<char>((size_t)n, 0)};
        struct Wave { int phase = 0; int64_t g = -1, g2 = -1; long long done = 0; };
        std::vector<Wave> wv((size_t)W);
        std::vector<long long> wg_done((size_t)NWG, 0);
        std::vector<int> wg_arrived((size_t)NWG, 0);
        std::vector<char> wg_passed((size_t)NWG, 0), wg_added((size_t)NWG, 0);
        long long counter = 0, tickets[2] = {0, 0}, finished[2] = {0, 0};
        auto draw = [&](int p) { return (int64_t)tickets[p]++; };
        // Wave::phase: 0 = walks phase 1, 1 = at the barrier, 2 = walks phase 2, 3 = gone
        auto start_phase = [&](Wave &w, int idx, int p) {
            w.phase = p == 0 ? 0 : 2;
            if (ticket) { w.g = draw(p); w.g2 = w.g < G[p] ? draw(p) : G[p]; }
            else { w.g = idx; w.g2 = idx + W; }
        };
        for (int i = 0; i < W; ++i) start_phase(wv[(size_t)i], i, 0);
        long long left = W;
        const bool xz = xzero && launch == 0;
        while (left > 0) {
            bool progress = false;
            ++rounds;
            for (int i = W - 1; i >= 0; --i) {                             // the adversarial order: the wave with the LATEST groups first
                Wave &w = wv[(size_t)i];
                const int wg = i / 4;
                if (w.phase == 3) continue;
                if (w.phase == 0 || w.phase == 2) {
                    const int p = w.phase == 0 ? 0 : 1;
                    if (w.g >= G[p]) {                                      // out of groups
                        if (p == 0) {
                            w.phase = 1;                                    // at the barrier: wait for stores, add to the workgroup's word
                            wg_done[(size_t)wg] += w.done;
                            wg_arrived[(size_t)wg]++;
                        } else { w.phase = 3; --left; }
                        progress = true;
                        continue;
                    }
                    if (p == 1 && (finished[0] != G[0] || counter != G[0] || !wg_passed[(size_t)wg])) return 21;      // a phase-2 group in front of the barrier
                    const double *old = p == 0 ? x : HF;                    // the vector this phase reads its old operands from
                    double val[2];
                    tmp.assign((size_t)n, 0);
                    const int rcg = group_value(*P[p], w.g, H[p], old, b, p == 0 && xz, val, tmp.data());
                    if (rcg > 0) return rcg;
                    if (rcg < 0) continue;                                  // still polling
                    for (int j = 0; j < n; ++j) if (tmp[(size_t)j]) old_read[p][(size_t)j] = 1;
                    // early operands must have been published in THIS phase (a stale value of an earlier sweep would also pass the sentinel test)
                    {
                        const LaneMPlan &Q = *P[p];
                        const size_t s0 = (size_t)Q.unit[(size_t)w.g] * 64;
                        for (int e = 0; e < Q.K[(size_t)w.g] * 64; ++e) {
                            const int c = Q.cols[s0 + (size_t)e];
                            if (!(c & LANE_NONE) && (c & LANE_EARLY) && !pub[p][(size_t)(c & LANEM_MASK)]) return 24;
                        }
                    }
                    for (int r = 0; r < P[p]->rpw; ++r) {
                        const int rid = P[p]->rid[(size_t)(w.g * P[p]->rpw + r)];
                        if (rid < 0) continue;
                        const int row = rid & LANE_MASK;
                        if (pub[p][(size_t)row]) return 14;
                        H[p][row] = val[r]; pub[p][(size_t)row] = 1;        // every row, a row without a diagonal its old value
                        if (H[p] == old) return 22;                         // a phase publishes in the vector it reads old operands from
                        if (p == 1 && !(rid & LANE_NODIAG)) x[row] = val[r];   // phase 1 does not write x: it reads its old operands there
                    }
                    // the wipe duty of group g: the entries of its block, if it is the block's first group
                    if (w.g % B[p] == 0) {
                        const int64_t q = n / G[p], r = n % G[p], g = w.g, g1 = std::min<int64_t>(g + B[p], G[p]);
                        const int64_t lo = g * q + (g < r ? g : r), hi = g1 * q + (g1 < r ? g1 : r);
                        if (lo < 0 || hi > n) return 25;
                        if (wipe[p] == old || wipe[p] == H[p]) return 23;   // a phase wipes a buffer it reads or publishes in
                        for (int64_t j = lo; j < hi; ++j) { wipe[p][j] = sentinel(); wiped[p][(size_t)j]++; }
                    }
                    ++w.done; ++finished[p];
                    w.g = w.g2;
                    w.g2 = ticket ? (w.g < G[p] ? draw(p) : G[p]) : w.g + W;
                    progress = true;
                    continue;
                }
                // w.phase == 1: the barrier.  The workgroup's one lane adds once its four waves have arrived, then polls; the others wait for it
                if (wg_arrived[(size_t)wg] == 4 && !wg_added[(size_t)wg]) { counter += wg_done[(size_t)wg]; wg_added[(size_t)wg] = 1; progress = true; }
                if (wg_added[(size_t)wg] && counter == G[0]) {
                    if (!wg_passed[(size_t)wg]) {
                        for (int j = 0; j < n; ++j) if (!is_sent(Hb[(size_t)j])) return 26;      // the barrier opens on a clean backward buffer
                        wg_passed[(size_t)wg] = 1;
                    }
                    w.done = 0;
                    start_phase(w, i, 1);
                    progress = true;
                }
            }
            if (!progress) return 20;                                       // deadlock
        }
        if (counter != G[0] || finished[0] != G[0] || finished[1] != G[1]) return 27;
        for (int p = 0; p < 2; ++p)
            for (int j = 0; j < n; ++j) if (wiped[p][(size_t)j] != 1) return 28 + p;            // every entry exactly once per phase
        for (int j = 0; j < n; ++j) if (!is_sent(HN[j])) return 31;                              // the next launch's forward buffer is clean
        if (std::memcmp(x, x2, (size_t)n * sizeof(double)) != 0) return 41 + launch;             // the bits of the two directional replays
        for (int j = 0; j < n; ++j) { o1 += old_read[0][(size_t)j]; o2 += old_read[1][(size_t)j]; }
        parity ^= 1;                                                     // the last workgroup to leave flips it
    }
    stats[0] = G[0]; stats[1] = G[1]; stats[2] = rounds; stats[3] = n; stats[4] = n; stats[5] = o1; stats[6] = o2; stats[7] = W;
    return 0;
}
