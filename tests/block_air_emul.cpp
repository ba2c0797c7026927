// block_air_emul.cpp -- host replay of pyamg_amd/csrc/pamg_air_block.hip through the per-row arithmetic of pamg_air_block.h (over pamg_air.h):
// the lanes of a launch and the lanes of a group as loops, in the kernels' phase structure (per C-row: gather the columns and the b
// right-hand sides; per QR step the head by the owner of column j, the column updates and the row updates by their lanes; Q^T b by the
// lanes, the b back substitutions by b lanes, the blocks of R by the lanes), with the kernels' padded leading dimension.  Systems of
// order n = N * b beyond the 64-lane class take air_block::solve_serial, as inside the library.  Built by tests/test_block_air_host.py with
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC
#include "../pyamg_amd/csrc/pamg_air_block.h"

#include <vector>

using namespace pamg;

namespace {

// air_count_kernel + the host's pass over what did not fit a 64-entry slot
int count_row(int n, int c, const int *Cp, const int *Cj, const int *splitting, int distance)
{
    int slot[air::MAX_STAGED + 1];
    int N = air::neighbourhood(c, Cp, Cj, splitting, distance, slot, air::MAX_STAGED);
    if (N < 0) {
        std::vector<int> buf((size_t)n + 1);
        N = air::neighbourhood(c, Cp, Cj, splitting, distance, buf.data(), n);
    }
    return N;
}

// block_solve_kernel<W> for one group
void solve_group(int W, int N, int b, const int *Nf, int cpoint, const int *Ap, const int *Aj, const double *Ax, double *Rx)
{
    const int LD = W + 1, LDQ = W == 64 ? W : LD, n = N * b;
    std::vector<double> R((size_t)W * LD, -7.0), Q((size_t)W * LDQ, -7.0), v((size_t)W), b0((size_t)W * air_block::MAX_B, -7.0),
        rhs((size_t)W * air_block::MAX_B, -7.0);
    double hdr[2] = {0.0, 0.0};
    for (int lane = 0; lane < n; ++lane) {
        air_block::gather_column(lane, N, b, Nf, Ap, Aj, Ax, R.data(), LD);
        air_block::gather_rhs(lane, n, b, Nf, Ap, Aj, Ax, cpoint, b0.data());
        air::q_identity_row(lane, n, Q.data(), LDQ);
    }
    for (int j = 0; j < n; ++j) {
        for (int lane = 0; lane < W; ++lane)
            if (lane == j) {
                double tau = 0.0;
                const bool kept = air::qr_head(j, n, R.data(), LD, v.data(), &tau);
                hdr[0] = tau;
                hdr[1] = kept ? 1.0 : 0.0;
            }
        for (int lane = W - 1; lane >= 0; --lane)           // (any lane order: a lane touches its own column and its own row)
            if (lane < n && hdr[1] != 0.0) {
                if (lane >= j) air::qr_col(j, lane, n, R.data(), LD, v.data(), hdr[0]);
                air::qr_row(j, lane, n, Q.data(), LDQ, v.data(), hdr[0]);
            }
    }
    for (int lane = n - 1; lane >= 0; --lane)
        for (int r = 0; r < b; ++r) rhs[(size_t)(r * n + lane)] = air::rhs_entry(lane, n, b0.data() + r * n, Q.data(), LDQ);
    for (int lane = W - 1; lane >= 0; --lane)
        if (n > 0 && lane < b) air::back_substitute(n, R.data(), LD, rhs.data() + lane * n, b0.data() + lane * n);
    for (int lane = 0; lane < n; ++lane) air_block::store_solution(lane, n, b, b0.data(), Rx);
}

void solve_one_lane(int N, int b, const int *Nf, int cpoint, const int *Ap, const int *Aj, const double *Ax, double *Rx)
{
    const size_t m = (size_t)N * b;
    std::vector<double> R(m * m), Q(m * m), w(2 * m + (size_t)b * m);
    air_block::solve_serial(N, b, Nf, cpoint, Ap, Aj, Ax, R.data(), (int)m, Q.data(), (int)m, w.data(), w.data() + 2 * m, w.data() + m, Rx);
}

}  // namespace

extern "C" {

// -2: what the entry point refuses as unsupported
int bae_measure(int nblk, int b, int norm, const double *Ax, double *out)
{
    if (b > air_block::MAX_B || (norm == air_block::NORM_FRO && b == air_block::MAX_B)) return -2;
    for (int p = 0; p < nblk; ++p) out[p] = air_block::measure(norm, b, Ax + (size_t)p * b * b);
    return 0;
}

// one_lane != 0: every row by air_block::solve_serial.  classes[c] receives the number of C-rows of size class c (N > 0), classes[5] the
// largest order n.  -1: Rp does not agree with the counts, and nothing was written
int bae_pass2(int n, int nc, const int *Rp, int *Rj, double *Rx, const int *Ap, const int *Aj, const double *Ax, const int *Cp, const int *Cj,
              const int *Cpts, const int *splitting, int b, int distance, int one_lane, int *classes)
{
    static const int widths[4] = {8, 16, 32, 64};
    const int bb = b * b;
    std::vector<int> cnt((size_t)nc);
    for (int r = 0; r < nc; ++r) cnt[(size_t)r] = count_row(n, Cpts[r], Cp, Cj, splitting, distance);
    if (nc && Rp[0] != 0) return -1;
    for (int r = 0; r < nc; ++r) if (Rp[r + 1] - Rp[r] != cnt[(size_t)r] + 1) return -1;
    for (int p = 0; p < (nc ? Rp[nc] : 0); ++p) {
        Rj[p] = 0;
        for (int e = 0; e < bb; ++e) Rx[(size_t)p * bb + e] = 0.0;
    }
    for (int c = 0; c <= air::NCLASS; ++c) classes[c] = 0;
    for (int r = 0; r < nc; ++r) {                           // block_fill_kernel (and the host's rows)
        const int N = cnt[(size_t)r], r0 = Rp[r];
        if (air::neighbourhood(Cpts[r], Cp, Cj, splitting, distance, Rj + r0, N) != N) return -3;
        Rj[r0 + N] = Cpts[r];
        air_block::identity_block(b, Rx + (size_t)(r0 + N) * bb);
    }
    for (int r = 0; r < nc; ++r) {
        const int N = cnt[(size_t)r], r0 = Rp[r];
        if (N == 0) continue;
        const int c = N > air::MAX_STAGED ? 4 : air::size_class(N * b);
        ++classes[c];
        if (N * b > classes[5]) classes[5] = N * b;
        if (one_lane || c == 4) solve_one_lane(N, b, Rj + r0, Cpts[r], Ap, Aj, Ax, Rx + (size_t)r0 * bb);
        else solve_group(widths[c], N, b, Rj + r0, Cpts[r], Ap, Aj, Ax, Rx + (size_t)r0 * bb);
    }
    return 0;
}

}  // extern "C"

#ifdef BAE_MAIN
// the replay as a program of its own, for a build with -fsanitize=address,undefined: a hub (one C-point with N F-neighbours in a chain)
// for every block size and the orders on both sides of every lane-group boundary, lane groups against the single lane
#include <cstdio>
int main()
{
    static const int cases[][2] = {{1, 1}, {1, 8}, {1, 9}, {1, 17}, {1, 70}, {2, 4}, {2, 32}, {3, 3}, {3, 11}, {4, 8}, {5, 13}, {7, 9}, {8, 1}, {8, 2}, {8, 8}, {8, 9}};
    for (const auto &cs : cases) {
        const int b = cs[0], N = cs[1], n = N + 2, bb = b * b;
        std::vector<int> Ap{0}, Aj, split((size_t)n, 0), Cpts{0, n - 1};
        std::vector<double> Ax;
        split[0] = split[(size_t)n - 1] = 1;
        auto block = [&](int i, int j, double a) {
            Aj.push_back(j);
            for (int e = 0; e < bb; ++e) Ax.push_back(a * ((e % (b + 1) == 0 ? (i == j ? 1.0 : 0.5) : 0.0) + ((i * 7 + j * 3 + e) % 4) / 32.0));
        };
        for (int i = 0; i < n; ++i) {
            if (i == 0) {
                for (int j = N; j >= 0; --j) block(0, j, j == 0 ? 6.0 : -1.0 - (j % 4) / 4.0);       // (stored in descending order)
            } else if (i == n - 1) {
                block(i, i, 5.0);
            } else {
                if (i + 1 <= N) block(i, i + 1, -0.5);
                block(i, i, i % 5 == 3 ? 0.0 : 5.0);
                if (i > 1) block(i, i - 1, -0.75);
                block(i, 0, -1.0);
            }
            Ap.push_back((int)Aj.size());
        }
        for (int norm = 0; norm < 3; ++norm) {
            std::vector<double> m(Aj.size());
            const int rc = bae_measure((int)Aj.size(), b, norm, Ax.data(), m.data());
            if (rc != (norm == 2 && b == 8 ? -2 : 0)) return 1;
        }
        for (int distance = 1; distance <= 2; ++distance) {
            std::vector<int> Rp{0, N + 1, N + 2};
            const size_t nnz = (size_t)Rp[2];
            std::vector<int> Rj(nnz), Sj(nnz);
            std::vector<double> Rx(nnz * bb), Sx(nnz * bb);
            int classes[6];
            if (bae_pass2(n, 2, Rp.data(), Rj.data(), Rx.data(), Ap.data(), Aj.data(), Ax.data(), Ap.data(), Aj.data(), Cpts.data(), split.data(), b, distance, 0,
                          classes)) return 2;
            if (classes[5] != N * b) return 3;
            if (bae_pass2(n, 2, Rp.data(), Sj.data(), Sx.data(), Ap.data(), Aj.data(), Ax.data(), Ap.data(), Aj.data(), Cpts.data(), split.data(), b, distance, 1,
                          classes)) return 4;
            for (size_t p = 0; p < nnz; ++p) if (Rj[p] != Sj[p]) return 5;
            for (size_t p = 0; p < nnz * bb; ++p) if (!(Rx[p] == Sx[p])) return 6;
            Rp[1] += 1;
            if (bae_pass2(n, 2, Rp.data(), Rj.data(), Rx.data(), Ap.data(), Aj.data(), Ax.data(), Ap.data(), Aj.data(), Cpts.data(), split.data(), b, distance, 0,
                          classes) != -1) return 7;
        }
    }
    std::printf("ok\n");
    return 0;
}
#endif
