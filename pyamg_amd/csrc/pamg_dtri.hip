// pamg_dtri.hip -- the DENSE BLOCK-TRIANGULAR form of a symmetric Gauss-Seidel sweep from zero (plan and layout: pamg_dtri_plan.h).
//
// x = S b (or x += S b) as 2 nb block steps of two plain launches each: the sparse phase forms a block's right-hand side from the off-block slice
// and the values of the blocks already done, the dense phase multiplies it by the block's inverse triangle.  The first block of each direction has an
// empty slice, its dense phase reads the right-hand side itself: 4 nb - 2 launches.  No persistent grid, no flags, no counters: a launch boundary is
// the only hand-off, so the form cannot wait for anything and needs no co-residency.
//
// Every row sum has a fixed lane partition and an XOR butterfly (pamg_wave.h): two runs give the same bits.
#include "pamg_common.h"
#include "pamg_dtri_plan.h"
#include "pamg_wave.h"
#include "pamg_sweep_host.h"

namespace pamg {

struct DtriSched {
    int n = 0, B = 0, nb = 0;
    int *d_Lp = nullptr, *d_Lj = nullptr, *d_Up = nullptr, *d_Uj = nullptr;
    double *d_Lx = nullptr, *d_Ux = nullptr;
    double *d_W[2] = {nullptr, nullptr};        // Wf / Wb: the packed triangles of all blocks
    double *d_t = nullptr, *d_y = nullptr, *d_dy = nullptr, *d_z = nullptr;   // work vectors: a block's right-hand side, y, D y, z
    int64_t *d_woff = nullptr;
    unsigned long long *d_growth = nullptr;
    std::vector<int64_t> woff;
    int64_t tri_bytes = 0, off_block = 0;
    double growth = 0.0;
    float inverse_ms = 0.f;
    size_t bytes = 0;
};

namespace {

constexpr int DTRI_L = 16;                       // lanes per row of the sparse phase

// ---- plan time: the block inverses.  One thread per column j of block blockIdx.y, walking the block's rows in order:
//      W[i][j] = (delta_ij - sum_{j <= c < i} T[i][c] W[c][j]) / T[i][i] over the sparse in-block row (a thread reads what it wrote itself).
//      dir 1: triu(A_kk) in reversed local order.  The padding slot of an even row is zeroed by the thread of its diagonal.
__global__ __launch_bounds__(BLK) void dtri_inverse_kernel(const int *__restrict__ Ap, const int *__restrict__ Aj, const double *__restrict__ Ax,
                                                          const double *__restrict__ diag, int n, int B, const int64_t *__restrict__ woff,
                                                          double *W, int dir)
{
    const int k = blockIdx.y, lo = k * B, hi = min(lo + B, n), m = hi - lo;
    const int j0 = blockIdx.x * BLK;
    if (j0 >= m) return;
    const int j = j0 + threadIdx.x;
    double *Wk = W + woff[k];
    for (int i = j0; i < m; ++i) {
        if (j > i) continue;
        const int gi = dir ? hi - 1 - i : lo + i;
        const int64_t ro = dtri_row_off(i);
        double s = i == j ? 1.0 : 0.0;
        for (int p = Ap[gi]; p < Ap[gi + 1]; ++p) {
            const int gc = Aj[p];
            if (gc < lo || gc >= hi) continue;
            const int c = dir ? hi - 1 - gc : gc - lo;
            if (c >= i || c < j) continue;
            s = s - Ax[p] * Wk[dtri_row_off(c) + j];
        }
        Wk[ro + j] = s / diag[gi];
        if (i == j && !(i & 1)) Wk[ro + i + 1] = 0.0;
    }
}

// ---- plan time: the guard's figure max_i sum_j |W_ij| |a_jj| over all blocks of one direction.  One wave per row; the maximum of non-negative
//      doubles is the maximum of their bit patterns (a sum that is not finite counts as infinity)
__global__ __launch_bounds__(BLK) void dtri_growth_kernel(const double *__restrict__ diag, int n, int B, const int64_t *__restrict__ woff,
                                                         const double *__restrict__ W, int dir, unsigned long long *out)
{
    const int64_t r = ((int64_t)blockIdx.x * BLK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    const int k = (int)(r / B), lo = k * B, hi = min(lo + B, n), i = (int)r - lo;
    const double *Wr = W + woff[k] + dtri_row_off(i);
    double s = 0.0;
    for (int j = lane; j <= i; j += 64) s += fabs(Wr[j]) * fabs(diag[dir ? hi - 1 - j : lo + j]);
    s = seg_allreduce<64>(s);
    if (!(s <= 1.79e308)) s = INFINITY;
    if (lane == 0) atomicMax(out, (unsigned long long)__double_as_longlong(s));
}

// ---- sparse phase: t[l] = rhs[g] - slice[g, :] . v for the rows of one block, DTRI_L lanes per row; l: the local row (BWD: reversed)
template <bool BWD>
__global__ __launch_bounds__(BLK) void gs_dtri_sparse_kernel(const int *__restrict__ Sp, const int *__restrict__ Sj, const double *__restrict__ Sx,
                                                            const double *__restrict__ rhs, const double *__restrict__ v, double *__restrict__ t,
                                                            int lo, int hi)
{
    const int m = hi - lo;
    const int l = (blockIdx.x * BLK + threadIdx.x) / DTRI_L, lane = threadIdx.x & (DTRI_L - 1);
    const bool live = l < m;
    const int g = live ? (BWD ? hi - 1 - l : lo + l) : lo;
    const int p0 = live ? Sp[g] : 0, p1 = live ? Sp[g + 1] : 0;
    double s = 0.0;
    for (int p = p0 + lane; p < p1; p += DTRI_L) s += Sx[p] * v[Sj[p]];
    s = seg_allreduce<DTRI_L>(s);
    if (live && lane == 0) t[l] = rhs[g] - s;
}

// ---- dense phase: out[g(l)] = sum_{j <= l} W[l][j] t[j] for the rows of one block.  One workgroup per PAIR of rows (w, m - 1 - w): every workgroup
//      streams m + 1 values of the triangle (balanced), 16 bytes per lane and load, non-temporal (a triangle is read once per application); the two
//      rows are walked as ONE run of slots so that all loads of a thread are in flight together.  Fixed partition: slot q belongs to thread q mod 256,
//      a butterfly adds the lanes of a wave, thread 0 adds the four waves in order.
//      tglobal: t is the right-hand side vector itself (the first block of a direction: its slice is empty), indexed like the result.
//      forward (BWD = false): o1 = y, o2 = D y.   backward: o1 = z, o2 = x, acc: x += z instead of x = z
template <bool BWD>
__global__ __launch_bounds__(BLK) void gs_dtri_dense_kernel(const double *__restrict__ W, const double *__restrict__ t, int tglobal,
                                                           const double *__restrict__ diag, double *__restrict__ o1, double *o2, int acc,
                                                           int lo, int hi)
{
    typedef double d2 __attribute__((ext_vector_type(2)));
    static_assert(BLK == 256, "four waves per workgroup");
    __shared__ double part[4][2];
    const int m = hi - lo;
    const int w = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = w, i1 = m - 1 - w;                              // (w < (m + 1) / 2: i0 <= i1)
    const int nd0 = (i0 + 2) >> 1, nd1 = i0 == i1 ? 0 : (i1 + 2) >> 1;   // 16-byte slots of the two rows
    const d2 *W0 = reinterpret_cast<const d2 *>(W + dtri_row_off(i0)), *W1 = reinterpret_cast<const d2 *>(W + dtri_row_off(i1));
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
    for (int q = threadIdx.x; q < nd0 + nd1; q += BLK) {
        const bool second = q >= nd0;
        const int qq = second ? q - nd0 : q, i = second ? i1 : i0, j = 2 * qq;
        const d2 wv = __builtin_nontemporal_load((second ? W1 : W0) + qq);
        double v = wv.x * t[tglobal ? (BWD ? hi - 1 - j : lo + j) : j];
        if (j + 1 <= i) v += wv.y * t[tglobal ? (BWD ? hi - 2 - j : lo + j + 1) : j + 1];
        if (second) s1 += v; else s0 += v;
    }
    s0 = seg_allreduce<64>(s0);
    s1 = seg_allreduce<64>(s1);
    if (lane == 0) { part[wave][0] = s0; part[wave][1] = s1; }
    __syncthreads();
    if (threadIdx.x < (i0 == i1 ? 1 : 2)) {
        const int h = threadIdx.x, i = h ? i1 : i0;
        const double s = (part[0][h] + part[1][h]) + (part[2][h] + part[3][h]);
        const int g = BWD ? hi - 1 - i : lo + i;
        o1[g] = s;
        if (BWD) o2[g] = acc ? o2[g] + s : s;
        else o2[g] = diag[g] * s;
    }
}

}  // namespace

void free_dtri_part(DtriSched *t)
{
    if (!t) return;
    hipFree(t->d_Lp); hipFree(t->d_Lj); hipFree(t->d_Lx); hipFree(t->d_Up); hipFree(t->d_Uj); hipFree(t->d_Ux);
    hipFree(t->d_W[0]); hipFree(t->d_W[1]); hipFree(t->d_t); hipFree(t->d_y); hipFree(t->d_dy); hipFree(t->d_z);
    hipFree(t->d_woff); hipFree(t->d_growth);
    delete t;
}

// the form's shape conditions on the operator itself (f64, scalar rows, square, fast order, the automatic scheduler)
bool dtri_form_ok(const pamg_matrix_s *A)
{
    return A->dtype == PAMG_F64 && A->R == 1 && A->C == 1 && A->nrows == A->ncols && A->nrows >= 1 && A->nrows < INT32_MAX &&
           A->gs_order == 1 && A->gs_mode == 0 && !A->gs_prof && A->d_Ax && A->d_diag && !A->h_Ap.empty();
}

int dtri_block_rows(const pamg_matrix_s *A) { return A->dtri_block_rows > 0 ? A->dtri_block_rows : DTRI_BLOCK_ROWS; }

// bytes of the inverse triangles of ONE direction at block size B
int64_t dtri_tri_bytes(int64_t n, int B)
{
    const int64_t full = n / B, rest = n - full * B;
    return 8 * (full * dtri_tri_slots(B) + dtri_tri_slots(rest));
}

// the automatic rule's conditions on the operator (the solver adds its own: a level below the finest, symmetric Gauss-Seidel before and after)
bool dtri_auto_eligible(const pamg_matrix_s *A)
{
    if (!dtri_form_ok(A) || A->nrows <= ONE_XCD_MAX_ROWS || A->dtri_unfit) return false;
    const int64_t tri = dtri_tri_bytes(A->nrows, dtri_block_rows(A));
    return tri <= DTRI_AUTO_RATIO * (12 * A->nnz + 4 * (A->nrows + 1)) && 2 * tri <= DTRI_MAX_BYTES;
}

// Plan, slices, inverses and the growth guard.  Allocates and synchronises: at solver finalise or at a bare operator's first such sweep, never
// inside a graph capture.  PAMG_E_ARG: the form does not fit (A->dtri_unfit; A->dtri_declined_growth where the guard said so)
int build_dtri_part(pamg_matrix_s *A)
{
    if (A->dtri || A->dtri_unfit) return A->dtri ? PAMG_OK : PAMG_E_ARG;
    auto decline = [&](bool growth) { A->dtri_unfit = true; A->dtri_declined_growth = growth; return PAMG_E_ARG; };
    if (!dtri_form_ok(A)) return decline(false);
    const int n = (int)A->nrows, B = dtri_block_rows(A);
    if (2 * dtri_tri_bytes(n, B) > DTRI_MAX_BYTES || (n + B - 1) / B > 65535) return decline(false);       // (blocks are a grid dimension of the inverse kernel)
    PhaseTimer pt_("build_dtri_part", A->nnz);
    std::vector<double> hAx((size_t)A->nnz + 1);
    if (A->nnz) PAMG_HIP(hipMemcpy(hAx.data(), A->d_Ax, (size_t)A->nnz * sizeof(double), hipMemcpyDeviceToHost));
    DtriPlan P;
    if (build_dtri_plan(n, A->h_Ap.data(), A->h_Aj.data(), hAx.data(), B, P) != DTRI_OK) return decline(false);
    hAx = std::vector<double>();
    DtriSched *t = new (std::nothrow) DtriSched();
    if (!t) return PAMG_E_ALLOC;
    t->n = n; t->B = B; t->nb = P.nb; t->woff = P.woff; t->off_block = P.off_block_entries();
    const size_t wb = (size_t)P.woff[(size_t)P.nb] * sizeof(double), vb = ((size_t)n + 8) * sizeof(double);
    t->tri_bytes = 2 * (int64_t)wb;
    int st = device_upload(&t->d_Lp, P.Lp.data(), P.Lp.size() * sizeof(int), &t->bytes);
    if (!st) st = device_upload(&t->d_Lj, P.Lj.data(), P.Lj.size() * sizeof(int), &t->bytes);
    if (!st) st = device_upload(&t->d_Lx, P.Lx.data(), P.Lx.size() * sizeof(double), &t->bytes);
    if (!st) st = device_upload(&t->d_Up, P.Up.data(), P.Up.size() * sizeof(int), &t->bytes);
    if (!st) st = device_upload(&t->d_Uj, P.Uj.data(), P.Uj.size() * sizeof(int), &t->bytes);
    if (!st) st = device_upload(&t->d_Ux, P.Ux.data(), P.Ux.size() * sizeof(double), &t->bytes);
    if (!st) st = device_upload(&t->d_woff, P.woff.data(), P.woff.size() * sizeof(int64_t), &t->bytes);
    if (!st) st = device_upload(&t->d_growth, nullptr, 2 * sizeof(unsigned long long), &t->bytes);
    for (int d = 0; d < 2 && !st; ++d) st = device_upload(&t->d_W[d], nullptr, wb, &t->bytes);
    if (!st) st = device_upload(&t->d_t, nullptr, ((size_t)B + 8) * sizeof(double), &t->bytes);
    if (!st) st = device_upload(&t->d_y, nullptr, vb, &t->bytes);
    if (!st) st = device_upload(&t->d_dy, nullptr, vb, &t->bytes);
    if (!st) st = device_upload(&t->d_z, nullptr, vb, &t->bytes);
    if (!st) st = (int)hipMemset(t->d_growth, 0, 2 * sizeof(unsigned long long));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!st) st = (int)hipEventCreate(&e0);
    if (!st) st = (int)hipEventCreate(&e1);
    if (!st) {
        const int m = std::min(B, n);
        hipEventRecord(e0, 0);
        for (int d = 0; d < 2; ++d)
            hipLaunchKernelGGL(dtri_inverse_kernel, dim3((m + BLK - 1) / BLK, P.nb), dim3(BLK), 0, 0, (const int *)A->d_Ap, (const int *)A->d_Aj,
                               (const double *)A->d_Ax, (const double *)A->d_diag, n, B, (const int64_t *)t->d_woff, t->d_W[d], d);
        hipEventRecord(e1, 0);
        const unsigned gg = (unsigned)(((int64_t)n * 64 + BLK - 1) / BLK);
        for (int d = 0; d < 2; ++d)
            hipLaunchKernelGGL(dtri_growth_kernel, dim3(gg), dim3(BLK), 0, 0, (const double *)A->d_diag, n, B, (const int64_t *)t->d_woff,
                               (const double *)t->d_W[d], d, t->d_growth + d);
        st = (int)hipGetLastError();
    }
    unsigned long long gbits[2] = {0, 0};
    if (!st) st = (int)hipMemcpy(gbits, t->d_growth, sizeof(gbits), hipMemcpyDeviceToHost);       // (synchronises)
    if (!st) hipEventElapsedTime(&t->inverse_ms, e0, e1);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    if (st) { free_dtri_part(t); return st; }
    double g[2];
    memcpy(g, gbits, sizeof(g));
    t->growth = std::max(g[0], g[1]);
    A->dtri_growth = t->growth;
    if (!(t->growth <= DTRI_GROWTH_CAP)) { free_dtri_part(t); return decline(true); }
    A->dtri = t;
    return PAMG_OK;
}

size_t dtri_part_bytes(const pamg_matrix_s *A) { return A->dtri ? A->dtri->bytes : 0; }

int dtri_launches(const DtriSched *t) { return 4 * t->nb - 2; }

// x = S b (acc = false) or x += S b (acc = true; b must not be x)
int dtri_sym_launch(pamg_matrix_s *A, void *x_, const void *b_, bool acc, hipStream_t s)
{
    DtriSched *t = A->dtri;
    if (!t) return PAMG_E_STATE;
    double *x = (double *)x_;
    const double *b = (const double *)b_, *diag = (const double *)A->d_diag;
    const int n = t->n, B = t->B, nb = t->nb;
    auto grids = [&](int m, unsigned &gs, unsigned &gd) {
        gs = (unsigned)(((int64_t)m * DTRI_L + BLK - 1) / BLK);
        gd = (unsigned)((m + 1) / 2);
    };
    for (int k = 0; k < nb; ++k) {
        const int lo = k * B, hi = std::min(lo + B, n);
        unsigned gs, gd;
        grids(hi - lo, gs, gd);
        if (k > 0)
            hipLaunchKernelGGL((gs_dtri_sparse_kernel<false>), dim3(gs), dim3(BLK), 0, s, (const int *)t->d_Lp, (const int *)t->d_Lj, (const double *)t->d_Lx,
                               b, (const double *)t->d_y, t->d_t, lo, hi);
        hipLaunchKernelGGL((gs_dtri_dense_kernel<false>), dim3(gd), dim3(BLK), 0, s, (const double *)(t->d_W[0] + t->woff[(size_t)k]),
                           k > 0 ? (const double *)t->d_t : b, k > 0 ? 0 : 1, diag, t->d_y, t->d_dy, 0, lo, hi);
    }
    for (int k = nb - 1; k >= 0; --k) {
        const int lo = k * B, hi = std::min(lo + B, n);
        unsigned gs, gd;
        grids(hi - lo, gs, gd);
        if (k < nb - 1)
            hipLaunchKernelGGL((gs_dtri_sparse_kernel<true>), dim3(gs), dim3(BLK), 0, s, (const int *)t->d_Up, (const int *)t->d_Uj, (const double *)t->d_Ux,
                               (const double *)t->d_dy, (const double *)t->d_z, t->d_t, lo, hi);
        hipLaunchKernelGGL((gs_dtri_dense_kernel<true>), dim3(gd), dim3(BLK), 0, s, (const double *)(t->d_W[1] + t->woff[(size_t)k]),
                           k < nb - 1 ? (const double *)t->d_t : (const double *)t->d_dy, k < nb - 1 ? 0 : 1, diag, t->d_z, x, acc ? 1 : 0, lo, hi);
    }
    return (int)hipGetLastError();
}

// info[0..15] = built, blocks, block rows, bytes of Wf + Wb, off-block entries, launches from zero, launches in correction form, auto-eligible,
// declined by growth, microseconds of the inverse kernels, mode, kernel launches per application, bytes the form added to the operator's account
// (triangles, slices, work vectors), 0, 0, 0; *growth = the guard's figure (0 = not computed)
int dtri_info(const pamg_matrix_s *A, int64_t *info, double *growth)
{
    for (int i = 0; i < 16; ++i) info[i] = 0;
    const DtriSched *t = A->dtri;
    if (t) {
        info[0] = 1; info[1] = t->nb; info[2] = t->B; info[3] = t->tri_bytes; info[4] = t->off_block;
        info[9] = (int64_t)(1e3 * (double)t->inverse_ms); info[11] = dtri_launches(t); info[12] = (int64_t)t->bytes;
    }
    info[5] = A->dtri_zero_launches; info[6] = A->dtri_correction_launches;
    info[7] = dtri_auto_eligible(A) ? 1 : 0; info[8] = A->dtri_declined_growth ? 1 : 0; info[10] = A->dtri_mode;
    if (growth) *growth = A->dtri_growth;
    return PAMG_OK;
}

}  // namespace pamg
