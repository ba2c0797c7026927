// pamg_schwarz_setup.hip -- the setup of overlapping Schwarz on the device: the dense diagonal block A[S_d, S_d] of every
// subdomain (amg_core::extract_subblocks, relaxation.h:1333-1396) and its pseudo-inverse (what the reference's
// schwarz_parameters gets from one LAPACK gelss call per subdomain, relaxation.py:1060-1074).
//
//   plan     one workgroup: the block pointer Tp (exclusive scan of m^2, 64-bit), the largest m, and the subdomains listed by
//            size class (m <= 8 / 16 / 32 / 64), in their own order -- no atomics, the same lists on every run
//   extract  a group of W lanes (W = the class width) per subdomain: its row list staged in LDS, rows one after another, lanes
//            over the stored entries of the row, binary search of the column in the list; values are copied
//   pinv     the same groups: one-sided Jacobi SVD of the block with U and V in LDS, lane i owns row i of both (column-major
//            with leading dimension W: lane-contiguous, no bank conflicts), column dot products by butterfly shuffles.  One
//            wave per workgroup; the groups of a wave walk the pair loop together (its bounds are the wave's maxima and the
//            shuffles are never under a divergent branch), a finished group idles.  The arithmetic is pamg_dense_pinv.h.
#include "pamg_common.h"
#include "pamg_dense_pinv.h"
#include "pamg_host_call.h"

using namespace pamg;

namespace {

// control words of one call (device, 64-bit)
enum : int { CW_TOTAL = 0, CW_MAXM, CW_SWEEPS, CW_TRUNC, CW_BAD, CW_NOCONV, CW_COUNT0, CW_WORDS = CW_COUNT0 + dpinv::NCLASS };

constexpr int PLAN_T = 256;

__global__ __launch_bounds__(PLAN_T) void schwarz_plan_kernel(int nsub, const int *__restrict__ Sp, long long *__restrict__ tp64,
                                                              int *__restrict__ lists, unsigned long long *__restrict__ cw)
{
    __shared__ long long s_sq[PLAN_T];
    __shared__ int s_cnt[dpinv::NCLASS][PLAN_T];
    __shared__ int s_max[PLAN_T], s_bad[PLAN_T];
    const int t = threadIdx.x;
    const int chunk = (nsub + PLAN_T - 1) / PLAN_T;
    const int d0 = min(nsub, t * chunk), d1 = min(nsub, d0 + chunk);
    long long sq = 0;
    int cnt[dpinv::NCLASS] = {0, 0, 0, 0}, mx = 0, bad = 0;
    for (int d = d0; d < d1; ++d) {
        const int m = Sp[d + 1] - Sp[d];
        if (m < 0 || Sp[d] < 0) { bad = 1; continue; }
        sq += (long long)m * m;
        mx = max(mx, m);
        if (m > 0 && m <= dpinv::MAX_M) ++cnt[dpinv::size_class(m)];
    }
    s_sq[t] = sq; s_max[t] = mx; s_bad[t] = bad;
    for (int c = 0; c < dpinv::NCLASS; ++c) s_cnt[c][t] = cnt[c];
    __syncthreads();
    if (t == 0) {                                      // exclusive scans over the 256 chunks
        long long run = 0;
        int rc[dpinv::NCLASS] = {0, 0, 0, 0}, m_all = 0, b_all = 0;
        for (int i = 0; i < PLAN_T; ++i) {
            const long long v = s_sq[i];
            s_sq[i] = run;
            run += v;
            for (int c = 0; c < dpinv::NCLASS; ++c) { const int n = s_cnt[c][i]; s_cnt[c][i] = rc[c]; rc[c] += n; }
            m_all = max(m_all, s_max[i]);
            b_all |= s_bad[i];
        }
        tp64[nsub] = run;
        cw[CW_TOTAL] = (unsigned long long)run;
        cw[CW_MAXM] = (unsigned long long)m_all;
        cw[CW_SWEEPS] = 0; cw[CW_TRUNC] = 0; cw[CW_NOCONV] = 0;
        cw[CW_BAD] = (unsigned long long)b_all;
        for (int c = 0; c < dpinv::NCLASS; ++c) cw[CW_COUNT0 + c] = (unsigned long long)rc[c];
    }
    __syncthreads();
    long long at = s_sq[t];
    int pos[dpinv::NCLASS];
    for (int c = 0; c < dpinv::NCLASS; ++c) pos[c] = s_cnt[c][t];
    for (int d = d0; d < d1; ++d) {
        const int m = Sp[d + 1] - Sp[d];
        tp64[d] = at;
        if (m < 0 || Sp[d] < 0) continue;
        at += (long long)m * m;
        if (m > 0 && m <= dpinv::MAX_M) {
            const int c = dpinv::size_class(m);
            lists[(size_t)c * nsub + pos[c]++] = d;
        }
    }
}

__global__ __launch_bounds__(256) void schwarz_tp_narrow_kernel(int n1, const long long *__restrict__ tp64, int *__restrict__ Tp)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n1) Tp[i] = (int)tp64[i];
}

// A[S_d, S_d] of the listed subdomains into Tx (zero-filled by the caller).  256 / W groups per workgroup.
template <typename T, int W>
__global__ __launch_bounds__(256) void schwarz_extract_kernel(const int *__restrict__ list, int count, const int *__restrict__ Sp,
                                                              const int *__restrict__ Sj, const int *__restrict__ Tp, int nrows,
                                                              const int *__restrict__ Ap, const int *__restrict__ Aj, const T *__restrict__ Ax,
                                                              T *__restrict__ Tx, unsigned long long *__restrict__ cw)
{
    __shared__ int s_S[256];
    const int g = threadIdx.x / W, l = threadIdx.x % W;
    const long long slot = (long long)blockIdx.x * (256 / W) + g;
    const int d = slot < count ? list[slot] : -1;
    int m = 0;
    if (d >= 0) {
        const int s0 = Sp[d];
        m = Sp[d + 1] - s0;                       // 1 .. W by the plan
        if (l < m) s_S[g * W + l] = Sj[s0 + l];
    }
    __syncthreads();
    if (d < 0) return;
    const int *S = s_S + g * W;
    T *blk = Tx + Tp[d];
    for (int r = 0; r < m; ++r) {
        const int row = S[r];
        if (row < 0 || row >= nrows) {            // not a row of A: refuse the call, touch nothing
            if (l == 0) atomicOr(&cw[CW_BAD], 1ull);
            continue;
        }
        const int a0 = Ap[row], a1 = Ap[row + 1];
        for (int k = a0 + l; k < a1; k += W) {
            const int c = dpinv::extract_target(Aj, a0, k, S, m);
            if (c >= 0) blk[r * m + c] = Ax[k];
        }
    }
}

template <typename T, int W>
__device__ __forceinline__ T group_sum(T v)
{
    dpinv::butterfly_offsets<W>([&](int off) { v += __shfl_xor(v, off, W); });
    return v;
}

template <typename T, int W>
__device__ __forceinline__ T group_max(T v)
{
    dpinv::butterfly_offsets<W>([&](int off) { v = fmax(v, __shfl_xor(v, off, W)); });
    return v;
}

// every listed block replaced by its pseudo-inverse.  One wave per workgroup, 64 / W groups per wave.
template <typename T, int W>
__global__ __launch_bounds__(64) void schwarz_pinv_kernel(const int *__restrict__ list, int count, const int *__restrict__ Sp,
                                                          const int *__restrict__ Tp, T *__restrict__ Tx, T rank_tol, int sweep_cap,
                                                          unsigned long long *__restrict__ cw)
{
    constexpr int NG = 64 / W;
    __shared__ T s_U[NG * W * W], s_V[NG * W * W];
    const int g = threadIdx.x / W, i = threadIdx.x % W;
    const long long slot = (long long)blockIdx.x * NG + g;
    const int d = slot < count ? list[slot] : -1;
    const int m = d >= 0 ? Sp[d + 1] - Sp[d] : 0;
    T *U = s_U + g * W * W, *V = s_V + g * W * W;
    T *blk = d >= 0 ? Tx + Tp[d] : nullptr;
    for (int e = i; e < W * W; e += W) {                   // column e / W, row i: lane-contiguous
        U[e] = T(0);
        V[e] = (e / W == i) ? T(1) : T(0);
    }
    __syncthreads();
    for (int e = i; e < m * m; e += W) U[(e % m) * W + e / m] = blk[e];      // U(r, c) = B[r][c], coalesced read
    __syncthreads();
    const bool row = i < m;
    // |B|_F^2 and the wave's loop bound
    T fro2 = T(0);
    if (row) for (int j = 0; j < m; ++j) fro2 += U[j * W + i] * U[j * W + i];
    fro2 = group_sum<T, W>(fro2);
    int mw = m;
    for (int off = 32; off >= W; off >>= 1) mw = max(mw, __shfl_xor(mw, off, 64));
    const T tol = dpinv::pair_tolerance<T>(m > 0 ? m : 1), floor2 = dpinv::noise_floor2<T>(m, fro2);
    bool live = m > 1;                 // this group still rotates
    int sweeps = 0;
    while (__any(live) && sweeps < sweep_cap) {
        int rotated = 0;
        for (int j = 0; j + 1 < mw; ++j) {
            for (int k = j + 1; k < mw; ++k) {
                const bool mine = live && k < m;
                T uj = T(0), uk = T(0);
                if (mine && row) { uj = U[j * W + i]; uk = U[k * W + i]; }
                const T aa = group_sum<T, W>(uj * uj), bb = group_sum<T, W>(uk * uk), dd = group_sum<T, W>(uj * uk);
                if (mine) {
                    const dpinv::Rotation<T> r = dpinv::rotation(aa, bb, dd, tol, floor2);
                    if (r.on) {
                        ++rotated;
                        if (row) {
                            dpinv::rotate(uj, uk, r.c, r.s);
                            U[j * W + i] = uj; U[k * W + i] = uk;
                            T vj = V[j * W + i], vk = V[k * W + i];
                            dpinv::rotate(vj, vk, r.c, r.s);
                            V[j * W + i] = vj; V[k * W + i] = vk;
                        }
                    }
                }
            }
        }
        ++sweeps;
        if (live && rotated == 0) live = false;          // a sweep without a rotation: converged (counted: it is the check)
        if (live && i == 0 && sweeps >= sweep_cap) atomicAdd(&cw[CW_NOCONV], 1ull);
    }
    const int my_sweeps = m > 1 ? sweeps : 0;              // (the slowest group of the wave; a bound for the others)
    // singular values: lane j keeps sigma_j
    T sig = T(0), smax = T(0);
    for (int j = 0; j < mw; ++j) {
        T u = T(0);
        if (row && j < m) u = U[j * W + i];
        const T s = sqrt(group_sum<T, W>(u * u));
        if (j == i) sig = s;
        smax = fmax(smax, s);
    }
    const bool keep = row && dpinv::kept(sig, smax, rank_tol);
    const T inv = keep ? T(1) / sig : T(0);
    int nkept = keep ? 1 : 0;
    for (int off = W / 2; off > 0; off >>= 1) nkept += __shfl_xor(nkept, off, W);
    // u_j / sigma_j and v_j / sigma_j (zero for a dropped j)
    for (int j = 0; j < mw; ++j) {
        const T w = __shfl(inv, j, W);
        if (row && j < m) {
            U[j * W + i] = U[j * W + i] * w;
            V[j * W + i] = V[j * W + i] * w;
        }
    }
    __syncthreads();
    if (row) {
        for (int c = 0; c < m; ++c) {
            T acc = T(0);
            for (int j = 0; j < m; ++j) acc += V[j * W + i] * U[j * W + c];
            blk[i * m + c] = acc;
        }
        if (i == 0) {
            if (nkept < m) atomicAdd(&cw[CW_TRUNC], 1ull);
            atomicMax(&cw[CW_SWEEPS], (unsigned long long)my_sweeps);
        }
    }
}

template <typename T, int W>
int launch_class(bool invert, const int *list, int count, const int *Sp, const int *Sj, const int *Tp, const pamg_matrix_s *A, T *Tx,
                 double rank_tol, unsigned long long *cw, hipStream_t s)
{
    if (count == 0) return PAMG_OK;
    if (!invert) {
        const int per = 256 / W;
        hipLaunchKernelGGL((schwarz_extract_kernel<T, W>), dim3((unsigned)((count + per - 1) / per)), dim3(256), 0, s, list, count, Sp, Sj, Tp,
                           (int)A->nrows, (const int *)A->d_Ap, (const int *)A->d_Aj, (const T *)A->d_Ax, Tx, cw);
    } else {
        const int per = 64 / W;
        hipLaunchKernelGGL((schwarz_pinv_kernel<T, W>), dim3((unsigned)((count + per - 1) / per)), dim3(64), 0, s, list, count, Sp, Tp, Tx,
                           (T)rank_tol, dpinv::SWEEP_CAP, cw);
    }
    return (int)hipGetLastError();
}

template <typename T>
int launch_all(bool invert, const int *lists, int nsub, const unsigned long long *h_cw, const int *Sp, const int *Sj, const int *Tp,
               const pamg_matrix_s *A, T *Tx, double rank_tol, unsigned long long *cw, hipStream_t s)
{
    const int *l = lists;
    PAMG_TRY((launch_class<T, 8>(invert, l, (int)h_cw[CW_COUNT0 + 0], Sp, Sj, Tp, A, Tx, rank_tol, cw, s)));
    PAMG_TRY((launch_class<T, 16>(invert, l + (size_t)nsub, (int)h_cw[CW_COUNT0 + 1], Sp, Sj, Tp, A, Tx, rank_tol, cw, s)));
    PAMG_TRY((launch_class<T, 32>(invert, l + 2 * (size_t)nsub, (int)h_cw[CW_COUNT0 + 2], Sp, Sj, Tp, A, Tx, rank_tol, cw, s)));
    PAMG_TRY((launch_class<T, 64>(invert, l + 3 * (size_t)nsub, (int)h_cw[CW_COUNT0 + 3], Sp, Sj, Tp, A, Tx, rank_tol, cw, s)));
    return PAMG_OK;
}

}  // namespace

namespace pamg {

// tp_given: d_Tp is the caller's block pointer (amg_core's calling convention; the caller has checked it against Tx) and is
// left as it is; otherwise it is written here.
int schwarz_blocks_device(int dtype, pamg_matrix_s *A, int nsub, const int *d_Sp, const int *d_Sj, int *d_Tp, void *d_Tx,
                          int64_t Tx_capacity, double rank_tol, int invert, bool tp_given, hipStream_t s, int64_t info[4])
{
    if ((dtype != PAMG_F64 && dtype != PAMG_F32) || !A || nsub < 0 || !d_Sp || !d_Tp || Tx_capacity < 0 || !(rank_tol >= 0.0)) return PAMG_E_ARG;
    if (A->dtype != dtype) return PAMG_E_ARG;
    if (!A->d_Ap || !A->d_Aj || !A->d_Ax) return PAMG_E_UNSUPPORTED;
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    Bufs d;
    long long *tp64;
    int *lists;
    unsigned long long *cw;
    PAMG_TRY(d.get(&tp64, (size_t)nsub + 1)); PAMG_TRY(d.get(&lists, (size_t)dpinv::NCLASS * nsub)); PAMG_TRY(d.get(&cw, (size_t)CW_WORDS));
    unsigned long long h_cw[CW_WORDS];
    hipLaunchKernelGGL(schwarz_plan_kernel, dim3(1), dim3(PLAN_T), 0, s, nsub, d_Sp, tp64, lists, cw);
    PAMG_HIP(hipGetLastError());
    PAMG_HIP(hipMemcpyAsync(h_cw, cw, sizeof(h_cw), hipMemcpyDeviceToHost, s));
    PAMG_HIP(hipStreamSynchronize(s));
    if (info) { info[0] = (int64_t)h_cw[CW_TOTAL]; info[1] = (int64_t)h_cw[CW_MAXM]; }
    if (h_cw[CW_BAD]) return PAMG_E_ARG;
    if (h_cw[CW_MAXM] > (unsigned long long)dpinv::MAX_M) return PAMG_E_UNSUPPORTED;
    if (h_cw[CW_TOTAL] > (unsigned long long)INT32_MAX) return PAMG_E_UNSUPPORTED;      // the reference's Tp is int32
    const size_t ts = tsize(dtype);
    if (!tp_given) {
        if ((int64_t)h_cw[CW_TOTAL] > Tx_capacity) return PAMG_E_ARG;
        hipLaunchKernelGGL(schwarz_tp_narrow_kernel, dim3((unsigned)(nsub / 256 + 1)), dim3(256), 0, s, nsub + 1, (const long long *)tp64, d_Tp);
        PAMG_HIP(hipGetLastError());
        if (h_cw[CW_TOTAL]) PAMG_HIP(hipMemsetAsync(d_Tx, 0, ts * (size_t)h_cw[CW_TOTAL], s));
    } else if (Tx_capacity) {
        PAMG_HIP(hipMemsetAsync(d_Tx, 0, ts * (size_t)Tx_capacity, s));              // (the caller passes Tp[nsub]: what the reference clears)
    }
    if (h_cw[CW_TOTAL] == 0) return PAMG_OK;
    if (!d_Sj || !d_Tx) return PAMG_E_ARG;
    for (int pass = 0; pass < (invert ? 2 : 1); ++pass) {
        if (dtype == PAMG_F64) PAMG_TRY(launch_all<double>(pass == 1, lists, nsub, h_cw, d_Sp, d_Sj, d_Tp, A, (double *)d_Tx, rank_tol, cw, s));
        else PAMG_TRY(launch_all<float>(pass == 1, lists, nsub, h_cw, d_Sp, d_Sj, d_Tp, A, (float *)d_Tx, rank_tol, cw, s));
    }
    PAMG_HIP(hipMemcpyAsync(h_cw, cw, sizeof(h_cw), hipMemcpyDeviceToHost, s));
    PAMG_HIP(hipStreamSynchronize(s));
    if (info) { info[2] = (int64_t)h_cw[CW_SWEEPS]; info[3] = (int64_t)h_cw[CW_TRUNC]; }
    if (h_cw[CW_BAD]) return PAMG_E_ARG;
    if (h_cw[CW_NOCONV]) return PAMG_E_NOCONV;
    return PAMG_OK;
}

}  // namespace pamg

extern "C" {

int pamg_dev_schwarz_blocks(int dtype, pamg_matrix_t A, int nsub, const int32_t *d_Sp, const int32_t *d_Sj, int32_t *d_Tp, void *d_Tx,
                            int64_t Tx_capacity, double rank_tol, int invert, pamg_stream_t s, int64_t info[4])
{
    return schwarz_blocks_device(dtype, A, nsub, d_Sp, d_Sj, d_Tp, d_Tx, Tx_capacity, rank_tol, invert, false, (hipStream_t)s, info);
}

int pamg_schwarz_blocks(int dtype, pamg_matrix_t A, int nsub, const int32_t *Sp, const int32_t *Sj, int32_t *Tp, void *Tx,
                        int64_t Tx_capacity, double rank_tol, int invert, int64_t info[4])
{
    if (!A || nsub < 0 || !Sp || !Tp || Tx_capacity < 0 || (dtype != PAMG_F64 && dtype != PAMG_F32)) return PAMG_E_ARG;
    if (Sp[0] < 0) return PAMG_E_ARG;
    for (int d = 0; d < nsub; ++d) if (Sp[d + 1] < Sp[d]) return PAMG_E_ARG;
    const size_t nS = (size_t)Sp[nsub];
    if (nS && !Sj) return PAMG_E_ARG;
    if (Tx_capacity && !Tx) return PAMG_E_ARG;
    Bufs d;
    int *dSp, *dSj, *dTp;
    char *dTx;                                  // Tx_capacity values of dtype
    const size_t ts = tsize(dtype);
    PAMG_TRY(d.put(&dSp, Sp, (size_t)nsub + 1)); PAMG_TRY(d.put(&dSj, Sj, nS));
    PAMG_TRY(d.get(&dTp, (size_t)nsub + 1)); PAMG_TRY(d.get(&dTx, ts * (size_t)Tx_capacity));
    int64_t loc[4];
    int64_t *inf = info ? info : loc;
    PAMG_TRY(schwarz_blocks_device(dtype, A, nsub, dSp, dSj, dTp, dTx, Tx_capacity, rank_tol, invert, false, nullptr, inf));
    PAMG_TRY(Bufs::fetch(Tp, dTp, (size_t)nsub + 1));
    return Bufs::fetch((char *)Tx, dTx, ts * (size_t)inf[0]);
}

}  // extern "C"
