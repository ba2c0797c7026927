// pamg_krylov.hip -- fused vector work of the device-resident BiCGStab / CR / steepest-descent / minimal-residual
// accelerators (pamg_solver.hip: bicgstab_core, cr_core, sd_core, mr_core).
//
// One launch per step of the iteration instead of one per axpy and per inner product: each kernel does an update and
// takes the inner products the next step needs in the same pass.  Step sizes are formed on the device from reduced
// slots (every workgroup computes the same double from the same bits), so nothing but the per-iteration residual norm
// crosses PCIe.  Inner products accumulate in double, one partial per workgroup over a grid fixed by n, summed by one
// workgroup per product in index order (kr_reduce_kernel): the same bits on every run, no atomics.
//
// Elementwise arithmetic rounds the way the reference's NumPy expressions do: every product is its own temporary
// (the build passes -ffp-contract=off) and sums go left to right, e.g. x + a*u + b*v is (x + a*u) + b*v.
#include "pamg_kernels.h"

namespace pamg {

namespace {

constexpr int KR_GRID_CAP = 2048;     // workgroups of the fused kernels (KR_PARTIALS / 3)

int kr_grid(int64_t n) { return (int)std::min<int64_t>(KR_GRID_CAP, std::max<int64_t>(1, (n + BLK - 1) / BLK)); }

#define KR_LOOP(i, n) for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < (n); i += (int64_t)gridDim.x * BLK)

// the K workgroup sums of acc[] -> part[k * gridDim.x + blockIdx.x]
template <int K>
__device__ __forceinline__ void store_partials(const double (&acc)[K], double *part)
{
    __shared__ double sm[K][BLK / 64];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double t = block_sum(acc[k], sm[k]);
        if (threadIdx.x == 0) part[(size_t)k * gridDim.x + blockIdx.x] = t;
    }
}

// K inner products (a_k, b_k) in one pass
template <typename T, int K>
__global__ __launch_bounds__(BLK) void kr_dots_kernel(int64_t n, const T *a0, const T *b0, const T *a1, const T *b1, const T *a2,
                                                      const T *b2, double *part)
{
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    KR_LOOP(i, n) {
        acc[0] += (double)a0[i] * (double)b0[i];
        if constexpr (K > 1) acc[1] += (double)a1[i] * (double)b1[i];
        if constexpr (K > 2) acc[2] += (double)a2[i] * (double)b2[i];
    }
    store_partials<K>(acc, part);
}

// workgroup k sums the G partials of product k into *out_k (reduce_final_kernel's order)
static __global__ __launch_bounds__(BLK) void kr_reduce_kernel(const double *part, int G, double *o0, double *o1, double *o2)
{
    __shared__ double sm[BLK / 64];
    const int k = (int)blockIdx.x;
    const double *p = part + (size_t)k * G;
    double acc = 0.0;
    for (int i = threadIdx.x; i < G; i += BLK) acc += p[i];
    const double tot = block_sum(acc, sm);
    if (threadIdx.x == 0) (k == 0 ? o0 : k == 1 ? o1 : o2)[0] = tot;
}

// ---- BiCGStab (krylov/_bicgstab.py:139-170).  Mp / Ms arrive in the fine level's iterate xc (the cycle's output), s is written
// into the fine level's right-hand side bc (the next cycle's operand), xc is cleared behind its last reader (the next cycle starts
// from zero).
// alpha = rr / (r*, AMp);  x = x + alpha Mp;  s = r - alpha AMp
template <typename T>
__global__ __launch_bounds__(BLK) void bicg_alpha_kernel(int64_t n, const double *rr, const double *d, double *alpha_out, T *x, T *xc,
                                                         const T *r, const T *AMp, T *bc)
{
    const double alpha = rr[0] / d[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) alpha_out[0] = alpha;
    const T a = (T)alpha;
    KR_LOOP(i, n) {
        const T am = a * AMp[i];
        bc[i] = r[i] - am;
        const T xm = a * xc[i];
        x[i] = x[i] + xm;
        xc[i] = T(0);
    }
}

// omega = (AMs, s) / (AMs, AMs);  x = x + omega Ms;  r = s - omega AMs;  partials of (r*, r) and (r, r)
template <typename T>
__global__ __launch_bounds__(BLK) void bicg_omega_kernel(int64_t n, const double *num, const double *den, double *omega_out, T *x,
                                                         const T *xc, const T *bc, const T *AMs, T *r, const T *rstar, double *part)
{
    const double omega = num[0] / den[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) omega_out[0] = omega;
    const T w = (T)omega;
    double acc[2] = {0.0, 0.0};
    KR_LOOP(i, n) {
        const T xm = w * xc[i];
        x[i] = x[i] + xm;
        const T am = w * AMs[i];
        const T ri = bc[i] - am;
        r[i] = ri;
        acc[0] += (double)rstar[i] * (double)ri;
        acc[1] += (double)ri * (double)ri;
    }
    store_partials<2>(acc, part);
}

// beta = (rr_new / rr_old) (alpha / omega);  p = r + beta (p - omega AMp);  the next cycle's operand bc = p, xc = 0
template <typename T>
__global__ __launch_bounds__(BLK) void bicg_dir_kernel(int64_t n, const double *rr_new, const double *rr_old, const double *alpha,
                                                       const double *omega, const T *r, T *p, const T *AMp, T *bc, T *xc)
{
    const double beta = (rr_new[0] / rr_old[0]) * (alpha[0] / omega[0]);
    const T bt = (T)beta, w = (T)omega[0];
    KR_LOOP(i, n) {
        const T am = w * AMp[i];
        const T d = p[i] - am;
        const T bd = bt * d;
        const T pi = r[i] + bd;
        p[i] = pi;
        bc[i] = pi;
        xc[i] = T(0);
    }
}

// ---- CR (krylov/_cr.py:144-167).  r lives in the fine level's right-hand side, z = M r in its iterate.
// alpha = rAz / (Ap, Ap);  x += alpha p;  [r -= alpha Ap];  xc = 0 (z has been used)
template <typename T>
__global__ __launch_bounds__(BLK) void cr_update_kernel(int64_t n, const double *rAz, const double *ApAp, T *x, const T *p, T *r,
                                                        const T *Ap, int update_r, T *xc)
{
    const T a = (T)(rAz[0] / ApAp[0]);
    KR_LOOP(i, n) {
        const T t = a * p[i];
        x[i] = x[i] + t;
        if (update_r) {
            const T u = a * Ap[i];
            r[i] = r[i] - u;
        }
        xc[i] = T(0);
    }
}

// beta = rAz_new / rAz_old;  p *= beta; p += z;  Ap *= beta; Ap += Az;  partial of (Ap, Ap)
template <typename T>
__global__ __launch_bounds__(BLK) void cr_dir_kernel(int64_t n, const double *rAz_new, const double *rAz_old, T *p, const T *z, T *Ap,
                                                     const T *Az, double *part)
{
    const T bt = (T)(rAz_new[0] / rAz_old[0]);
    double acc[1] = {0.0};
    KR_LOOP(i, n) {
        const T tp = p[i] * bt;
        p[i] = tp + z[i];
        const T ta = Ap[i] * bt;
        const T api = ta + Az[i];
        Ap[i] = api;
        acc[0] += (double)api * (double)api;
    }
    store_partials<1>(acc, part);
}

// ---- steepest descent (krylov/_steepest_descent.py:144-160) and minimal residual (krylov/_minimal_residual.py:131-149).
// gate < 0 (curvature of A, resp. of M A): the reference returns before it touches x -- the write is skipped on the device and the
// host reports -1 after this iteration's read-back.
// SD:  alpha = rz / zAz;  x = x + alpha z;  [r = r - alpha q];  xc = 0 (z = xc has been used)
template <typename T>
__global__ __launch_bounds__(BLK) void sd_update_kernel(int64_t n, const double *rz, const double *zAz, T *x, T *xc, T *r, const T *q,
                                                        int update_r)
{
    const double g = zAz[0];
    const bool write_x = !(g < 0.0);
    const T a = (T)(rz[0] / g);
    KR_LOOP(i, n) {
        const T t = a * xc[i];
        if (write_x) x[i] = x[i] + t;
        if (update_r) {
            const T u = a * q[i];
            r[i] = r[i] - u;
        }
        xc[i] = T(0);
    }
}

// MR:  alpha = pz / pp;  x = x + alpha z;  [z = z - alpha p, partial of (z, z)];  xc = 0 (p = xc has been used)
template <typename T>
__global__ __launch_bounds__(BLK) void mr_update_kernel(int64_t n, const double *pz, const double *pp, T *x, T *z, T *xc, int update_z,
                                                        double *part)
{
    const double g = pz[0];
    const bool write_x = !(g < 0.0);
    const T a = (T)(g / pp[0]);
    double acc[1] = {0.0};
    KR_LOOP(i, n) {
        const T zi = z[i];
        const T t = a * zi;
        if (write_x) x[i] = x[i] + t;
        if (update_z) {
            const T u = a * xc[i];
            const T zn = zi - u;
            z[i] = zn;
            acc[0] += (double)zn * (double)zn;
        }
        xc[i] = T(0);
    }
    store_partials<1>(acc, part);
}

// dst = xc; xc = 0; partial of (dst, dst): the cycle's result taken out of the fine level's iterate
template <typename T>
__global__ __launch_bounds__(BLK) void kr_take_kernel(int64_t n, T *xc, T *dst, double *part)
{
    double acc[1] = {0.0};
    KR_LOOP(i, n) {
        const T v = xc[i];
        dst[i] = v;
        xc[i] = T(0);
        acc[0] += (double)v * (double)v;
    }
    store_partials<1>(acc, part);
}

#undef KR_LOOP

template <typename T> T *tp(void *p) { return reinterpret_cast<T *>(p); }
template <typename T> const T *tp(const void *p) { return reinterpret_cast<const T *>(p); }

}  // namespace

int kr_reduce(int64_t n, const double *part, int k, double *o0, double *o1, double *o2, hipStream_t s)
{
    hipLaunchKernelGGL(kr_reduce_kernel, dim3(k), dim3(BLK), 0, s, part, kr_grid(n), o0, o1, o2);
    return (int)hipGetLastError();
}

int kr_dots(int dt, int64_t n, int k, const void *a0, const void *b0, const void *a1, const void *b1, const void *a2, const void *b2,
            double *part, hipStream_t s)
{
    const int G = kr_grid(n);
    auto go = [&](auto tag) {
        using T = decltype(tag);
        if (k == 1) hipLaunchKernelGGL((kr_dots_kernel<T, 1>), dim3(G), dim3(BLK), 0, s, n, tp<T>(a0), tp<T>(b0), tp<T>(a1), tp<T>(b1), tp<T>(a2), tp<T>(b2), part);
        else if (k == 2) hipLaunchKernelGGL((kr_dots_kernel<T, 2>), dim3(G), dim3(BLK), 0, s, n, tp<T>(a0), tp<T>(b0), tp<T>(a1), tp<T>(b1), tp<T>(a2), tp<T>(b2), part);
        else hipLaunchKernelGGL((kr_dots_kernel<T, 3>), dim3(G), dim3(BLK), 0, s, n, tp<T>(a0), tp<T>(b0), tp<T>(a1), tp<T>(b1), tp<T>(a2), tp<T>(b2), part);
    };
    if (k < 1 || k > 3) return PAMG_E_ARG;
    if (dt == PAMG_F64) go(double()); else go(float());
    return (int)hipGetLastError();
}

int bicg_alpha(int dt, int64_t n, const double *rr, const double *d, double *alpha, void *x, void *xc, const void *r, const void *AMp,
               void *bc, hipStream_t s)
{
    const int G = kr_grid(n);
    if (dt == PAMG_F64) hipLaunchKernelGGL(bicg_alpha_kernel<double>, dim3(G), dim3(BLK), 0, s, n, rr, d, alpha, tp<double>(x), tp<double>(xc), tp<double>(r), tp<double>(AMp), tp<double>(bc));
    else hipLaunchKernelGGL(bicg_alpha_kernel<float>, dim3(G), dim3(BLK), 0, s, n, rr, d, alpha, tp<float>(x), tp<float>(xc), tp<float>(r), tp<float>(AMp), tp<float>(bc));
    return (int)hipGetLastError();
}

int bicg_omega(int dt, int64_t n, const double *num, const double *den, double *omega, void *x, const void *xc, const void *bc,
               const void *AMs, void *r, const void *rstar, double *part, hipStream_t s)
{
    const int G = kr_grid(n);
    if (dt == PAMG_F64) hipLaunchKernelGGL(bicg_omega_kernel<double>, dim3(G), dim3(BLK), 0, s, n, num, den, omega, tp<double>(x), tp<double>(xc), tp<double>(bc), tp<double>(AMs), tp<double>(r), tp<double>(rstar), part);
    else hipLaunchKernelGGL(bicg_omega_kernel<float>, dim3(G), dim3(BLK), 0, s, n, num, den, omega, tp<float>(x), tp<float>(xc), tp<float>(bc), tp<float>(AMs), tp<float>(r), tp<float>(rstar), part);
    return (int)hipGetLastError();
}

int bicg_dir(int dt, int64_t n, const double *rr_new, const double *rr_old, const double *alpha, const double *omega, const void *r,
             void *p, const void *AMp, void *bc, void *xc, hipStream_t s)
{
    const int G = kr_grid(n);
    if (dt == PAMG_F64) hipLaunchKernelGGL(bicg_dir_kernel<double>, dim3(G), dim3(BLK), 0, s, n, rr_new, rr_old, alpha, omega, tp<double>(r), tp<double>(p), tp<double>(AMp), tp<double>(bc), tp<double>(xc));
    else hipLaunchKernelGGL(bicg_dir_kernel<float>, dim3(G), dim3(BLK), 0, s, n, rr_new, rr_old, alpha, omega, tp<float>(r), tp<float>(p), tp<float>(AMp), tp<float>(bc), tp<float>(xc));
    return (int)hipGetLastError();
}

int cr_update(int dt, int64_t n, const double *rAz, const double *ApAp, void *x, const void *p, void *r, const void *Ap, bool update_r,
              void *xc, hipStream_t s)
{
    const int G = kr_grid(n);
    if (dt == PAMG_F64) hipLaunchKernelGGL(cr_update_kernel<double>, dim3(G), dim3(BLK), 0, s, n, rAz, ApAp, tp<double>(x), tp<double>(p), tp<double>(r), tp<double>(Ap), update_r ? 1 : 0, tp<double>(xc));
    else hipLaunchKernelGGL(cr_update_kernel<float>, dim3(G), dim3(BLK), 0, s, n, rAz, ApAp, tp<float>(x), tp<float>(p), tp<float>(r), tp<float>(Ap), update_r ? 1 : 0, tp<float>(xc));
    return (int)hipGetLastError();
}

int cr_dir(int dt, int64_t n, const double *rAz_new, const double *rAz_old, void *p, const void *z, void *Ap, const void *Az, double *part,
           hipStream_t s)
{
    const int G = kr_grid(n);
    if (dt == PAMG_F64) hipLaunchKernelGGL(cr_dir_kernel<double>, dim3(G), dim3(BLK), 0, s, n, rAz_new, rAz_old, tp<double>(p), tp<double>(z), tp<double>(Ap), tp<double>(Az), part);
    else hipLaunchKernelGGL(cr_dir_kernel<float>, dim3(G), dim3(BLK), 0, s, n, rAz_new, rAz_old, tp<float>(p), tp<float>(z), tp<float>(Ap), tp<float>(Az), part);
    return (int)hipGetLastError();
}

int sd_update(int dt, int64_t n, const double *rz, const double *zAz, void *x, void *xc, void *r, const void *q, bool update_r, hipStream_t s)
{
    const int G = kr_grid(n);
    if (dt == PAMG_F64) hipLaunchKernelGGL(sd_update_kernel<double>, dim3(G), dim3(BLK), 0, s, n, rz, zAz, tp<double>(x), tp<double>(xc), tp<double>(r), tp<double>(q), update_r ? 1 : 0);
    else hipLaunchKernelGGL(sd_update_kernel<float>, dim3(G), dim3(BLK), 0, s, n, rz, zAz, tp<float>(x), tp<float>(xc), tp<float>(r), tp<float>(q), update_r ? 1 : 0);
    return (int)hipGetLastError();
}

int mr_update(int dt, int64_t n, const double *pz, const double *pp, void *x, void *z, void *xc, bool update_z, double *part, hipStream_t s)
{
    const int G = kr_grid(n);
    if (dt == PAMG_F64) hipLaunchKernelGGL(mr_update_kernel<double>, dim3(G), dim3(BLK), 0, s, n, pz, pp, tp<double>(x), tp<double>(z), tp<double>(xc), update_z ? 1 : 0, part);
    else hipLaunchKernelGGL(mr_update_kernel<float>, dim3(G), dim3(BLK), 0, s, n, pz, pp, tp<float>(x), tp<float>(z), tp<float>(xc), update_z ? 1 : 0, part);
    return (int)hipGetLastError();
}

int kr_take(int dt, int64_t n, void *xc, void *dst, double *part, hipStream_t s)
{
    const int G = kr_grid(n);
    if (dt == PAMG_F64) hipLaunchKernelGGL(kr_take_kernel<double>, dim3(G), dim3(BLK), 0, s, n, tp<double>(xc), tp<double>(dst), part);
    else hipLaunchKernelGGL(kr_take_kernel<float>, dim3(G), dim3(BLK), 0, s, n, tp<float>(xc), tp<float>(dst), part);
    return (int)hipGetLastError();
}

}  // namespace pamg
