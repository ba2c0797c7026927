// pamg_host_call.h -- what every Layer-1 setup call (host arrays in, host arrays out) does around its kernels: the device buffers of one
// call, the device test, the pattern check and the launch grid.  Host code over the HIP runtime: the arithmetic headers that the host
// replays include (pamg_classical.h, pamg_air.h, pamg_evolution.h, ...) do not depend on it.
#pragma once

#include "pamg_common.h"

namespace pamg {

// device buffers of one call, released when it returns
struct Bufs {
    std::vector<void *> p;
    ~Bufs() { for (void *q : p) hipFree(q); }
    template <typename T>
    int get(T **out, size_t n)
    {
        void *q = nullptr;
        PAMG_HIP(hipMalloc(&q, std::max<size_t>(sizeof(T) * n, 256)));
        p.push_back(q);
        *out = (T *)q;
        return PAMG_OK;
    }
    template <typename T>
    int put(T **out, const T *host, size_t n)
    {
        PAMG_TRY(get(out, n));
        if (n) PAMG_HIP(hipMemcpy(*out, host, sizeof(T) * n, hipMemcpyHostToDevice));
        return PAMG_OK;
    }
    // n values back to the host (a blocking copy: it also waits for the kernels launched before it)
    template <typename T>
    static int fetch(T *host, const T *dev, size_t n)
    {
        if (n) PAMG_HIP(hipMemcpy(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost));
        return PAMG_OK;
    }
};

inline int have_device()
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return PAMG_E_NODEVICE;
    return PAMG_OK;
}

// a compressed pattern of n rows (or columns) whose indices lie in [0, ncol): sizes, the pointer starting at 0 and monotone, indices in
// range; with_values: also room for Ap[n] values in Ax.  (A negative size fails the comparison with Ap[n] >= 0.)
inline int check_pattern(int n, int ncol, const int *Ap, int Ap_size, const int *Aj, int Aj_size, int64_t *nnz_out, bool with_values = false,
                         const double *Ax = nullptr, int Ax_size = 0)
{
    if (n < 0 || !Ap || Ap_size < n + 1 || Ap[0] != 0) return PAMG_E_ARG;
    for (int i = 0; i < n; ++i) if (Ap[i + 1] < Ap[i]) return PAMG_E_ARG;
    const int64_t nnz = Ap[n];
    if (nnz > Aj_size || (nnz && !Aj)) return PAMG_E_ARG;
    if (with_values && (nnz > Ax_size || (nnz && !Ax))) return PAMG_E_ARG;
    for (int64_t p = 0; p < nnz; ++p) if (Aj[p] < 0 || Aj[p] >= ncol) return PAMG_E_ARG;
    *nnz_out = nnz;
    return PAMG_OK;
}

// The transposed off-diagonal pattern of the n-row device pattern dSp / dSj with nnz entries (pamg_classical.hip): ddeg [n] receives the
// in-degrees, dTp [n + 1] / dTj [nnz] the pattern, dcur [n] and dflag [1] are scratch.  Built with atomics: the order inside a transposed
// row is not reproducible.
int device_transposed_pattern(int n, int64_t nnz, const int *dSp, const int *dSj, int *ddeg, int *dTp, int *dTj, int *dcur, unsigned *dflag);

// What the scalar and the block AIR entry points share (pamg_air.hip).  air_check_cf: the C-point list and the splitting of an n-row
// pattern.  air_neighbourhood_counts: cnt[r] = the size N of the neighbourhood of Cpts[r] (pamg_air.h) -- the device's counts, and the
// host threads for what did not fit its 64-entry slots; dCp / dCj / dCpts / dsp are the device copies of the host arrays beside them.
int air_check_cf(int n, const int *Cpts, int Cpts_size, const int *splitting, int splitting_size);
int air_neighbourhood_counts(int n, int nc, const int *Cp, const int *Cj, const int *Cpts, const int *splitting, int distance, const int *dCp,
                             const int *dCj, const int *dCpts, const int *dsp, Bufs &d, std::vector<int> &cnt);

// workgroups of a grid-stride launch over n items, per_block of them per workgroup and pass
inline int launch_grid(int64_t n, int per_block, int cap) { return (int)std::min<int64_t>(cap, std::max<int64_t>(1, (n + per_block - 1) / per_block)); }

}  // namespace pamg
