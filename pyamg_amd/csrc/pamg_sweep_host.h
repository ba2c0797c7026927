// pamg_sweep_host.h -- what the launchers of the persistent sweeps (pamg_lane.hip, pamg_blane.hip, pamg_kz.hip, pamg_line.hip) share on
// the host: the upload of a plan array, the co-residency cap, the profile buffer and the launch tail of the static / one-XCD forms.
#pragma once

#include "pamg_common.h"

namespace pamg {

// a plan array on the device; src = nullptr: allocation only (filled on the device).  total: where the schedule books its bytes
template <typename U>
int device_upload(U **dst, const void *src, size_t bytes, size_t *total)
{
    *dst = nullptr;
    const size_t alloc = std::max<size_t>(bytes, 256) + 256;   // slack: nothing reads past the end, but keep allocations non-empty
    PAMG_HIP(hipMalloc((void **)dst, alloc));
    if (bytes && src) PAMG_HIP(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
    if (total) *total += alloc;
    return PAMG_OK;
}

// workgroups per CU of kernel k that are certainly co-resident (every workgroup of a persistent sweep must be): the occupancy query
// minus one -- it can over-report by one per CU (MI355X_MICROARCH.md) --, at most max_per_cu.  Asked once per (cap, cap_kernel) pair
// and kernel, not per sweep.  A failed query counts as two workgroups: one is certain
inline int resident_cap(int &cap, const void *&cap_kernel, const void *k, int max_per_cu = 8)
{
    if (cap > 0 && cap_kernel == k) return cap;
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, BLK, 0) != hipSuccess) nb = 2;
    cap = std::max(1, std::min(nb - 1, max_per_cu));
    cap_kernel = k;
    return cap;
}

// the time stamps of a sweep (PAMG_TUNE_GS_PROF): four words per group, allocated on the first profiled sweep ...
inline int ensure_profile(long long **d_prof, int64_t ngroups)
{
    if (*d_prof) return PAMG_OK;
    PAMG_HIP(hipMalloc((void **)d_prof, (size_t)ngroups * 4 * sizeof(long long)));
    PAMG_HIP(hipMemset(*d_prof, 0, (size_t)ngroups * 4 * sizeof(long long)));
    return PAMG_OK;
}
// ... and read back: *n = groups, out filled when it has room for them
inline int read_profile(const long long *d_prof, int64_t ngroups, long long *out, int64_t cap, int64_t *n)
{
    *n = ngroups;
    if (out && cap >= *n) PAMG_HIP(hipMemcpy(out, d_prof, (size_t)*n * 4 * sizeof(long long), hipMemcpyDeviceToHost));
    return PAMG_OK;
}

// the launch of a persistent sweep of G workgroups.  One-XCD form: the ticket counter and the home word (ticket_words[0..1]) are zeroed and
// 8x the wanted grid is launched -- the workgroups off the home XCD leave at once --, the wanted grid being what one XCD's CUs hold
inline int launch_persistent(const void *k, void **args, int G, bool xcd, unsigned *ticket_words, int cus, int cap, int *last_grid, hipStream_t s)
{
    if (xcd) {
        PAMG_HIP(hipMemsetAsync(ticket_words, 0, 2 * sizeof(unsigned), s));
        G = 8 * std::max(1, std::min(G, (cus / 8) * cap));
    }
    *last_grid = G;
    PAMG_HIP(hipLaunchKernel(k, dim3(G), dim3(BLK), args, 0, s));
    return PAMG_OK;
}

}  // namespace pamg
