// pamg_wave.h -- what the persistent sweeps share on the device: the sentinel of the hand-off buffers, the sum across the lanes of a row,
// the one-XCD claim, the ticket draw and the profile stamp.  Plain C++ and compiler builtins; included by every sweep file and by
// pamg_kernels.h, so each of these exists once.
#pragma once
#include "pamg_common.h"

namespace pamg {

// Sentinel bit patterns of the hand-off buffer xs (a quiet NaN with a payload no arithmetic
// produces): xs[j] == sentinel  <=>  row j has not published its new value in this sweep yet.
template <typename T> struct Sentinel;
template <> struct Sentinel<double> {
    using bits_t = unsigned long long;
    static constexpr bits_t value = 0x7FF8DEADBEEF5A5Aull;
    static __device__ __forceinline__ bits_t bits(double v) { return (bits_t)__double_as_longlong(v); }
    static __device__ __forceinline__ bool missing(double v) { return bits(v) == value; }
};
template <> struct Sentinel<float> {
    using bits_t = unsigned int;
    static constexpr bits_t value = 0x7FC5BEEFu;
    static __device__ __forceinline__ bits_t bits(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ bool missing(float v) { return bits(v) == value; }
};

template <typename T>
__global__ __launch_bounds__(BLK) void fill_sentinel_kernel(T *xs, int64_t n)
{
    using B = typename Sentinel<T>::bits_t;
    B *p = reinterpret_cast<B *>(xs);
    for (int64_t i = (int64_t)blockIdx.x * BLK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLK) p[i] = Sentinel<T>::value;
}

// the XCD this wave runs on: HW_REG_XCC_ID[3:0]
__device__ __forceinline__ unsigned xcc_id() { return __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xF; }

// ---- sum over the L lanes that share a row; every lane ends up with the total (bit for bit the same total: an XOR butterfly
//      adds the same two values in both lanes of a pair at every step)
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);       // (no `old` operand: every lane has a source, the compiler needs no copy)
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// lane ^ 16 and lane ^ 32 without the LDS path (ds_swizzle / ds_bpermute cost ~100 cycles of latency each and a wait per value):
// v_permlane16_swap / v_permlane32_swap (CDNA4) exchange the odd 16-lane rows (the upper half) of one copy with the even rows (the lower
// half) of the other; afterwards one copy holds the even-row (lower-half) values everywhere, the other the odd-row (upper-half) ones, and
// their sum is the butterfly step
template <bool HALF>
__device__ __forceinline__ double swap_sum(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    if constexpr (HALF) {
        const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        return __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
    } else {
        const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        return __hiloint2double(b[0], a[0]) + __hiloint2double(b[1], a[1]);
    }
}
template <bool HALF>
__device__ __forceinline__ float swap_sum(float v)
{
    const int w = __float_as_int(v);
    if constexpr (HALF) {
        const auto a = __builtin_amdgcn_permlane32_swap(w, w, false, false);
        return __int_as_float(a[0]) + __int_as_float(a[1]);
    } else {
        const auto a = __builtin_amdgcn_permlane16_swap(w, w, false, false);
        return __int_as_float(a[0]) + __int_as_float(a[1]);
    }
}

template <int L, typename T>
__device__ __forceinline__ T seg_allreduce(T v)
{
    static_assert(L >= 4 && L <= 64 && (L & (L - 1)) == 0, "rows share 4 .. 64 lanes");
    v = v + dpp_mov<0xB1>(v);                                   // quad_perm [1,0,3,2]: lane ^ 1
    v = v + dpp_mov<0x4E>(v);                                   // quad_perm [2,3,0,1]: lane ^ 2
    if constexpr (L >= 8) v = v + dpp_mov<0x141>(v);            // row_half_mirror: the other quad of the 8
    if constexpr (L >= 16) v = v + dpp_mov<0x140>(v);           // row_mirror: the other half of the 16
    if constexpr (L >= 32) v = swap_sum<false>(v);              // lane ^ 16
    if constexpr (L >= 64) v = swap_sum<true>(v);               // lane ^ 32
    return v;
}

// ---- the one-XCD forms: the first workgroup to arrive claims its XCD as the home (*slot = XCD + 1, zero before the launch), workgroups
// elsewhere leave.  home_xcd_vote: the calling thread's answer for its workgroup
__device__ __forceinline__ bool home_xcd_vote(unsigned *slot)
{
    const unsigned me = xcc_id() + 1u;
    unsigned home = 0u;
    __hip_atomic_compare_exchange_strong(slot, &home, me, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return home == 0u || home == me;                            // home holds the previous value
}
// every thread of the workgroup calls it (a barrier inside) and learns whether the workgroup stays
__device__ __forceinline__ bool claim_home_xcd(unsigned *slot)
{
    __shared__ int sh_home;
    if (threadIdx.x == 0) sh_home = home_xcd_vote(slot) ? 1 : 0;
    __syncthreads();
    return sh_home != 0;
}

// ---- tickets: lane 0 draws into its tk, the wave reads lane 0's register.  Two steps, so that a wave can draw its next ticket before it
// starts to wait for the current group and read the number afterwards (the atomic returns long before the group's operands do).
// wanted: a wave-uniform condition of the caller's (no ticket beyond the last group)
__device__ __forceinline__ void draw_ticket(unsigned *counter, unsigned &tk, const bool wanted = true)
{
    if (wanted && (threadIdx.x & 63) == 0) tk = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ticket_number(unsigned tk) { return (int)__builtin_amdgcn_readfirstlane(tk); }

// ---- the profile record of a group (PAMG_TUNE_GS_PROF): started, last operand seen, published, XCD | workgroup << 4.  One lane writes it
__device__ __forceinline__ void profile_stamp(long long *o, long long t0, long long t1)
{
    o[0] = t0; o[1] = t1; o[2] = wall_clock64();
    o[3] = (long long)(xcc_id() | (blockIdx.x << 4));
}

}  // namespace pamg
