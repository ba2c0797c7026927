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

// ---- segmented inclusive scan over the 64 lanes of a wave, in registers (the cluster layout of the merged lane sweep: a lane serves one row, a
//      row owns consecutive lanes, the row's LAST lane ends up with the row's sum).  The additions and their association are those of the loop
//          for (d = 1; d < 64; d *= 2) s[i] = s[i] + (i - d >= seglo[i] ? s[i - d] : 0)          (all lanes at once)
//      -- only the way lane i gets lane i - d's value is chosen here: no ds_bpermute / ds_swizzle, no LDS, no wait per step.
// the value of lane - 16 (rows 1 .. 3 of 16 lanes; row 0 gets nothing it may use): v_permlane16_swap leaves the even rows' values in the odd rows
// of one copy (rows 1 and 3 are served) and the odd rows' values in the even rows of the other, whose lower half v_permlane32_swap hands to row 2
__device__ __forceinline__ double lane_shr16(double v, int lane)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);         // a[0]: rows (0, 0, 2, 2) of v, a[1]: rows (1, 1, 3, 3)
    const auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    const auto c = __builtin_amdgcn_permlane32_swap(a[1], a[1], false, false);     // c[0]: rows (1, 1, 1, 1)
    const auto d = __builtin_amdgcn_permlane32_swap(b[1], b[1], false, false);
    const bool row2 = (lane & 48) == 32;
    return __hiloint2double((int)(row2 ? d[0] : b[0]), (int)(row2 ? c[0] : a[0]));
}
// the value of lane - 32 (lanes 32 .. 63): the copy of v_permlane32_swap that holds the lower half everywhere
__device__ __forceinline__ double lane_shr32(double v)
{
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __hiloint2double((int)b[0], (int)a[0]);
}
// the value of lane - D, D = 2, 4, 8 (lanes >= D): DPP row_ror:D rotates inside the rows of 16 lanes -- the lanes whose value stays in the row send
// their own, the last D lanes of a row send what lane - 16 holds, which is what the first D lanes of the NEXT row are to receive
template <int D>
__device__ __forceinline__ double lane_shr(double v, int lane)
{
    static_assert(D == 2 || D == 4 || D == 8, "1: wave_shr, 16 / 32: the permlane swaps");
    const double below = lane_shr16(v, lane);
    return dpp_mov<0x120 + D>((lane & 15) < 16 - D ? v : below);
}

// the row boundaries from the lanes' keys (equal keys on consecutive lanes = one row; static plan data, so a sweep forms them BEFORE it waits for
// its operands): seg_scan_heads = the mask of the rows' first lanes (wave-uniform: a pair of scalar registers is all that has to live through the
// waits), seg_scan_first = the first lane of the calling lane's row
__device__ __forceinline__ unsigned long long seg_scan_heads(unsigned key, int lane)
{
    const unsigned left = (unsigned)__builtin_amdgcn_update_dpp(0, (int)key, 0x138, 0xF, 0xF, true);      // wave_shr:1 (lane 0 is a head anyway)
    return __builtin_amdgcn_ballot_w64(lane == 0 || left != key);
}
__device__ __forceinline__ int seg_scan_first(unsigned long long heads, int lane) { return 63 - __builtin_clzll(heads & (~0ull >> (63 - lane))); }
__device__ __forceinline__ double seg_scan_incl(double s, int seglo, int lane)
{
    // (every exchange is a statement of its own, in front of the select: all 64 lanes take part in it, also those that add a zero)
    const double o1 = dpp_mov<0x138>(s);                                           // wave_shr:1
    s = s + ((lane - 1 >= seglo) ? o1 : 0.0);
    const double o2 = lane_shr<2>(s, lane);
    s = s + ((lane - 2 >= seglo) ? o2 : 0.0);
    const double o4 = lane_shr<4>(s, lane);
    s = s + ((lane - 4 >= seglo) ? o4 : 0.0);
    const double o8 = lane_shr<8>(s, lane);
    s = s + ((lane - 8 >= seglo) ? o8 : 0.0);
    const double o16 = lane_shr16(s, lane);
    s = s + ((lane - 16 >= seglo) ? o16 : 0.0);
    const double o32 = lane_shr32(s);
    s = s + ((lane - 32 >= seglo) ? o32 : 0.0);
    return s;
}
__device__ __forceinline__ double seg_scan_incl(double s, unsigned key, int lane)
{
    return seg_scan_incl(s, seg_scan_first(seg_scan_heads(key, lane), lane), lane);
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
