// pamg_lloyd.hip -- Bellman-Ford, most_interior_nodes and the Lloyd clustering loop on the device.  Layer 1 of the C ABI: HOST arrays in,
// HOST arrays out.  The per-edge and per-node rules, the argument why order-free rounds give the arrays of the reference's in-place
// serial loop, and its limit (exact weights only) are pamg_lloyd.h (replayed on the host by tests/lloyd_emul.cpp).
//
// Every kernel runs over the EDGES (the row of every entry is looked up once, on the device) or over the nodes, so a row of any length
// costs what its entries cost.  One Bellman-Ford is
//   distances  synchronous rounds: a copy of d, then every edge lowers the head's new value by a 64-bit atomic min on the bit pattern
//   stamps     in-place rounds: every tight edge whose tail is stamped offers the head (sweep << 32 | tail) by a 64-bit atomic min
//   labels     pointer jumping down the predecessor chains to the sources, then m and p of the nodes the loop wrote
// each step a plain launch repeated until its changed-flag stays clear; the flags of LL_BATCH rounds are read back together (the rounds
// behind the first clear one changed nothing).  most_interior_nodes marks the boundary, runs the same three steps from it and moves the
// centres with two more atomics per node (the cluster's largest distance, then the lowest node attaining it).  pamg_lloyd_cluster keeps
// everything resident: the graph goes up once, and per Lloyd iteration one int -- the number of centres that moved -- comes back beside
// the round flags.  No persistent kernel, no waiting between workgroups.
#include "pamg_common.h"
#include "pamg_lloyd.h"
#include "pamg_host_call.h"

using namespace pamg;
using lloyd::stamp_t;

namespace {

constexpr int LL_BATCH = 4;                 // rounds between two read-backs

int lgrid(int64_t n) { return launch_grid(n, BLK, 8192); }

#define PAMG_LLOYD_FOR(T, IT, n) for (T IT = (T)blockIdx.x * BLK + threadIdx.x; IT < (n); IT += (T)gridDim.x * BLK)

// ------------------------------------------------------------------------------------------------ one Bellman-Ford
__global__ __launch_bounds__(BLK) void ll_rows_kernel(int n, int64_t nnz, const int *__restrict__ Ap, int *__restrict__ row)
{
    PAMG_LLOYD_FOR(int64_t, e, nnz) row[e] = lloyd::row_of_entry(n, Ap, e);
}

__global__ __launch_bounds__(BLK) void ll_fill_kernel(int n, double *__restrict__ d, int *__restrict__ m, int *__restrict__ p)
{
    PAMG_LLOYD_FOR(int, i, n) {
        d[i] = lloyd::infinity();
        if (m) { m[i] = -1; p[i] = -1; }
    }
}

// The centres start unique, but a centre update can leave two clusters with one centre (a centre that stays although the boundary
// Bellman-Ford relabelled it, and the cluster it now belongs to moving onto it).  The reference's clusters[centers] = arange(...) then
// keeps the last, i.e. the largest, cluster index: m is -1 here, so that is an atomic max
__global__ __launch_bounds__(BLK) void ll_seed_kernel(int nc, const int *__restrict__ c, double *__restrict__ d, int *m)
{
    PAMG_LLOYD_FOR(int, a, nc) { d[c[a]] = 0.0; atomicMax(&m[c[a]], a); }
}

__global__ __launch_bounds__(BLK) void ll_relax_kernel(int64_t nnz, const int *__restrict__ row, const int *__restrict__ Aj,
                                                       const double *__restrict__ Ax, const double *__restrict__ dprev, double *dnext,
                                                       unsigned *__restrict__ flag)
{
    PAMG_LLOYD_FOR(int64_t, e, nnz) {
        const int j = Aj[e];
        double cand;
        if (lloyd::relaxes(dprev[row[e]], Ax[e], dprev[j], &cand)) {
            atomicMin((stamp_t *)&dnext[j], lloyd::bits_of(cand));
            *flag = 1u;                                     // every writer stores the same value
        }
    }
}

__global__ __launch_bounds__(BLK) void ll_stamp_init_kernel(int n, const double *__restrict__ d, stamp_t *__restrict__ key)
{
    PAMG_LLOYD_FOR(int, i, n) key[i] = d[i] == 0.0 ? lloyd::SOURCE_STAMP : lloyd::NO_STAMP;
}

// key is read while other lanes lower it: a stale value only offers a larger candidate, and the round is repeated
__global__ __launch_bounds__(BLK) void ll_stamp_kernel(int64_t nnz, const int *__restrict__ row, const int *__restrict__ Aj,
                                                       const double *__restrict__ Ax, const double *__restrict__ d, stamp_t *key,
                                                       unsigned *__restrict__ flag)
{
    PAMG_LLOYD_FOR(int64_t, e, nnz) {
        const int i = row[e], j = Aj[e];
        if (!lloyd::tight(d[i], Ax[e], d[j])) continue;
        const stamp_t ki = __hip_atomic_load(&key[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (ki == lloyd::NO_STAMP) continue;
        const stamp_t cand = lloyd::stamp_of(ki, i);
        if (atomicMin(&key[j], cand) > cand) *flag = 1u;
    }
}

__global__ __launch_bounds__(BLK) void ll_jump_init_kernel(int n, const stamp_t *__restrict__ key, int *__restrict__ q)
{
    PAMG_LLOYD_FOR(int, j, n) q[j] = lloyd::was_written(key[j]) ? lloyd::writer_of(key[j]) : j;
}

// in place: whatever q[q[j]] holds when it is read is an ancestor of j
__global__ __launch_bounds__(BLK) void ll_jump_kernel(int n, int *q, unsigned *__restrict__ flag)
{
    PAMG_LLOYD_FOR(int, j, n) {
        const int a = __hip_atomic_load(&q[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int b = __hip_atomic_load(&q[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (b != a) { __hip_atomic_store(&q[j], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); *flag = 1u; }
    }
}

// q[j] is a source, whose label nobody writes
__global__ __launch_bounds__(BLK) void ll_label_kernel(int n, const stamp_t *__restrict__ key, const int *__restrict__ q, int *m, int *__restrict__ p)
{
    PAMG_LLOYD_FOR(int, j, n)
        if (lloyd::was_written(key[j])) { p[j] = lloyd::writer_of(key[j]); m[j] = m[q[j]]; }
}

// ------------------------------------------------------------------------------------------------ most_interior_nodes
__global__ __launch_bounds__(BLK) void ll_boundary_kernel(int64_t nnz, const int *__restrict__ row, const int *__restrict__ Aj,
                                                          const int *__restrict__ m, double *__restrict__ d)
{
    PAMG_LLOYD_FOR(int64_t, e, nnz) {
        const int i = row[e];
        if (lloyd::is_boundary_edge(m[i], m[Aj[e]])) d[i] = 0.0;       // every writer stores the same value
    }
}

__global__ __launch_bounds__(BLK) void ll_centre_init_kernel(int nc, stamp_t *__restrict__ dmax, int *__restrict__ first)
{
    PAMG_LLOYD_FOR(int, a, nc) { dmax[a] = 0ull; first[a] = lloyd::NO_NODE; }
}

__global__ __launch_bounds__(BLK) void ll_centre_max_kernel(int n, const int *__restrict__ m, const double *__restrict__ d, stamp_t *dmax)
{
    PAMG_LLOYD_FOR(int, i, n)
        if (m[i] >= 0) atomicMax(&dmax[m[i]], lloyd::bits_of(d[i]));
}

__global__ __launch_bounds__(BLK) void ll_centre_first_kernel(int n, const int *__restrict__ m, const double *__restrict__ d,
                                                              const stamp_t *__restrict__ dmax, int *first)
{
    PAMG_LLOYD_FOR(int, i, n)
        if (m[i] >= 0 && lloyd::bits_of(d[i]) == dmax[m[i]]) atomicMin(&first[m[i]], i);
}

__global__ __launch_bounds__(BLK) void ll_centre_update_kernel(int nc, int *__restrict__ c, const double *__restrict__ d,
                                                               const stamp_t *__restrict__ dmax, const int *__restrict__ first, int *moved)
{
    PAMG_LLOYD_FOR(int, a, nc)
        if (lloyd::centre_moves(d[c[a]], lloyd::dist_of(dmax[a]), first[a])) { c[a] = first[a]; atomicAdd(moved, 1); }
}

// ------------------------------------------------------------------------------------------------ host side
// the device state of one call
struct Work {
    int n = 0, nc = 0;
    int64_t nnz = 0;
    int *row = nullptr, *Aj = nullptr, *c = nullptr, *m = nullptr, *p = nullptr, *q = nullptr, *first = nullptr, *moved = nullptr;
    double *Ax = nullptr, *d[2] = {nullptr, nullptr};
    stamp_t *key = nullptr, *dmax = nullptr;
    unsigned *flags = nullptr;
    int cur = 0;                            // d[cur] holds the distances
    int dist_rounds = 0, stamp_rounds = 0;

    int setup(Bufs &b, int n_, int64_t nnz_, const int *Ap, const int *Aj_h, const double *Ax_h, const int *c_h, int nc_)
    {
        n = n_; nnz = nnz_; nc = nc_;
        int *dAp;
        PAMG_TRY(b.put(&dAp, Ap, (size_t)n + 1)); PAMG_TRY(b.get(&row, (size_t)nnz));
        PAMG_TRY(b.put(&Aj, Aj_h, (size_t)nnz)); PAMG_TRY(b.put(&Ax, Ax_h, (size_t)nnz));
        if (nnz) hipLaunchKernelGGL(ll_rows_kernel, dim3(lgrid(nnz)), dim3(BLK), 0, 0, n, nnz, (const int *)dAp, row);
        PAMG_TRY(b.put(&c, c_h, (size_t)nc));
        PAMG_TRY(b.get(&m, (size_t)n)); PAMG_TRY(b.get(&p, (size_t)n)); PAMG_TRY(b.get(&q, (size_t)n));
        PAMG_TRY(b.get(&d[0], (size_t)n)); PAMG_TRY(b.get(&d[1], (size_t)n)); PAMG_TRY(b.get(&key, (size_t)n));
        PAMG_TRY(b.get(&dmax, (size_t)nc)); PAMG_TRY(b.get(&first, (size_t)nc)); PAMG_TRY(b.get(&moved, 1));
        PAMG_TRY(b.get(&flags, LL_BATCH));
        return PAMG_OK;
    }

    // launch(flag) until a round leaves its flag clear; *count: the rounds up to and including that one
    template <class Launch>
    int rounds(int limit, Launch launch, int *count)
    {
        int launched = 0, done = 0;
        for (;;) {
            const int batch = std::min(LL_BATCH, limit - launched);
            if (batch <= 0) return PAMG_E_NOCONV;
            PAMG_HIP(hipMemset(flags, 0, sizeof(unsigned) * LL_BATCH));
            for (int r = 0; r < batch; ++r, ++launched) PAMG_TRY(launch(flags + r));
            PAMG_HIP(hipGetLastError());
            unsigned h[LL_BATCH];
            PAMG_TRY(Bufs::fetch(h, flags, LL_BATCH));
            for (int r = 0; r < batch; ++r) {
                ++done;
                if (!h[r]) { *count = done; return PAMG_OK; }
            }
        }
    }

    // from d[cur] (0 at the sources, +inf elsewhere), m and p as they stand.  A round that changes something finishes at least the
    // nearest unfinished node, so n rounds always suffice (the last one changes nothing)
    int bellman_ford()
    {
        int nr = 0;
        PAMG_TRY(rounds(n, [&](unsigned *flag) {
            PAMG_HIP(hipMemcpyAsync(d[cur ^ 1], d[cur], sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, 0));
            hipLaunchKernelGGL(ll_relax_kernel, dim3(lgrid(nnz)), dim3(BLK), 0, 0, nnz, row, Aj, Ax, (const double *)d[cur], d[cur ^ 1], flag);
            cur ^= 1;
            return PAMG_OK;
        }, &nr));
        dist_rounds += nr;
        hipLaunchKernelGGL(ll_stamp_init_kernel, dim3(lgrid(n)), dim3(BLK), 0, 0, n, (const double *)d[cur], key);
        PAMG_TRY(rounds(n, [&](unsigned *flag) {
            hipLaunchKernelGGL(ll_stamp_kernel, dim3(lgrid(nnz)), dim3(BLK), 0, 0, nnz, row, Aj, Ax, (const double *)d[cur], key, flag);
            return PAMG_OK;
        }, &nr));
        stamp_rounds += nr;
        hipLaunchKernelGGL(ll_jump_init_kernel, dim3(lgrid(n)), dim3(BLK), 0, 0, n, (const stamp_t *)key, q);
        PAMG_TRY(rounds(40, [&](unsigned *flag) {           // a chain of fewer than 2^31 nodes halves at most 31 times
            hipLaunchKernelGGL(ll_jump_kernel, dim3(lgrid(n)), dim3(BLK), 0, 0, n, q, flag);
            return PAMG_OK;
        }, &nr));
        hipLaunchKernelGGL(ll_label_kernel, dim3(lgrid(n)), dim3(BLK), 0, 0, n, (const stamp_t *)key, (const int *)q, m, p);
        PAMG_HIP(hipGetLastError());
        return PAMG_OK;
    }

    // amg_core::most_interior_nodes from m and p as they stand; *nmoved: the centres that moved
    int most_interior(int *nmoved)
    {
        hipLaunchKernelGGL(ll_fill_kernel, dim3(lgrid(n)), dim3(BLK), 0, 0, n, d[cur], (int *)nullptr, (int *)nullptr);
        if (nnz) hipLaunchKernelGGL(ll_boundary_kernel, dim3(lgrid(nnz)), dim3(BLK), 0, 0, nnz, row, Aj, (const int *)m, d[cur]);
        PAMG_TRY(bellman_ford());
        PAMG_HIP(hipMemset(moved, 0, sizeof(int)));
        if (nc) {
            const double *dd = d[cur];
            hipLaunchKernelGGL(ll_centre_init_kernel, dim3(lgrid(nc)), dim3(BLK), 0, 0, nc, dmax, first);
            hipLaunchKernelGGL(ll_centre_max_kernel, dim3(lgrid(n)), dim3(BLK), 0, 0, n, (const int *)m, dd, dmax);
            hipLaunchKernelGGL(ll_centre_first_kernel, dim3(lgrid(n)), dim3(BLK), 0, 0, n, (const int *)m, dd, (const stamp_t *)dmax, first);
            hipLaunchKernelGGL(ll_centre_update_kernel, dim3(lgrid(nc)), dim3(BLK), 0, 0, nc, c, dd, (const stamp_t *)dmax, (const int *)first, moved);
        }
        PAMG_HIP(hipGetLastError());
        return Bufs::fetch(nmoved, (const int *)moved, 1);
    }
};

// the checks of all three entries, before any device work: the pattern with its values, exact weights, the centres
int check_graph(int n, const int *Ap, int Ap_size, const int *Aj, int Aj_size, const double *Ax, int Ax_size, const int *c, int c_size, int64_t *nnz)
{
    PAMG_TRY(check_pattern(n, n, Ap, Ap_size, Aj, Aj_size, nnz, true, Ax, Ax_size));
    if (c_size < 0 || (c_size && !c)) return PAMG_E_ARG;
    PAMG_TRY(lloyd::check_centres(n, c, c_size));
    return lloyd::check_weights(n, *nnz, Ax);
}

}  // namespace

extern "C" {

int pamg_bellman_ford(int32_t num_nodes, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const double *Ax, int Ax_size,
                      const int32_t *c, int c_size, double *d, int d_size, int32_t *m, int m_size, int32_t *p, int p_size, int32_t *info)
{
    const int n = num_nodes;
    int64_t nnz = 0;
    if (n < 0) return PAMG_E_ARG;
    if (d_size < n || m_size < n || p_size < n || (n && (!d || !m || !p))) return PAMG_E_ARG;
    PAMG_TRY(check_graph(n, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, c, c_size, &nnz));
    PAMG_TRY(lloyd::check_start(n, d));
    if (info) info[0] = info[1] = 0;
    if (n == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs b;
    Work w;
    PAMG_TRY(w.setup(b, n, nnz, Ap, Aj, Ax, c, c_size));
    PAMG_HIP(hipMemcpy(w.d[0], d, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    PAMG_HIP(hipMemcpy(w.m, m, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    PAMG_HIP(hipMemcpy(w.p, p, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    PAMG_TRY(w.bellman_ford());
    std::vector<double> hd((size_t)n);
    std::vector<int> hm((size_t)n), hp((size_t)n);          // the caller's arrays change only when everything went through
    PAMG_TRY(Bufs::fetch(hd.data(), (const double *)w.d[w.cur], (size_t)n));
    PAMG_TRY(Bufs::fetch(hm.data(), (const int *)w.m, (size_t)n)); PAMG_TRY(Bufs::fetch(hp.data(), (const int *)w.p, (size_t)n));
    std::copy(hd.begin(), hd.end(), d); std::copy(hm.begin(), hm.end(), m); std::copy(hp.begin(), hp.end(), p);
    if (info) { info[0] = w.dist_rounds; info[1] = w.stamp_rounds; }
    return PAMG_OK;
}

int pamg_most_interior_nodes(int32_t num_nodes, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const double *Ax, int Ax_size,
                             int32_t *c, int c_size, double *d, int d_size, int32_t *m, int m_size, int32_t *p, int p_size, int32_t *info)
{
    const int n = num_nodes;
    int64_t nnz = 0;
    if (n < 0) return PAMG_E_ARG;
    if (d_size < n || m_size < n || p_size < n || (n && (!d || !m || !p))) return PAMG_E_ARG;
    PAMG_TRY(check_graph(n, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, c, c_size, &nnz));
    PAMG_TRY(lloyd::check_labels(n, m, c_size));
    if (info) info[0] = info[1] = info[2] = 0;
    if (n == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs b;
    Work w;
    PAMG_TRY(w.setup(b, n, nnz, Ap, Aj, Ax, c, c_size));
    PAMG_HIP(hipMemcpy(w.m, m, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    PAMG_HIP(hipMemcpy(w.p, p, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    int nmoved = 0;
    PAMG_TRY(w.most_interior(&nmoved));
    std::vector<double> hd((size_t)n);
    std::vector<int> hm((size_t)n), hp((size_t)n), hc((size_t)c_size);
    PAMG_TRY(Bufs::fetch(hd.data(), (const double *)w.d[w.cur], (size_t)n));
    PAMG_TRY(Bufs::fetch(hm.data(), (const int *)w.m, (size_t)n)); PAMG_TRY(Bufs::fetch(hp.data(), (const int *)w.p, (size_t)n));
    PAMG_TRY(Bufs::fetch(hc.data(), (const int *)w.c, (size_t)c_size));
    std::copy(hd.begin(), hd.end(), d); std::copy(hm.begin(), hm.end(), m); std::copy(hp.begin(), hp.end(), p); std::copy(hc.begin(), hc.end(), c);
    if (info) { info[0] = w.dist_rounds; info[1] = w.stamp_rounds; info[2] = nmoved; }
    return PAMG_OK;
}

int pamg_lloyd_cluster(int32_t num_nodes, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const double *Ax, int Ax_size,
                       int32_t *c, int c_size, int32_t maxiter, int32_t *clusters, int clusters_size, int32_t *info)
{
    const int n = num_nodes;
    int64_t nnz = 0;
    if (n < 0) return PAMG_E_ARG;
    if (clusters_size < n || (n && !clusters)) return PAMG_E_ARG;
    PAMG_TRY(check_graph(n, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, c, c_size, &nnz));
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (n == 0) return PAMG_OK;
    if (maxiter <= 0) {                                     // the reference's loop does not run: the start labels
        std::fill(clusters, clusters + n, -1);
        for (int a = 0; a < c_size; ++a) clusters[c[a]] = a;
        return PAMG_OK;
    }
    PAMG_TRY(have_device());
    Bufs b;
    Work w;
    PAMG_TRY(w.setup(b, n, nnz, Ap, Aj, Ax, c, c_size));
    int it = 0, nmoved = 0;
    bool changed = true;
    while (changed && it < maxiter) {
        hipLaunchKernelGGL(ll_fill_kernel, dim3(lgrid(n)), dim3(BLK), 0, 0, n, w.d[w.cur], w.m, w.p);
        if (c_size) hipLaunchKernelGGL(ll_seed_kernel, dim3(lgrid(c_size)), dim3(BLK), 0, 0, c_size, (const int *)w.c, w.d[w.cur], w.m);
        PAMG_TRY(w.bellman_ford());
        PAMG_TRY(w.most_interior(&nmoved));
        changed = nmoved > 0;
        ++it;
    }
    std::vector<int> hm((size_t)n), hc((size_t)c_size);
    PAMG_TRY(Bufs::fetch(hm.data(), (const int *)w.m, (size_t)n)); PAMG_TRY(Bufs::fetch(hc.data(), (const int *)w.c, (size_t)c_size));
    std::copy(hm.begin(), hm.end(), clusters); std::copy(hc.begin(), hc.end(), c);
    if (info) { info[0] = it; info[1] = w.dist_rounds; info[2] = w.stamp_rounds; info[3] = nmoved; }
    return PAMG_OK;
}

}  // extern "C"
