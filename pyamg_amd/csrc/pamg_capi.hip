// pamg_capi.hip -- runtime plumbing and Layer 1 of the C ABI: the amg_core-compatible
// entry points that take HOST buffers exactly like the reference's pybind11 layer
// (pyamg/amg_core/relaxation_bind.cpp:11-44) and run the sweep on the GPU.
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <new>
#include <vector>

#include "pamg_common.h"
#include "pamg_wave.h"

using namespace pamg;

namespace {

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    int alloc(size_t bytes) { return (int)hipMalloc(&p, std::max<size_t>(bytes, 256)); }
    int put(const void *h, size_t bytes)
    {
        PAMG_TRY(alloc(bytes));
        if (bytes) PAMG_HIP(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice));
        return PAMG_OK;
    }
    int get(void *h, size_t bytes) const
    {
        if (bytes) PAMG_HIP(hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost));
        return PAMG_OK;
    }
};

struct MatGuard {
    pamg_matrix_t A = nullptr;
    bool cached = false;          // owned by the Layer-1 operator cache
    ~MatGuard() { if (A && !cached) pamg_matrix_destroy(A); }
};

// ---- Layer-1 operator cache.  The amg_core entry points get the operator as three host arrays on EVERY call; a
// smoother applied sweep after sweep would upload the matrix and redo the dependency analysis each time.  The last few
// operators stay resident instead, keyed by the identity of the arrays (addresses, sizes, dtype, block shape) AND a
// 64-bit hash of their full contents, so an operator modified in place is never mistaken for its old self.  Hashing
// streams the arrays once on the host (~10 GB/s): cheap next to the upload and the analysis it saves.  Layer-1 calls
// are synchronous and serialised by the cache's mutex.  PAMG_L1_CACHE=0 disables it; pamg_l1_cache_clear() empties it.
struct L1Entry {
    const void *Ap, *Aj, *Ax;
    int dtype, flavour, nbr, nbc, R, C;
    int64_t nblk;
    uint64_t hash;
    pamg_matrix_t A;
    uint64_t stamp;
};
std::mutex l1_mu;
std::vector<L1Entry> l1_entries;
uint64_t l1_clock = 0;
constexpr size_t L1_CAPACITY = 4;

uint64_t hash_bytes(const void *p, size_t bytes, uint64_t seed)
{
    const unsigned char *c = static_cast<const unsigned char *>(p);
    uint64_t h[4] = {seed ^ 0x9E3779B97F4A7C15ull, seed ^ 0xC2B2AE3D27D4EB4Full, seed ^ 0x165667B19E3779F9ull, seed ^ 0x27D4EB2F165667C5ull};
    size_t i = 0;
    for (; i + 32 <= bytes; i += 32) {
        uint64_t w[4];
        std::memcpy(w, c + i, 32);
        for (int k = 0; k < 4; ++k) { h[k] = (h[k] ^ w[k]) * 0xFF51AFD7ED558CCDull; h[k] ^= h[k] >> 29; }
    }
    uint64_t tail = 0;
    if (i < bytes) std::memcpy(&tail, c + i, std::min<size_t>(8, bytes - i));
    uint64_t r = (h[0] ^ tail) * 0xC4CEB9FE1A85EC53ull;
    for (size_t j = i + 8; j < bytes; ++j) r = (r ^ c[j]) * 0x100000001B3ull;
    r ^= h[1] + 0x9E3779B97F4A7C15ull + (r << 6) + (r >> 2);
    r ^= h[2] + 0x9E3779B97F4A7C15ull + (r << 6) + (r >> 2);
    r ^= h[3] + 0x9E3779B97F4A7C15ull + (r << 6) + (r >> 2);
    return r ^ bytes;
}

bool l1_enabled()
{
    static const bool on = [] { const char *e = std::getenv("PAMG_L1_CACHE"); return !(e && e[0] == '0'); }();
    return on;
}

// the operator behind (Ap, Aj, Ax): from the cache or created (and cached).  Caller holds l1_mu.
int l1_acquire(MatGuard &g, int dtype, int flavour, int nbr, int nbc, int R, int C, const int32_t *Ap, const int32_t *Aj,
               const void *Ax)
{
    if (!l1_enabled() || nbr < 0 || !Ap) return pamg_matrix_create(&g.A, dtype, flavour, nbr, nbc, R, C, Ap, Aj, Ax);
    const int64_t nblk = Ap[nbr];
    if (nblk < 0) return PAMG_E_ARG;
    const size_t ts = dtype == PAMG_F64 ? 8 : 4;
    uint64_t h = hash_bytes(Ap, sizeof(int32_t) * ((size_t)nbr + 1), 1);
    h = hash_bytes(Aj, sizeof(int32_t) * (size_t)nblk, h);
    h = hash_bytes(Ax, ts * (size_t)nblk * R * C, h);
    for (L1Entry &e : l1_entries) {
        if (e.Ap == Ap && e.Aj == Aj && e.Ax == Ax && e.dtype == dtype && e.flavour == flavour && e.nbr == nbr && e.nbc == nbc &&
            e.R == R && e.C == C && e.nblk == nblk && e.hash == h) {
            e.stamp = ++l1_clock;
            g.A = e.A;
            g.cached = true;
            return PAMG_OK;
        }
    }
    // same arrays, different contents: the old copy is stale
    for (size_t k = 0; k < l1_entries.size();) {
        if (l1_entries[k].Ap == Ap && l1_entries[k].Aj == Aj && l1_entries[k].Ax == Ax) {
            pamg_matrix_destroy(l1_entries[k].A);
            l1_entries.erase(l1_entries.begin() + (long)k);
        } else {
            ++k;
        }
    }
    PAMG_TRY(pamg_matrix_create(&g.A, dtype, flavour, nbr, nbc, R, C, Ap, Aj, Ax));
    if (l1_entries.size() >= L1_CAPACITY) {
        size_t old = 0;
        for (size_t k = 1; k < l1_entries.size(); ++k) if (l1_entries[k].stamp < l1_entries[old].stamp) old = k;
        pamg_matrix_destroy(l1_entries[old].A);
        l1_entries.erase(l1_entries.begin() + (long)old);
    }
    l1_entries.push_back(L1Entry{Ap, Aj, Ax, dtype, flavour, nbr, nbc, R, C, nblk, h, g.A, ++l1_clock});
    g.cached = true;
    return PAMG_OK;
}

template <typename T> constexpr int dt() { return sizeof(T) == 8 ? PAMG_F64 : PAMG_F32; }

int check_csr(const int32_t *Ap, int Ap_size, int Aj_size, int Ax_size, int bb)
{
    if (!Ap || Ap_size < 1) return PAMG_E_ARG;
    const int64_t nb = Ap[Ap_size - 1];
    if (nb < 0 || nb > Aj_size || nb * bb > Ax_size) return PAMG_E_ARG;
    return PAMG_OK;
}

template <typename T>
int l1_matvec(int n_brow, int n_bcol, int R, int C, const int32_t *Ap, const int32_t *Aj, const T *Ax,
              const T *Xx, T *Yx)
{
    if (n_brow < 0 || n_bcol < 0 || !Ap || (!Xx && n_bcol) || (!Yx && n_brow)) return PAMG_E_ARG;
    std::lock_guard<std::mutex> lock(l1_mu);
    MatGuard g;
    PAMG_TRY(l1_acquire(g, dt<T>(), (R == 1 && C == 1) ? PAMG_CSR : PAMG_BSR, n_brow, n_bcol, R, C, Ap, Aj, Ax));
    DevBuf x, y;
    PAMG_TRY(x.put(Xx, sizeof(T) * (size_t)n_bcol * C));
    PAMG_TRY(y.put(Yx, sizeof(T) * (size_t)n_brow * R));
    PAMG_TRY(stream_launch(g.A, EPI_ACCSEQ, x.p, nullptr, y.p, 0.0, 0.0, nullptr, nullptr));
    PAMG_HIP(hipDeviceSynchronize());
    return y.get(Yx, sizeof(T) * (size_t)n_brow * R);
}

// gauss_seidel / sor_gauss_seidel / bsr_gauss_seidel
template <typename T>
int l1_gs(int epi, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax, int Ax_size,
          T *x, int x_size, const T *b, int b_size, int row_start, int row_stop, int row_step, double omega,
          int bs)
{
    if (bs < 1 || !x || !b) return PAMG_E_ARG;
    PAMG_TRY(check_csr(Ap, Ap_size, Aj_size, Ax_size, bs * bs));
    const int nb = Ap_size - 1;
    if ((int64_t)nb * bs > x_size || (int64_t)nb * bs > b_size) return PAMG_E_ARG;
    if (row_start == row_stop) return PAMG_OK;
    std::lock_guard<std::mutex> lock(l1_mu);
    MatGuard g;
    PAMG_TRY(l1_acquire(g, dt<T>(), epi == EPI_GS_B ? PAMG_BSR : PAMG_CSR, nb, nb, bs, bs, Ap, Aj, Ax));
    DevBuf dx, db;
    PAMG_TRY(dx.put(x, sizeof(T) * (size_t)nb * bs));
    PAMG_TRY(db.put(b, sizeof(T) * (size_t)nb * bs));
    PAMG_TRY(gs_sweep(g.A, epi, dx.p, db.p, omega, row_start, row_stop, row_step, nullptr));
    PAMG_HIP(hipDeviceSynchronize());
    return dx.get(x, sizeof(T) * (size_t)nb * bs);
}

// amg_core::gauss_seidel_indexed (relaxation.h:736-790): the rows Id[row_start], Id[row_start + row_step], ... relaxed in
// place in that order.  Renumbering the unknowns so that the listed rows come first, in list order, turns this into a
// plain forward sweep over rows 0..m-1 of the renumbered operator: the stored order inside every row is kept, so every
// row sum has the reference's bits, and a listed column is "new" exactly when its row comes earlier in the list.  Rows
// that are not listed are never relaxed: the renumbered operator keeps them empty.  A list that names a row twice is
// cut into duplicate-free pieces, swept one after another.
template <typename T>
int l1_gs_indexed(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax, int Ax_size, T *x, int x_size,
                  const T *b, int b_size, const int32_t *Id, int Id_size, int row_start, int row_stop, int row_step)
{
    if (!x || !b || Id_size < 0 || (Id_size > 0 && !Id) || row_step == 0) return PAMG_E_ARG;
    PAMG_TRY(check_csr(Ap, Ap_size, Aj_size, Ax_size, 1));
    const int n = Ap_size - 1;
    if (n > x_size || n > b_size) return PAMG_E_ARG;
    const long span = (long)row_stop - row_start;
    if (span % row_step != 0 || span / row_step < 0) return PAMG_E_ARG;
    const long m_all = span / row_step;
    if (m_all == 0) return PAMG_OK;
    if (row_start < 0 || row_start >= Id_size || row_start + (m_all - 1) * row_step < 0 || row_start + (m_all - 1) * row_step >= Id_size)
        return PAMG_E_ARG;
    std::vector<int> list((size_t)m_all);
    for (long t = 0; t < m_all; ++t) {
        list[(size_t)t] = Id[row_start + t * row_step];
        if (list[(size_t)t] < 0 || list[(size_t)t] >= n) return PAMG_E_ARG;
    }
    std::lock_guard<std::mutex> lock(l1_mu);
    std::vector<int> stamp((size_t)n, -1), pos((size_t)n), inv((size_t)n), tp, tj;
    std::vector<T> tx, xs((size_t)n), bs_((size_t)n);
    size_t t0 = 0;
    int piece = 0;
    while (t0 < list.size()) {
        size_t t1 = t0;
        while (t1 < list.size() && stamp[(size_t)list[t1]] != piece) { stamp[(size_t)list[t1]] = piece; ++t1; }
        const int m = (int)(t1 - t0);
        // new number of every old row: listed rows 0..m-1 in list order, the others behind them
        std::fill(pos.begin(), pos.end(), -1);
        for (int t = 0; t < m; ++t) { pos[(size_t)list[t0 + t]] = t; inv[(size_t)t] = list[t0 + t]; }
        int next = m;
        for (int i = 0; i < n; ++i) if (pos[(size_t)i] < 0) { pos[(size_t)i] = next; inv[(size_t)next] = i; ++next; }
        tp.assign((size_t)n + 1, 0);
        for (int r = 0; r < m; ++r) tp[(size_t)r + 1] = tp[(size_t)r] + (Ap[inv[(size_t)r] + 1] - Ap[inv[(size_t)r]]);
        for (int r = m; r < n; ++r) tp[(size_t)r + 1] = tp[(size_t)r];
        tj.resize((size_t)tp[(size_t)m] + 1);
        tx.resize((size_t)tp[(size_t)m] + 1);
        for (int r = 0; r < m; ++r) {
            const int i = inv[(size_t)r];
            int w = tp[(size_t)r];
            for (int p = Ap[i]; p < Ap[i + 1]; ++p, ++w) { tj[(size_t)w] = pos[(size_t)Aj[p]]; tx[(size_t)w] = Ax[p]; }
        }
        for (int r = 0; r < n; ++r) { xs[(size_t)r] = x[inv[(size_t)r]]; bs_[(size_t)r] = b[inv[(size_t)r]]; }
        {
            MatGuard g;
            // a temporary of this call (renumbered rows in function-local arrays): created directly, never through the
            // Layer-1 cache -- it would evict a resident user operator and stay pinned behind dead addresses
            PAMG_TRY(pamg_matrix_create(&g.A, dt<T>(), PAMG_CSR, n, n, 1, 1, tp.data(), tj.data(), tx.data()));
            DevBuf dx, db;
            PAMG_TRY(dx.put(xs.data(), sizeof(T) * (size_t)n));
            PAMG_TRY(db.put(bs_.data(), sizeof(T) * (size_t)n));
            PAMG_TRY(gs_sweep(g.A, EPI_GS, dx.p, db.p, 1.0, 0, m, 1, nullptr));
            PAMG_HIP(hipDeviceSynchronize());
            PAMG_TRY(dx.get(xs.data(), sizeof(T) * (size_t)n));
        }
        for (int r = 0; r < m; ++r) x[inv[(size_t)r]] = xs[(size_t)r];
        t0 = t1;
        ++piece;
    }
    return PAMG_OK;
}

int64_t l1_schwarz_reruns = 0;        // Layer-1 Schwarz sweeps repeated as per-level launches after a time-out (under l1_mu)

// test hook, like check_sweeps of pamg_solver.hip: PAMG_FORCE_TIMEOUT=N reports the first N checks as timed out (caller holds l1_mu)
bool l1_schwarz_forced_timeout()
{
    static int forced = [] { const char *e = getenv("PAMG_FORCE_TIMEOUT"); return e ? atoi(e) : 0; }();
    if (forced <= 0) return false;
    --forced;
    return true;
}

// amg_core::overlapping_schwarz_csr (relaxation.h:1420-1492)
template <typename T>
int l1_schwarz(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax, int Ax_size, T *x, int x_size,
               const T *b, int b_size, const T *Tx, int Tx_size, const int32_t *Tp, int Tp_size, const int32_t *Sj, int Sj_size,
               const int32_t *Sp, int Sp_size, int nsdomains, int nrows, int row_start, int row_stop, int row_step)
{
    if (!x || !b || !Tp || !Sp || nsdomains < 0 || Sp_size < nsdomains + 1 || Tp_size < nsdomains + 1) return PAMG_E_ARG;
    PAMG_TRY(check_csr(Ap, Ap_size, Aj_size, Ax_size, 1));
    const int n = Ap_size - 1;
    if (n != nrows || n > x_size || n > b_size) return PAMG_E_ARG;
    if (Sp[nsdomains] > Sj_size || Tp[nsdomains] > Tx_size) return PAMG_E_ARG;
    if (row_start == row_stop) return PAMG_OK;
    std::lock_guard<std::mutex> lock(l1_mu);
    MatGuard g;
    PAMG_TRY(l1_acquire(g, dt<T>(), PAMG_CSR, n, n, 1, 1, Ap, Aj, Ax));
    pamg_schwarz_t h = nullptr;
    PAMG_TRY(pamg_schwarz_create(&h, g.A, nsdomains, Sp, Sj, Tp, Tx));
    DevBuf dx, db;
    int st = dx.put(x, sizeof(T) * (size_t)n);
    if (!st) st = db.put(b, sizeof(T) * (size_t)n);
    if (!st) st = schwarz_sweep(h, dx.p, db.p, row_start, row_stop, row_step, nullptr);
    if (!st) st = (int)hipDeviceSynchronize();
    // a wave of the persistent sweep gave up waiting: dx holds unfilled slots.  Like pamg_solver_solve: one launch per dependency level
    // from the caller's x again
    bool timed_out = false;
    if (!st) st = schwarz_error(h, &timed_out);
    if (!st && l1_schwarz_forced_timeout()) timed_out = true;
    if (!st && timed_out) {
        schwarz_level_launches(h);
        ++l1_schwarz_reruns;
        st = dx.put(x, sizeof(T) * (size_t)n);
        if (!st) st = schwarz_sweep(h, dx.p, db.p, row_start, row_stop, row_step, nullptr);
        if (!st) st = (int)hipDeviceSynchronize();
    }
    if (!st) st = dx.get(x, sizeof(T) * (size_t)n);
    pamg_schwarz_destroy(h);
    return st;
}

// amg_core::extract_subblocks (relaxation.h:1333-1396); the caller's Tp is honoured
template <typename T>
int l1_extract_subblocks(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax, int Ax_size, T *Tx, int Tx_size,
                         const int32_t *Tp, int Tp_size, const int32_t *Sj, int Sj_size, const int32_t *Sp, int Sp_size, int nsdomains, int nrows)
{
    if (!Tp || !Sp || nsdomains < 0 || Sp_size < nsdomains + 1 || Tp_size < nsdomains + 1 || Tx_size < 0 || Sj_size < 0) return PAMG_E_ARG;
    PAMG_TRY(check_csr(Ap, Ap_size, Aj_size, Ax_size, 1));
    const int n = Ap_size - 1;
    if (n != nrows) return PAMG_E_ARG;
    if (Sp[0] < 0 || Sp[nsdomains] > Sj_size || Tp[nsdomains] < 0 || Tp[nsdomains] > Tx_size) return PAMG_E_ARG;
    if ((Tx_size && !Tx) || (Sp[nsdomains] && !Sj)) return PAMG_E_ARG;
    int mmax = 0;
    for (int d = 0; d < nsdomains; ++d) {
        const int64_t m = (int64_t)Sp[d + 1] - Sp[d];
        if (m < 0 || Tp[d] < 0 || (int64_t)Tp[d] + m * m > (int64_t)Tp[nsdomains]) return PAMG_E_ARG;
        mmax = std::max<int>(mmax, (int)std::min<int64_t>(m, INT32_MAX));
    }
    if (mmax > 64) return PAMG_E_UNSUPPORTED;
    std::lock_guard<std::mutex> lock(l1_mu);
    MatGuard g;
    PAMG_TRY(l1_acquire(g, dt<T>(), PAMG_CSR, n, n, 1, 1, Ap, Aj, Ax));
    DevBuf dSp, dSj, dTp, dTx;
    PAMG_TRY(dSp.put(Sp, sizeof(int32_t) * ((size_t)nsdomains + 1)));
    PAMG_TRY(dSj.put(Sj, sizeof(int32_t) * (size_t)Sp[nsdomains]));
    PAMG_TRY(dTp.put(Tp, sizeof(int32_t) * ((size_t)nsdomains + 1)));
    PAMG_TRY(dTx.alloc(sizeof(T) * (size_t)Tp[nsdomains]));
    int64_t info[4];
    PAMG_TRY(schwarz_blocks_device(dt<T>(), g.A, nsdomains, (const int *)dSp.p, (const int *)dSj.p, (int *)dTp.p, dTx.p, Tp[nsdomains], 0.0, 0, true,
                                   nullptr, info));
    return dTx.get(Tx, sizeof(T) * (size_t)Tp[nsdomains]);
}

// jacobi / bsr_jacobi: the device sweep relaxes every row out of place; only the rows of the
// (row_start,row_stop,row_step) slice are copied back, as in the reference.
template <typename T>
int l1_jacobi(bool bsr, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax,
              int Ax_size, T *x, int x_size, const T *b, int b_size, T *temp, int temp_size, int row_start,
              int row_stop, int row_step, int bs, const T *omega, int omega_size)
{
    if (bs < 1 || !x || !b || !temp || !omega || omega_size < 1 || row_step == 0) return PAMG_E_ARG;
    PAMG_TRY(check_csr(Ap, Ap_size, Aj_size, Ax_size, bs * bs));
    const int nb = Ap_size - 1;
    const int64_t n = (int64_t)nb * bs;
    if (n > x_size || n > b_size || n > temp_size) return PAMG_E_ARG;
    const long span = (long)row_stop - row_start;
    if (span % row_step != 0 || span / row_step < 0) return PAMG_E_ARG;
    const long m = span / row_step;
    if (m == 0) return PAMG_OK;
    if (row_start < 0 || row_start >= nb || row_start + (m - 1) * row_step < 0 || row_start + (m - 1) * row_step >= nb)
        return PAMG_E_ARG;
    if (bsr && !(row_start == 0 && row_stop == nb && row_step == 1))
        return PAMG_E_UNSUPPORTED;      // the reference's partial bsr sweep snapshots x[0:m*bs] (relaxation.h:505-508)
    // reference order of events (relaxation.h:321-345): snapshot the swept entries of x into
    // temp, then relax the swept rows reading ONLY temp (entries of temp outside the slice
    // are whatever the caller left there -- the reference reads them too).
    for (long t = 0; t < m; ++t) {
        const long i = row_start + t * row_step;
        for (int k = 0; k < bs; ++k) temp[i * bs + k] = x[i * bs + k];
    }
    std::lock_guard<std::mutex> lock(l1_mu);
    MatGuard g;
    PAMG_TRY(l1_acquire(g, dt<T>(), bsr ? PAMG_BSR : PAMG_CSR, nb, nb, bs, bs, Ap, Aj, Ax));
    DevBuf dt_, db, dn;
    PAMG_TRY(dt_.put(temp, sizeof(T) * (size_t)n));
    PAMG_TRY(db.put(b, sizeof(T) * (size_t)n));
    PAMG_TRY(dn.alloc(sizeof(T) * (size_t)n));
    if (bs > 1)
        PAMG_TRY(block_jacobi_step(g.A, PNT_JACOBI, nullptr, dt_.p, dn.p, db.p, (double)omega[0], nullptr));
    else
        PAMG_TRY(stream_launch(g.A, bsr ? EPI_JACOBI_B : EPI_JACOBI, dt_.p, db.p, dn.p, 0.0, (double)omega[0], nullptr, nullptr));
    PAMG_HIP(hipDeviceSynchronize());
    std::vector<T> xn((size_t)n);
    PAMG_TRY(dn.get(xn.data(), sizeof(T) * (size_t)n));
    for (long t = 0; t < m; ++t) {
        const long i = row_start + t * row_step;
        for (int k = 0; k < bs; ++k) x[i * bs + k] = xn[(size_t)(i * bs + k)];
    }
    return PAMG_OK;
}

// jacobi_indexed (relaxation.h:382-427): temp = x; every listed row is relaxed from temp.  A row listed
// twice is simply relaxed twice from the same old values -- same result as the reference's loop.
template <typename T>
int l1_jacobi_indexed(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax, int Ax_size, T *x,
                      int x_size, const T *b, int b_size, const int32_t *indices, int indices_size, const T *omega,
                      int omega_size)
{
    if (!x || !b || !omega || omega_size < 1 || indices_size < 0 || (indices_size > 0 && !indices)) return PAMG_E_ARG;
    PAMG_TRY(check_csr(Ap, Ap_size, Aj_size, Ax_size, 1));
    const int n = Ap_size - 1;
    if (n > x_size || n > b_size) return PAMG_E_ARG;
    if (indices_size == 0) return PAMG_OK;
    std::lock_guard<std::mutex> lock(l1_mu);
    MatGuard g, sub;
    PAMG_TRY(l1_acquire(g, dt<T>(), PAMG_CSR, n, n, 1, 1, Ap, Aj, Ax));
    PAMG_TRY(matrix_row_subset(g.A, indices, indices_size, &sub.A));
    DevBuf dx, db, dw;
    PAMG_TRY(dx.put(x, sizeof(T) * (size_t)n));
    PAMG_TRY(db.put(b, sizeof(T) * (size_t)n));
    PAMG_TRY(dw.alloc(sizeof(T) * (size_t)indices_size));
    PAMG_TRY(jacobi_indexed(sub.A, dx.p, db.p, (double)omega[0], dw.p, nullptr));
    PAMG_HIP(hipDeviceSynchronize());
    return dx.get(x, sizeof(T) * (size_t)n);
}

// gauss_seidel_ne / gauss_seidel_nr: the arrays are the lines the sweep walks (rows of A for NE, the CSC
// arrays of A for NR); v is the vector the sweep reads and updates (x for NE, the residual z for NR)
template <typename T>
int l1_kaczmarz(bool nr, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax, int Ax_size, T *x,
                int x_size, T *v_nr, const T *b, int vb_size, int start, int stop, int step, const T *Tx, int Tx_size,
                double omega)
{
    if (!x || !Tx || (nr ? !v_nr : !b)) return PAMG_E_ARG;
    PAMG_TRY(check_csr(Ap, Ap_size, Aj_size, Ax_size, 1));
    const int n = Ap_size - 1;
    if (n > x_size || n > vb_size || n > Tx_size) return PAMG_E_ARG;
    if (start == stop) return PAMG_OK;
    std::lock_guard<std::mutex> lock(l1_mu);
    MatGuard g;
    PAMG_TRY(l1_acquire(g, dt<T>(), PAMG_CSR, n, n, 1, 1, Ap, Aj, Ax));
    DevBuf dx, dv, dD;
    PAMG_TRY(dx.put(x, sizeof(T) * (size_t)n));
    PAMG_TRY(dv.put(nr ? (const void *)v_nr : (const void *)b, sizeof(T) * (size_t)n));
    PAMG_TRY(dD.put(Tx, sizeof(T) * (size_t)n));
    if (nr) PAMG_TRY(kaczmarz_sweep(g.A, true, dv.p, nullptr, dD.p, omega, start, stop, step, dx.p, nullptr));
    else PAMG_TRY(kaczmarz_sweep(g.A, false, dx.p, dv.p, dD.p, omega, start, stop, step, nullptr, nullptr));
    PAMG_HIP(hipDeviceSynchronize());
    if (nr) PAMG_TRY(dv.get(v_nr, sizeof(T) * (size_t)n));
    return dx.get(x, sizeof(T) * (size_t)n);
}

// jacobi_ne (relaxation.h:811-840), full row range: temp = sum over rows of omega * a_ij * delta_i in row order
// -- an SpMV with the transposed operator whose values are omega * a_ij -- then x += temp
template <typename T>
int l1_jacobi_ne(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax, int Ax_size, T *x, int x_size,
                 const T *delta, int delta_size, T *temp, int temp_size, int row_start, int row_stop, int row_step,
                 const T *omega, int omega_size)
{
    if (!x || !delta || !temp || !omega || omega_size < 1) return PAMG_E_ARG;
    PAMG_TRY(check_csr(Ap, Ap_size, Aj_size, Ax_size, 1));
    const int n = Ap_size - 1;
    if (n > x_size || n > delta_size || n > temp_size) return PAMG_E_ARG;
    if (!(row_start == 0 && row_stop == n && row_step == 1)) return PAMG_E_UNSUPPORTED;   // the wrapper's only call
    if (n == 0) return PAMG_OK;
    const int nnz = Ap[n];
    std::vector<int32_t> tp((size_t)n + 1, 0), tj((size_t)std::max(nnz, 1));
    std::vector<T> tx((size_t)std::max(nnz, 1));
    for (int p = 0; p < nnz; ++p) {
        if (Aj[p] < 0 || Aj[p] >= n) return PAMG_E_ARG;
        tp[Aj[p] + 1]++;
    }
    for (int j = 0; j < n; ++j) tp[j + 1] += tp[j];
    std::vector<int32_t> cur(tp.begin(), tp.end() - 1);
    const T om = omega[0];
    for (int i = 0; i < n; ++i)
        for (int p = Ap[i]; p < Ap[i + 1]; ++p) {
            const int q = cur[Aj[p]]++;
            tj[q] = i;
            tx[q] = om * Ax[p];                          // omega2 * conjugate(Ax[j]), :835
        }
    MatGuard g;
    PAMG_TRY(pamg_matrix_create(&g.A, dt<T>(), PAMG_CSR, n, n, 1, 1, tp.data(), tj.data(), tx.data()));
    DevBuf dx, dd, dtmp;
    PAMG_TRY(dx.put(x, sizeof(T) * (size_t)n));
    PAMG_TRY(dd.put(delta, sizeof(T) * (size_t)n));
    PAMG_TRY(dtmp.alloc(sizeof(T) * (size_t)n));
    PAMG_TRY(stream_launch(g.A, EPI_SET, dd.p, nullptr, dtmp.p, 0.0, 0.0, nullptr, nullptr));
    PAMG_TRY(vec_axpy(dt<T>(), n, 1.0, dtmp.p, dx.p, nullptr));
    PAMG_HIP(hipDeviceSynchronize());
    PAMG_TRY(dtmp.get(temp, sizeof(T) * (size_t)n));
    return dx.get(x, sizeof(T) * (size_t)n);
}

template <typename T>
int l1_block(bool gs, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax, int Ax_size,
             T *x, int x_size, const T *b, int b_size, const T *Tx, int Tx_size, T *temp, int temp_size,
             int row_start, int row_stop, int row_step, const T *omega, int bs)
{
    if (bs < 1 || !x || !b || !Tx) return PAMG_E_ARG;
    if (bs < 2) return PAMG_E_UNSUPPORTED;     // the reference's Python layer maps bs == 1 to the point smoothers
    PAMG_TRY(check_csr(Ap, Ap_size, Aj_size, Ax_size, bs * bs));
    const int nb = Ap_size - 1;
    const int64_t n = (int64_t)nb * bs;
    if (n > x_size || n > b_size || (int64_t)nb * bs * bs > Tx_size) return PAMG_E_ARG;
    if (row_start == row_stop) return PAMG_OK;
    std::lock_guard<std::mutex> lock(l1_mu);
    MatGuard g;
    PAMG_TRY(l1_acquire(g, dt<T>(), PAMG_BSR, nb, nb, bs, bs, Ap, Aj, Ax));
    DevBuf dx, db, dd, dn;
    PAMG_TRY(dx.put(x, sizeof(T) * (size_t)n));
    PAMG_TRY(db.put(b, sizeof(T) * (size_t)n));
    PAMG_TRY(dd.put(Tx, sizeof(T) * (size_t)nb * bs * bs));
    if (gs) {
        PAMG_TRY(block_gs_sweep(g.A, dx.p, db.p, dd.p, row_start, row_stop, row_step, nullptr));
        PAMG_HIP(hipDeviceSynchronize());
        return dx.get(x, sizeof(T) * (size_t)n);
    }
    if (!temp || n > temp_size || !omega) return PAMG_E_ARG;
    if (!((row_start == 0 && row_stop == nb && row_step == 1) || (row_start == nb - 1 && row_stop == -1 && row_step == -1)))
        return PAMG_E_UNSUPPORTED;
    PAMG_TRY(dn.alloc(sizeof(T) * (size_t)n));
    PAMG_TRY(block_jacobi_step(g.A, BLK_JACOBI, dd.p, dx.p, dn.p, db.p, (double)omega[0], nullptr));
    PAMG_HIP(hipDeviceSynchronize());
    std::memcpy(temp, x, sizeof(T) * (size_t)n);
    return dn.get(x, sizeof(T) * (size_t)n);
}

// amg_core::block_jacobi_indexed (relaxation.h:1129-1199): one block-Jacobi step from the old x, kept for the listed
// block rows only
template <typename T>
int l1_block_jacobi_indexed(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax, int Ax_size, T *x,
                            int x_size, const T *b, int b_size, const T *Tx, int Tx_size, const int32_t *indices,
                            int indices_size, const T *omega, int omega_size, int bs)
{
    if (bs < 1 || !x || !b || !Tx || !omega || omega_size < 1 || indices_size < 0 || (indices_size > 0 && !indices)) return PAMG_E_ARG;
    if (bs < 2) return PAMG_E_UNSUPPORTED;     // 1x1 blocks: the reference's setup layer uses the point kernel (smoothing.py:731-734)
    PAMG_TRY(check_csr(Ap, Ap_size, Aj_size, Ax_size, bs * bs));
    const int nb = Ap_size - 1;
    const int64_t n = (int64_t)nb * bs;
    if (n > x_size || n > b_size || (int64_t)nb * bs * bs > Tx_size) return PAMG_E_ARG;
    for (int k = 0; k < indices_size; ++k) if (indices[k] < 0 || indices[k] >= nb) return PAMG_E_ARG;
    if (indices_size == 0) return PAMG_OK;
    std::lock_guard<std::mutex> lock(l1_mu);
    MatGuard g;
    PAMG_TRY(l1_acquire(g, dt<T>(), PAMG_BSR, nb, nb, bs, bs, Ap, Aj, Ax));
    std::vector<int> idx((size_t)indices_size * bs);
    for (int k = 0; k < indices_size; ++k) for (int c = 0; c < bs; ++c) idx[(size_t)k * bs + c] = indices[k] * bs + c;
    DevBuf dx, db, dd, dn, di;
    PAMG_TRY(dx.put(x, sizeof(T) * (size_t)n));
    PAMG_TRY(db.put(b, sizeof(T) * (size_t)n));
    PAMG_TRY(dd.put(Tx, sizeof(T) * (size_t)nb * bs * bs));
    PAMG_TRY(di.put(idx.data(), sizeof(int) * idx.size()));
    PAMG_TRY(dn.alloc(sizeof(T) * (size_t)n));
    PAMG_TRY(block_jacobi_step(g.A, BLK_JACOBI, dd.p, dx.p, dn.p, db.p, (double)omega[0], nullptr));
    PAMG_TRY(vec_copy_indexed(dt<T>(), (int64_t)idx.size(), (const int *)di.p, dn.p, dx.p, nullptr));
    PAMG_HIP(hipDeviceSynchronize());
    return dx.get(x, sizeof(T) * (size_t)n);
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------------------ plumbing
int pamg_l1_cache_clear(void)
{
    std::lock_guard<std::mutex> lock(l1_mu);
    for (L1Entry &e : l1_entries) pamg_matrix_destroy(e.A);
    l1_entries.clear();
    return PAMG_OK;
}

int pamg_l1_cache_size(int *entries)
{
    if (!entries) return PAMG_E_ARG;
    std::lock_guard<std::mutex> lock(l1_mu);
    *entries = (int)l1_entries.size();
    return PAMG_OK;
}

int pamg_l1_schwarz_reruns(int64_t *count)
{
    if (!count) return PAMG_E_ARG;
    std::lock_guard<std::mutex> lock(l1_mu);
    *count = l1_schwarz_reruns;
    return PAMG_OK;
}

const char *pamg_version(void) { return "pyamg_amd 0.1.0 (gfx950, ROCm " PAMG_STR(HIP_VERSION_MAJOR) "." PAMG_STR(HIP_VERSION_MINOR) ")"; }

const char *pamg_status_string(int st)
{
    switch (st) {
        case PAMG_OK: return "ok";
        case PAMG_E_ARG: return "invalid argument";
        case PAMG_E_UNSUPPORTED: return "not supported on the device path";
        case PAMG_E_NODEVICE: return "no HIP device";
        case PAMG_E_STATE: return "invalid call sequence";
        case PAMG_E_ALLOC: return "host allocation failed";
        case PAMG_E_TIMEOUT: return "a persistent sweep hit its spin bound; results are invalid";
        case PAMG_E_COMM: return "RCCL / transport failure in the sharded cycle";
        case PAMG_E_NOCONV: return "an iteration of a setup kernel did not converge; results are invalid";
    }
    if (st > 0) return hipGetErrorString((hipError_t)st);
    return "unknown error";
}

// ---- measured bandwidth ceiling of this device (bench.py reports it beside the 8 TB/s datasheet peak)
extern "C++" {
namespace {
__global__ __launch_bounds__(256) void bw_copy_kernel(const double2 *__restrict__ a, double2 *__restrict__ c, int64_t n2)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256) c[i] = a[i];
}
__global__ __launch_bounds__(256) void bw_triad_kernel(const double2 *__restrict__ a, const double2 *__restrict__ b, double2 *__restrict__ c, double s, int64_t n2)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256) {
        const double2 x = a[i], y = b[i];
        double2 r;
        r.x = x.x + s * y.x;
        r.y = x.y + s * y.y;
        c[i] = r;
    }
}
// variants of the copy (which access shape gets closest to the HBM on this part): U 16-byte accesses per lane, one block-contiguous
// piece per workgroup, no loop; NT = nontemporal loads and stores
template <int U, bool NT>
__global__ __launch_bounds__(256) void bw_copy_block_kernel(const double2 *__restrict__ a, double2 *__restrict__ c, int64_t n2)
{
    const int64_t base = (int64_t)blockIdx.x * (256 * U) + threadIdx.x;
    double2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t i = base + (int64_t)u * 256;
        if (i < n2) {
            if (NT) { v[u].x = __builtin_nontemporal_load(&a[i].x); v[u].y = __builtin_nontemporal_load(&a[i].y); }
            else v[u] = a[i];
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t i = base + (int64_t)u * 256;
        if (i < n2) {
            if (NT) { __builtin_nontemporal_store(v[u].x, &c[i].x); __builtin_nontemporal_store(v[u].y, &c[i].y); }
            else c[i] = v[u];
        }
    }
}
template <bool NT>
__global__ __launch_bounds__(256) void bw_copy8_kernel(const double *__restrict__ a, double *__restrict__ c, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        if (NT) __builtin_nontemporal_store(__builtin_nontemporal_load(a + i), c + i);
        else c[i] = a[i];
    }
}
template <int U>
__global__ __launch_bounds__(256) void bw_read_kernel(const double2 *__restrict__ a, double *__restrict__ c, int64_t n2)
{
    const int64_t base = (int64_t)blockIdx.x * (256 * U) + threadIdx.x;
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t i = base + (int64_t)u * 256;
        if (i < n2) { const double2 v = a[i]; s += v.x + v.y; }
    }
    if (s == 1.2345e300) c[0] = s;                                  // never true for the zero-filled probe vectors; keeps the loads
}
// what ONE XCD reads: workgroups on the other seven leave at once, the 1/8 that stay walk the whole vector (16-byte loads, U per trip).
// The one-XCD forms of the sweeps are bound by this when a dependency level streams more than the hand-off takes.
template <int U>
__global__ __launch_bounds__(256) void bw_read_xcd_kernel(const double2 *__restrict__ a, double *__restrict__ c, int64_t n2, int home_wgs)
{
    if (xcc_id() != 0) return;
    const int64_t w = blockIdx.x >> 3;                                                   // (round-robin placement: every eighth workgroup is here)
    double s = 0.0;
    for (int64_t base = w * (256 * U) + threadIdx.x; base < n2; base += (int64_t)home_wgs * (256 * U)) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = base + (int64_t)u * 256;
            if (i < n2) { const double2 v = a[i]; s += v.x + v.y; }
        }
    }
    if (s == 1.2345e300) c[0] = s;
}
template <int U>
__global__ __launch_bounds__(256) void bw_write_kernel(double2 *__restrict__ c, int64_t n2)
{
    const int64_t base = (int64_t)blockIdx.x * (256 * U) + threadIdx.x;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t i = base + (int64_t)u * 256;
        if (i < n2) c[i] = double2{0.0, 0.0};
    }
}
}  // namespace
}  // extern "C++"

// kind 0 copy (grid-stride), 1 triad, 2 copy 1 x 16 B per lane, 3 copy 4 x 16 B, 4 copy 4 x 16 B nontemporal, 5 copy 8 x 16 B,
// 6 read only (4 x 16 B), 7 write only (4 x 16 B), 8 hipMemcpyAsync device to device, 9 copy 1 x 8 B per lane, 10 the same nontemporal,
// 11 copy 1 x 16 B nontemporal
int pamg_bandwidth_probe(int kind, int64_t n, int reps, double *gbps)
{
    if (kind < 0 || kind > 13 || n < 1024 || reps < 1 || !gbps) return PAMG_E_ARG;
    n &= ~(int64_t)1;
    double *a = nullptr, *b = nullptr, *c = nullptr;
    PAMG_HIP(hipMalloc((void **)&a, (size_t)n * 8));
    if (hipMalloc((void **)&b, (size_t)n * 8) != hipSuccess) { hipFree(a); return PAMG_E_ALLOC; }
    if (hipMalloc((void **)&c, (size_t)n * 8) != hipSuccess) { hipFree(a); hipFree(b); return PAMG_E_ALLOC; }
    hipMemset(a, 0, (size_t)n * 8); hipMemset(b, 0, (size_t)n * 8); hipMemset(c, 0, (size_t)n * 8);
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    const int64_t n2 = n / 2;
    const int grid = (int)std::min<int64_t>((n2 + 255) / 256, 256 * 64);
    auto blocks = [&](int U) { return dim3((unsigned)((n2 + 256 * U - 1) / (256 * U))); };
    auto run = [&]() {
        switch (kind) {
            case 0: hipLaunchKernelGGL(bw_copy_kernel, dim3(grid), dim3(256), 0, 0, (const double2 *)a, (double2 *)c, n2); break;
            case 1: hipLaunchKernelGGL(bw_triad_kernel, dim3(grid), dim3(256), 0, 0, (const double2 *)a, (const double2 *)b, (double2 *)c, 0.5, n2); break;
            case 2: hipLaunchKernelGGL((bw_copy_block_kernel<1, false>), blocks(1), dim3(256), 0, 0, (const double2 *)a, (double2 *)c, n2); break;
            case 3: hipLaunchKernelGGL((bw_copy_block_kernel<4, false>), blocks(4), dim3(256), 0, 0, (const double2 *)a, (double2 *)c, n2); break;
            case 4: hipLaunchKernelGGL((bw_copy_block_kernel<4, true>), blocks(4), dim3(256), 0, 0, (const double2 *)a, (double2 *)c, n2); break;
            case 5: hipLaunchKernelGGL((bw_copy_block_kernel<8, false>), blocks(8), dim3(256), 0, 0, (const double2 *)a, (double2 *)c, n2); break;
            case 6: hipLaunchKernelGGL((bw_read_kernel<4>), blocks(4), dim3(256), 0, 0, (const double2 *)a, c, n2); break;
            case 7: hipLaunchKernelGGL((bw_write_kernel<4>), blocks(4), dim3(256), 0, 0, (double2 *)c, n2); break;
            case 9: hipLaunchKernelGGL((bw_copy8_kernel<false>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const double *)a, c, n); break;
            case 10: hipLaunchKernelGGL((bw_copy8_kernel<true>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (const double *)a, c, n); break;
            case 11: hipLaunchKernelGGL((bw_copy_block_kernel<1, true>), blocks(1), dim3(256), 0, 0, (const double2 *)a, (double2 *)c, n2); break;
            case 12: hipLaunchKernelGGL((bw_read_xcd_kernel<4>), dim3(8 * 256), dim3(256), 0, 0, (const double2 *)a, c, n2, 256); break;    // 8 workgroups per CU of the XCD
            case 13: hipLaunchKernelGGL((bw_read_xcd_kernel<4>), dim3(8 * 64), dim3(256), 0, 0, (const double2 *)a, c, n2, 64); break;      // 2 per CU
            default: hipMemcpyAsync(c, a, (size_t)n * 8, hipMemcpyDeviceToDevice, 0); break;
        }
    };
    for (int i = 0; i < 3; ++i) run();
    hipEventRecord(e0, 0);
    for (int i = 0; i < reps; ++i) run();
    hipEventRecord(e1, 0);
    hipEventSynchronize(e1);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    const hipError_t err = hipGetLastError();
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(a); hipFree(b); hipFree(c);
    if (err != hipSuccess) return (int)err;
    const double bytes = (kind == 1 ? 24.0 : (kind == 6 || kind == 7 || kind == 12 || kind == 13) ? 8.0 : 16.0) * (double)n * reps;
    *gbps = ms > 0.f ? bytes / ((double)ms * 1e6) : 0.0;
    return PAMG_OK;
}

// ---- the segmented scan of the cluster layout (pamg_wave.h) on its own: one wave per 64 (key, value) pairs
extern "C++" {
namespace {
__global__ __launch_bounds__(256) void segscan_probe_kernel(const unsigned *__restrict__ keys, const double *__restrict__ vals, double *__restrict__ out, int64_t nwaves)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nwaves) return;                                                             // (wave-uniform: a wave that stays is whole)
    const int64_t i = w * 64 + lane;
    out[i] = seg_scan_incl(vals[i], keys[i], lane);
}
}  // namespace
}  // extern "C++"

int pamg_segscan_probe(int64_t nwaves, const unsigned *keys, const double *vals, double *out)
{
    if (nwaves < 1 || nwaves > ((int64_t)1 << 24) || !keys || !vals || !out) return PAMG_E_ARG;
    const size_t n = (size_t)nwaves * 64;
    unsigned *dk = nullptr;
    double *dv = nullptr, *dout = nullptr;
    PAMG_HIP(hipMalloc((void **)&dk, n * sizeof(unsigned)));
    if (hipMalloc((void **)&dv, n * 8) != hipSuccess) { hipFree(dk); return PAMG_E_ALLOC; }
    if (hipMalloc((void **)&dout, n * 8) != hipSuccess) { hipFree(dk); hipFree(dv); return PAMG_E_ALLOC; }
    hipError_t err = hipMemcpy(dk, keys, n * sizeof(unsigned), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(dv, vals, n * 8, hipMemcpyHostToDevice);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(segscan_probe_kernel, dim3((unsigned)((nwaves + 3) / 4)), dim3(256), 0, 0, (const unsigned *)dk, (const double *)dv, dout, nwaves);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipMemcpy(out, dout, n * 8, hipMemcpyDeviceToHost);
    hipFree(dk); hipFree(dv); hipFree(dout);
    return (int)err;
}

int pamg_device_count(int *count)
{
    if (!count) return PAMG_E_ARG;
    *count = 0;
    const hipError_t e = hipGetDeviceCount(count);
    if (e == hipErrorNoDevice) { *count = 0; return PAMG_OK; }
    return (int)e;
}
int pamg_set_device(int device) { return (int)hipSetDevice(device); }
int pamg_get_device(int *device) { return device ? (int)hipGetDevice(device) : PAMG_E_ARG; }
int pamg_device_name(int device, char *buf, int buflen)
{
    if (!buf || buflen < 1) return PAMG_E_ARG;
    hipDeviceProp_t p;
    PAMG_HIP(hipGetDeviceProperties(&p, device));
    std::snprintf(buf, (size_t)buflen, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
    return PAMG_OK;
}
int pamg_malloc(void **dptr, size_t bytes) { return dptr ? (int)hipMalloc(dptr, std::max<size_t>(bytes, 256)) : PAMG_E_ARG; }
int pamg_free(void *dptr) { return (int)hipFree(dptr); }
int pamg_memcpy_h2d(void *dst, const void *src, size_t bytes, pamg_stream_t s)
{
    if (!bytes) return PAMG_OK;
    return s ? (int)hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)s)
             : (int)hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
}
int pamg_memcpy_d2h(void *dst, const void *src, size_t bytes, pamg_stream_t s)
{
    if (!bytes) return PAMG_OK;
    return s ? (int)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)s)
             : (int)hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
}
int pamg_memcpy_d2d(void *dst, const void *src, size_t bytes, pamg_stream_t s)
{
    if (!bytes) return PAMG_OK;
    return (int)hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)s);
}
int pamg_memset(void *dst, int byte, size_t bytes, pamg_stream_t s)
{
    if (!bytes) return PAMG_OK;
    return (int)hipMemsetAsync(dst, byte, bytes, (hipStream_t)s);
}
int pamg_stream_create(pamg_stream_t *s) { return s ? (int)hipStreamCreateWithFlags((hipStream_t *)s, hipStreamNonBlocking) : PAMG_E_ARG; }
int pamg_stream_destroy(pamg_stream_t s) { return (int)hipStreamDestroy((hipStream_t)s); }
int pamg_stream_synchronize(pamg_stream_t s) { return (int)hipStreamSynchronize((hipStream_t)s); }
int pamg_device_synchronize(void) { return (int)hipDeviceSynchronize(); }
int pamg_event_create(pamg_event_t *e) { return e ? (int)hipEventCreate((hipEvent_t *)e) : PAMG_E_ARG; }
int pamg_event_destroy(pamg_event_t e) { return (int)hipEventDestroy((hipEvent_t)e); }
int pamg_event_record(pamg_event_t e, pamg_stream_t s) { return (int)hipEventRecord((hipEvent_t)e, (hipStream_t)s); }
int pamg_event_synchronize(pamg_event_t e) { return (int)hipEventSynchronize((hipEvent_t)e); }
int pamg_event_elapsed_ms(pamg_event_t a, pamg_event_t b, float *ms) { return ms ? (int)hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b) : PAMG_E_ARG; }

// -------------------------------------------------------------------- Layer 1 (HOST buffers)
#define PAMG_L1(T, SFX)                                                                                         \
    int pamg_csr_matvec_##SFX(int n_row, int n_col, const int32_t *Ap, const int32_t *Aj, const T *Ax,          \
                              const T *Xx, T *Yx)                                                               \
    { return l1_matvec<T>(n_row, n_col, 1, 1, Ap, Aj, Ax, Xx, Yx); }                                            \
    int pamg_bsr_matvec_##SFX(int n_brow, int n_bcol, int R, int C, const int32_t *Ap, const int32_t *Aj,       \
                              const T *Ax, const T *Xx, T *Yx)                                                  \
    { return l1_matvec<T>(n_brow, n_bcol, R, C, Ap, Aj, Ax, Xx, Yx); }                                          \
    int pamg_gauss_seidel_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax,    \
                                int Ax_size, T *x, int x_size, const T *b, int b_size, int32_t row_start,       \
                                int32_t row_stop, int32_t row_step)                                             \
    { return l1_gs<T>(EPI_GS, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, x, x_size, b, b_size, row_start, row_stop, \
                      row_step, 1.0, 1); }                                                                      \
    int pamg_gauss_seidel_indexed_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax, \
                                        int Ax_size, T *x, int x_size, const T *b, int b_size, const int32_t *Id,\
                                        int Id_size, int32_t row_start, int32_t row_stop, int32_t row_step)     \
    { return l1_gs_indexed<T>(Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, x, x_size, b, b_size, Id, Id_size,         \
                              row_start, row_stop, row_step); }                                                 \
    int pamg_overlapping_schwarz_csr_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size,      \
                                           const T *Ax, int Ax_size, T *x, int x_size, const T *b, int b_size,  \
                                           const T *Tx, int Tx_size, const int32_t *Tp, int Tp_size,            \
                                           const int32_t *Sj, int Sj_size, const int32_t *Sp, int Sp_size,      \
                                           int32_t nsdomains, int32_t nrows, int32_t row_start,                 \
                                           int32_t row_stop, int32_t row_step)                                  \
    { return l1_schwarz<T>(Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, x, x_size, b, b_size, Tx, Tx_size, Tp, Tp_size,\
                           Sj, Sj_size, Sp, Sp_size, nsdomains, nrows, row_start, row_stop, row_step); }        \
    int pamg_extract_subblocks_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size,            \
                                     const T *Ax, int Ax_size, T *Tx, int Tx_size, const int32_t *Tp,           \
                                     int Tp_size, const int32_t *Sj, int Sj_size, const int32_t *Sp,            \
                                     int Sp_size, int32_t nsdomains, int32_t nrows)                             \
    { return l1_extract_subblocks<T>(Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, Tx, Tx_size, Tp, Tp_size, Sj,       \
                                     Sj_size, Sp, Sp_size, nsdomains, nrows); }                                 \
    int pamg_sor_gauss_seidel_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size,             \
                                    const T *Ax, int Ax_size, T *x, int x_size, const T *b, int b_size,         \
                                    int32_t row_start, int32_t row_stop, int32_t row_step, T omega)             \
    { return l1_gs<T>(EPI_SOR, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, x, x_size, b, b_size, row_start,          \
                      row_stop, row_step, (double)omega, 1); }                                                  \
    int pamg_bsr_gauss_seidel_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size,             \
                                    const T *Ax, int Ax_size, T *x, int x_size, const T *b, int b_size,         \
                                    int32_t row_start, int32_t row_stop, int32_t row_step, int32_t blocksize)   \
    { return l1_gs<T>(EPI_GS_B, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, x, x_size, b, b_size, row_start,         \
                      row_stop, row_step, 1.0, blocksize); }                                                    \
    int pamg_jacobi_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax,          \
                          int Ax_size, T *x, int x_size, const T *b, int b_size, T *temp, int temp_size,        \
                          int32_t row_start, int32_t row_stop, int32_t row_step, const T *omega,                \
                          int omega_size)                                                                       \
    { return l1_jacobi<T>(false, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, x, x_size, b, b_size, temp, temp_size,  \
                          row_start, row_stop, row_step, 1, omega, omega_size); }                               \
    int pamg_gauss_seidel_ne_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax, \
                                   int Ax_size, T *x, int x_size, const T *b, int b_size, int32_t row_start,   \
                                   int32_t row_stop, int32_t row_step, const T *Tx, int Tx_size, T omega)      \
    { return l1_kaczmarz<T>(false, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, x, x_size, nullptr, b, b_size,       \
                            row_start, row_stop, row_step, Tx, Tx_size, (double)omega); }                       \
    int pamg_gauss_seidel_nr_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax, \
                                   int Ax_size, T *x, int x_size, T *z, int z_size, int32_t col_start,         \
                                   int32_t col_stop, int32_t col_step, const T *Tx, int Tx_size, T omega)      \
    { return l1_kaczmarz<T>(true, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, x, x_size, z, nullptr, z_size,        \
                            col_start, col_stop, col_step, Tx, Tx_size, (double)omega); }                       \
    int pamg_jacobi_ne_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax,       \
                             int Ax_size, T *x, int x_size, const T *b, int b_size, const T *Tx, int Tx_size,  \
                             T *temp, int temp_size, int32_t row_start, int32_t row_stop, int32_t row_step,    \
                             const T *omega, int omega_size)                                                   \
    { (void)b; (void)b_size;                                                                                    \
      return l1_jacobi_ne<T>(Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, x, x_size, Tx, Tx_size, temp, temp_size,   \
                             row_start, row_stop, row_step, omega, omega_size); }                               \
    int pamg_jacobi_indexed_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax,  \
                                  int Ax_size, T *x, int x_size, const T *b, int b_size,                        \
                                  const int32_t *indices, int indices_size, const T *omega, int omega_size)     \
    { return l1_jacobi_indexed<T>(Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, x, x_size, b, b_size, indices,         \
                                  indices_size, omega, omega_size); }                                           \
    int pamg_block_jacobi_indexed_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax, \
                                        int Ax_size, T *x, int x_size, const T *b, int b_size, const T *Tx,      \
                                        int Tx_size, const int32_t *indices, int indices_size, const T *omega,  \
                                        int omega_size, int32_t blocksize)                                      \
    { return l1_block_jacobi_indexed<T>(Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, x, x_size, b, b_size, Tx, Tx_size,\
                                        indices, indices_size, omega, omega_size, blocksize); }                 \
    int pamg_bsr_jacobi_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax,      \
                              int Ax_size, T *x, int x_size, const T *b, int b_size, T *temp, int temp_size,    \
                              int32_t row_start, int32_t row_stop, int32_t row_step, int32_t blocksize,         \
                              const T *omega, int omega_size)                                                   \
    { return l1_jacobi<T>(true, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, x, x_size, b, b_size, temp, temp_size,   \
                          row_start, row_stop, row_step, blocksize, omega, omega_size); }                       \
    int pamg_block_jacobi_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, const T *Ax,    \
                                int Ax_size, T *x, int x_size, const T *b, int b_size, const T *Tx,             \
                                int Tx_size, T *temp, int temp_size, int32_t row_start, int32_t row_stop,       \
                                int32_t row_step, const T *omega, int omega_size, int32_t blocksize)            \
    { (void)omega_size;                                                                                         \
      return l1_block<T>(false, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, x, x_size, b, b_size, Tx, Tx_size, temp, \
                         temp_size, row_start, row_stop, row_step, omega, blocksize); }                         \
    int pamg_block_gauss_seidel_##SFX(const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size,           \
                                      const T *Ax, int Ax_size, T *x, int x_size, const T *b, int b_size,       \
                                      const T *Tx, int Tx_size, int32_t row_start, int32_t row_stop,            \
                                      int32_t row_step, int32_t blocksize)                                      \
    { return l1_block<T>(true, Ap, Ap_size, Aj, Aj_size, Ax, Ax_size, x, x_size, b, b_size, Tx, Tx_size,        \
                         nullptr, 0, row_start, row_stop, row_step, nullptr, blocksize); }

PAMG_L1(double, f64)
PAMG_L1(float, f32)

}  // extern "C"
