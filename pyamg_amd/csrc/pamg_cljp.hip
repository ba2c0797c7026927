// pamg_cljp.hip -- the CLJP and CLJP-c coarse-grid selection and the MIS vertex colouring on the device.  Layer 1 of the C ABI: HOST
// arrays in, HOST arrays out.  The per-node and per-edge rules, and the argument why synchronous passes give the reference's arrays
// although it sweeps in place, are pamg_cljp.h (replayed on the host by tests/cljp_emul.cpp); every result is the reference's.
//
//   colouring  for each colour K, synchronous rounds over two state buffers, one plain launch each: an uncoloured node takes K, is out
//              for K, or waits for its lower-index in-neighbours.  The flags of CLJP_BATCH rounds are read back together, as the MIS does
//   weights    the reference's rand() draw on the host (or colour / colours on the device), then the in-degree one addition at a time
//   a pass     select (old state -> new state buffer), P5 (the rows selected in this pass; integer atomics on the decrement counters),
//              apply, P6 (a group of W = 8 / 16 / 32 / 64 lanes per row by its length, the entries selected in this pass staged in LDS;
//              rows beyond 64 entries: a wave per row that loops, staged in global scratch), apply with the count of U nodes.  The
//              counts of CLJP_BATCH passes are read back together; a pass without U nodes changes nothing
// No persistent kernel, no waiting between workgroups.
#include "pamg_common.h"
#include "pamg_cljp.h"
#include "pamg_host_call.h"

using namespace pamg;

namespace {

constexpr int CLJP_BATCH = 8;               // rounds / passes between two read-backs

int cgrid(int64_t n) { return launch_grid(n, BLK, 8192); }

// ------------------------------------------------------------------------------------------------ colouring
__global__ __launch_bounds__(BLK) void colour_round_kernel(int n, const int *__restrict__ Tp, const int *__restrict__ Tj, const int *__restrict__ prev,
                                                           int *__restrict__ next, int K, unsigned *__restrict__ flag)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) {
        int x = prev[i];
        if (x == cljp::UNDECIDED) {
            x = cljp::colour_node(i, Tp, Tj, prev, K);
            if (x == cljp::UNDECIDED) *flag = 1u;           // every writer stores the same value
        }
        next[i] = x;
    }
}

// between two colours: the nodes that were out are candidates again
__global__ __launch_bounds__(BLK) void colour_next_kernel(int n, int *__restrict__ x, unsigned *__restrict__ flag)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK)
        if (x[i] == cljp::OUT) { x[i] = cljp::UNDECIDED; *flag = 1u; }
}

// d_x[0] holds UNDECIDED everywhere; *final_buf = the buffer with the colours.  The lowest undecided node is decided in every round and
// the lowest uncoloured node is coloured by every colour, so n rounds per colour and n colours always suffice
int colouring(int n, const int *Tp, const int *Tj, int *d_x[2], unsigned *d_flags, int *final_buf, int *ncolors, int *rounds_out)
{
    int cur = 0, K = 0, total = 0;
    for (;;) {
        if (K == n) return PAMG_E_NOCONV;
        int nr = 0;
        bool done = false;
        while (!done) {
            const int batch = std::min(CLJP_BATCH, n - nr);
            if (batch <= 0) return PAMG_E_NOCONV;
            PAMG_HIP(hipMemset(d_flags, 0, sizeof(unsigned) * CLJP_BATCH));
            for (int r = 0; r < batch; ++r) {
                hipLaunchKernelGGL(colour_round_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, Tp, Tj, (const int *)d_x[cur], d_x[cur ^ 1], K, d_flags + r);
                cur ^= 1;
            }
            PAMG_HIP(hipGetLastError());
            unsigned h[CLJP_BATCH];
            PAMG_TRY(Bufs::fetch(h, d_flags, CLJP_BATCH));
            for (int r = 0; r < batch; ++r) {
                ++nr;
                if (!h[r]) { done = true; break; }          // the rounds after it in this batch changed nothing
            }
        }
        total += nr;
        ++K;
        PAMG_HIP(hipMemset(d_flags, 0, sizeof(unsigned)));
        hipLaunchKernelGGL(colour_next_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, d_x[cur], d_flags);
        PAMG_HIP(hipGetLastError());
        unsigned more = 0;
        PAMG_TRY(Bufs::fetch(&more, d_flags, 1));
        if (!more) break;
    }
    *final_buf = cur;
    *ncolors = K;
    *rounds_out = total;
    return PAMG_OK;
}

// ------------------------------------------------------------------------------------------------ CLJP
// base: the random numbers, or null with the colours in `colour`; every node starts undecided
__global__ __launch_bounds__(BLK) void cljp_init_kernel(int n, const int *__restrict__ deg, const double *__restrict__ base, const int *__restrict__ colour,
                                                        int ncolors, double *__restrict__ w, int *__restrict__ state)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) {
        w[i] = cljp::initial_weight(base ? base[i] : cljp::colour_weight(colour[i], ncolors), deg[i]);
        state[i] = cljp::U_NODE;
    }
}

__global__ __launch_bounds__(BLK) void cljp_select_kernel(int n, const int *__restrict__ Sp, const int *__restrict__ Sj, const int *__restrict__ Tp,
                                                          const int *__restrict__ Tj, const double *__restrict__ w, const int *__restrict__ prev,
                                                          int *__restrict__ next, int *__restrict__ selpass, int pass)
{
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) {
        int s = prev[i];
        if (s == cljp::U_NODE && cljp::selects(i, Sp, Sj, Tp, Tj, w, prev)) { s = cljp::C_NODE; selpass[i] = pass; }
        next[i] = s;
    }
}

// an entry of S belongs to one row, so its mark has one writer; the counters are integer atomics, whose sum has no order
__global__ __launch_bounds__(BLK) void cljp_p5_kernel(int n, const int *__restrict__ Sp, const int *__restrict__ Sj, const int *__restrict__ state,
                                                      const int *__restrict__ selpass, int pass, unsigned char *__restrict__ edgemark,
                                                      int *__restrict__ cnt)
{
    for (int c = blockIdx.x * BLK + threadIdx.x; c < n; c += gridDim.x * BLK) {
        if (selpass[c] != pass) continue;
        for (int jj = Sp[c]; jj < Sp[c + 1]; ++jj)
            if (cljp::p5_edge(c, jj, Sj, state, edgemark)) { edgemark[jj] = 0; atomicAdd(&cnt[Sj[jj]], 1); }
    }
}

// ucount != null: *ucount += the U nodes that remain
__global__ __launch_bounds__(BLK) void cljp_apply_kernel(int n, int *__restrict__ state, int *__restrict__ cnt, double *__restrict__ w,
                                                         int *__restrict__ ucount)
{
    __shared__ int s_u;
    if (threadIdx.x == 0) s_u = 0;
    __syncthreads();
    int mine = 0;
    for (int i = blockIdx.x * BLK + threadIdx.x; i < n; i += gridDim.x * BLK) {
        const int c = cnt[i];
        int s = state[i];
        if (c) {
            double wi = w[i];
            s = cljp::apply_node(s, c, &wi);
            w[i] = wi; state[i] = s; cnt[i] = 0;
        }
        mine += s == cljp::U_NODE;
    }
    if (ucount) {
        if (mine) atomicAdd(&s_u, mine);
        __syncthreads();
        if (threadIdx.x == 0 && s_u) atomicAdd(ucount, s_u);
    }
}

// One group of W lanes per listed row j.  STAGED: the row has at most W entries, so its entries selected in this pass fit W LDS slots;
// otherwise the lanes loop over the row and stage in global scratch aligned with S.  The barriers are reached by every lane of the
// workgroup the same number of times: the outer loop's bounds depend on the workgroup only.
template <int W, bool STAGED>
__global__ __launch_bounds__(BLK) void cljp_p6_kernel(int nlist, const int *__restrict__ rows, const int *__restrict__ Sp, const int *__restrict__ Sj,
                                                      const int *__restrict__ state, const int *__restrict__ selpass, int pass,
                                                      unsigned char *__restrict__ edgemark, int *__restrict__ cnt, int *g_stage)
{
    constexpr int G = BLK / W, LDS = STAGED ? BLK : 1;
    __shared__ int s_stage[LDS];
    __shared__ int s_n[G];
    const int g = threadIdx.x / W, lane = threadIdx.x % W;
    for (int base = blockIdx.x * G; base < nlist; base += gridDim.x * G) {
        const bool live = base + g < nlist;
        const int j = live ? rows[base + g] : 0;
        const int s0 = live ? Sp[j] : 0, ns = live ? Sp[j + 1] - s0 : 0;
        int *stage = STAGED ? s_stage + g * W : g_stage + s0;
        if (lane == 0) s_n[g] = 0;
        __syncthreads();
        for (int t = lane; t < ns; t += W) {
            const int c = Sj[s0 + t];
            if (cljp::stages(j, c, selpass, pass)) stage[atomicAdd(&s_n[g], 1)] = c;     // at most ns of them; their order has no say
        }
        __syncthreads();
        const int nst = s_n[g];
        if (nst)
            for (int t = lane; t < ns; t += W)
                if (cljp::p6_edge(j, s0 + t, Sp, Sj, state, edgemark, selpass, pass, stage, nst)) {
                    edgemark[s0 + t] = 0;
                    atomicAdd(&cnt[Sj[s0 + t]], 1);
                }
        __syncthreads();                                    // the slots are restaged by the next row
    }
}

template <int W, bool STAGED>
void launch_p6(int nlist, const int *rows, const int *Sp, const int *Sj, const int *state, const int *selpass, int pass, unsigned char *edgemark,
               int *cnt, int *g_stage)
{
    if (!nlist) return;
    const int G = BLK / W;
    hipLaunchKernelGGL((cljp_p6_kernel<W, STAGED>), dim3(std::min(8192, (nlist + G - 1) / G)), dim3(BLK), 0, 0, nlist, rows, Sp, Sj, state, selpass,
                       pass, edgemark, cnt, g_stage);
}

}  // namespace

extern "C" {

int pamg_vertex_coloring_mis(int32_t num_rows, const int32_t *Ap, int Ap_size, const int32_t *Aj, int Aj_size, int32_t *x, int x_size,
                             int32_t *info)
{
    const int n = num_rows;
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(n, n, Ap, Ap_size, Aj, Aj_size, &nnz));
    if (x_size < n || (n && !x)) return PAMG_E_ARG;
    if (info) info[0] = info[1] = 0;
    if (n == 0) return PAMG_OK;
    PAMG_TRY(have_device());
    Bufs d;
    int *dAp, *dAj, *ddeg, *dTp, *dTj, *dcur, *dx[2];
    unsigned *dflags;
    PAMG_TRY(d.put(&dAp, Ap, (size_t)n + 1)); PAMG_TRY(d.put(&dAj, Aj, (size_t)nnz));
    PAMG_TRY(d.get(&ddeg, (size_t)n)); PAMG_TRY(d.get(&dTp, (size_t)n + 1)); PAMG_TRY(d.get(&dTj, (size_t)nnz)); PAMG_TRY(d.get(&dcur, (size_t)n));
    PAMG_TRY(d.get(&dx[0], (size_t)n)); PAMG_TRY(d.get(&dx[1], (size_t)n)); PAMG_TRY(d.get(&dflags, CLJP_BATCH));
    PAMG_TRY(device_transposed_pattern(n, nnz, dAp, dAj, ddeg, dTp, dTj, dcur, dflags));
    PAMG_HIP(hipMemset(dx[0], 0xFF, sizeof(int) * (size_t)n));          // UNDECIDED
    int fin = 0, K = 0, nr = 0;
    PAMG_TRY(colouring(n, dTp, dTj, dx, dflags, &fin, &K, &nr));
    PAMG_TRY(Bufs::fetch(x, dx[fin], (size_t)n));
    if (info) { info[0] = K; info[1] = nr; }
    return PAMG_OK;
}

int pamg_cljp_splitting(int32_t n_nodes, const int32_t *Sp, int Sp_size, const int32_t *Sj, int Sj_size, int32_t colorflag, int32_t *splitting,
                        int splitting_size, int32_t *info)
{
    const int n = n_nodes;
    int64_t nnz = 0;
    PAMG_TRY(check_pattern(n, n, Sp, Sp_size, Sj, Sj_size, &nnz));
    if (splitting_size < n || (n && !splitting)) return PAMG_E_ARG;
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (n == 0) return PAMG_OK;                             // (the reference would take max_element of an empty range for the colour count)
    PAMG_TRY(have_device());
    Bufs d;
    int *dSp, *dSj, *ddeg, *dTp, *dTj, *dcur, *dst[2], *dcnt, *dsel, *ducount, *dstage = nullptr;
    double *dw, *dbase = nullptr;
    unsigned char *dmark;
    unsigned *dflags;
    PAMG_TRY(d.put(&dSp, Sp, (size_t)n + 1)); PAMG_TRY(d.put(&dSj, Sj, (size_t)nnz));
    PAMG_TRY(d.get(&ddeg, (size_t)n)); PAMG_TRY(d.get(&dTp, (size_t)n + 1)); PAMG_TRY(d.get(&dTj, (size_t)nnz)); PAMG_TRY(d.get(&dcur, (size_t)n));
    PAMG_TRY(d.get(&dst[0], (size_t)n)); PAMG_TRY(d.get(&dst[1], (size_t)n)); PAMG_TRY(d.get(&dcnt, (size_t)n)); PAMG_TRY(d.get(&dsel, (size_t)n));
    PAMG_TRY(d.get(&dw, (size_t)n)); PAMG_TRY(d.get(&dmark, (size_t)nnz)); PAMG_TRY(d.get(&dflags, CLJP_BATCH)); PAMG_TRY(d.get(&ducount, CLJP_BATCH));
    PAMG_TRY(device_transposed_pattern(n, nnz, dSp, dSj, ddeg, dTp, dTj, dcur, dflags));
    // weights
    int K = 0, crounds = 0;
    if (colorflag == 1) {
        int fin = 0;
        PAMG_HIP(hipMemset(dst[0], 0xFF, sizeof(int) * (size_t)n));     // UNDECIDED
        PAMG_TRY(colouring(n, dTp, dTj, dst, dflags, &fin, &K, &crounds));
        hipLaunchKernelGGL(cljp_init_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, ddeg, (const double *)nullptr, dst[fin], K, dw, dst[fin ^ 1]);
        PAMG_HIP(hipGetLastError());
        if (fin == 0) std::swap(dst[0], dst[1]);            // the start states are in dst[0]
    } else {
        std::vector<double> rnd((size_t)n);
        cljp::random_weights(n, rnd.data());
        PAMG_TRY(d.put(&dbase, (const double *)rnd.data(), (size_t)n));
        hipLaunchKernelGGL(cljp_init_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, ddeg, dbase, (const int *)nullptr, 0, dw, dst[0]);
        PAMG_HIP(hipGetLastError());
    }
    PAMG_HIP(hipMemset(dcnt, 0, sizeof(int) * (size_t)n));
    PAMG_HIP(hipMemset(dsel, 0, sizeof(int) * (size_t)n));
    if (nnz) PAMG_HIP(hipMemset(dmark, 1, (size_t)nnz));
    // the rows by size class, each class in row order
    std::vector<int> lists[cljp::NCLASS];
    for (int i = 0; i < n; ++i) {
        const int ns = Sp[i + 1] - Sp[i];
        if (ns > 0) lists[cljp::size_class(ns)].push_back(i);
    }
    int *drows[cljp::NCLASS];
    for (int c = 0; c < cljp::NCLASS; ++c) PAMG_TRY(d.put(&drows[c], (const int *)lists[c].data(), lists[c].size()));
    if (!lists[4].empty()) PAMG_TRY(d.get(&dstage, (size_t)nnz));
    // passes until no node is undecided.  At least the heaviest U node is selected per pass, so n passes always suffice
    int cur = 0, launched = 0, passes = 0;
    bool done = false;
    while (!done) {
        const int batch = std::min(CLJP_BATCH, n - launched);
        if (batch <= 0) return PAMG_E_NOCONV;
        PAMG_HIP(hipMemset(ducount, 0, sizeof(int) * CLJP_BATCH));
        for (int r = 0; r < batch; ++r) {
            const int pass = ++launched;
            hipLaunchKernelGGL(cljp_select_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, dSp, dSj, dTp, dTj, dw, (const int *)dst[cur], dst[cur ^ 1], dsel,
                               pass);
            cur ^= 1;
            int *st = dst[cur];
            hipLaunchKernelGGL(cljp_p5_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, dSp, dSj, (const int *)st, (const int *)dsel, pass, dmark, dcnt);
            hipLaunchKernelGGL(cljp_apply_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, st, dcnt, dw, (int *)nullptr);
#define PAMG_CLJP_P6(c, W, STAGED) \
            launch_p6<W, STAGED>((int)lists[c].size(), drows[c], dSp, dSj, st, dsel, pass, dmark, dcnt, dstage)
            PAMG_CLJP_P6(0, 8, true); PAMG_CLJP_P6(1, 16, true); PAMG_CLJP_P6(2, 32, true); PAMG_CLJP_P6(3, 64, true); PAMG_CLJP_P6(4, 64, false);
#undef PAMG_CLJP_P6
            hipLaunchKernelGGL(cljp_apply_kernel, dim3(cgrid(n)), dim3(BLK), 0, 0, n, st, dcnt, dw, ducount + r);
        }
        PAMG_HIP(hipGetLastError());
        int h[CLJP_BATCH];
        PAMG_TRY(Bufs::fetch(h, ducount, CLJP_BATCH));
        for (int r = 0; r < batch; ++r) {
            ++passes;
            if (!h[r]) { done = true; break; }              // the passes after it in this batch changed nothing
        }
    }
    PAMG_TRY(Bufs::fetch(splitting, dst[cur], (size_t)n));
    int selected = 0;
    for (int i = 0; i < n; ++i) {
        if (splitting[i] == cljp::U_NODE) splitting[i] = cljp::F_NODE;  // ruge_stuben.h:735-739
        selected += splitting[i] == cljp::C_NODE;
    }
    if (info) { info[0] = passes; info[1] = K; info[2] = crounds; info[3] = selected; }
    return PAMG_OK;
}

}  // extern "C"
