// pamg_solver.hip -- smoother drivers on operator handles and the device-resident
// multigrid cycle / outer iteration (MultilevelSolver.__solve and .solve,
// reference pyamg/multilevel.py:584-662 and :537-582).
//
// Every level vector is preallocated once; a cycle is a fixed sequence of kernel launches
// on one stream, captured into a hipGraph per (cycle type, cycles_per_level) and replayed,
// which removes the host launch cost of the many tiny coarse-level / GS-level kernels.
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <functional>
#include <map>
#include <new>
#include <thread>

#include "pamg_common.h"

using namespace pamg;

namespace {

struct Smoother {
    int kind = PAMG_SMOOTH_NONE;
    int iterations = 1;
    double omega = 1.0;
    int sweep = PAMG_FORWARD;
    std::vector<double> coeffs;
    void *d_Dinv = nullptr;
    int blocksize = 1;
    // CF / FC Jacobi: row-subset copies of the level operator and one work value per listed row
    pamg_matrix_s *AF = nullptr, *AC = nullptr;
    void *wF = nullptr, *wC = nullptr;
    int f_iterations = 1, c_iterations = 1;
    // CF / FC block Jacobi: scalar indices of the listed block rows
    int *iF = nullptr, *iC = nullptr;
    int64_t nF = 0, nC = 0;
    pamg_schwarz_s *sw = nullptr;     // Schwarz: subdomains + inverted blocks + schedules (owned)
    // normal-equation smoothers: d_Dinv holds 1/||row||^2 or 1/||col||^2; At is borrowed (see the header)
    pamg_matrix_s *At = nullptr, *Ar = nullptr;
    // Krylov methods as smoothers (smoothing.py:794-830): x[:] = method(A, b, x0=x, tol, maxiter, [restart])[0]; At (borrowed) = A^H for cgne / cgnr
    int kmethod = 0, kmaxiter = 1, krestart = 0;
    double ktol = 1e-12;
    void *kw = nullptr;               // 4 n work values
};

struct Level {
    pamg_matrix_s *A = nullptr, *P = nullptr, *R = nullptr;
    Smoother pre, post;
    int64_t n = 0;
    void *x = nullptr, *xalt = nullptr;   // ping-pong pair; x is where the iterate lives NOW
    void *x_home = nullptr;               // canonical buffer (graph replays start/end here)
    void *b = nullptr, *r = nullptr, *work = nullptr;
    void *amli = nullptr;                 // AMLI: [p0 | p1 | q | acc], 4n values (allocated on first use)
};

int sweep_bounds(const pamg_matrix_s *A, int dir, int &r0, int &r1, int &rs)
{
    const int n = A->R > 1 ? A->n_brow : (int)A->nrows;
    if (dir == PAMG_FORWARD) { r0 = 0; r1 = n; rs = 1; }
    else if (dir == PAMG_BACKWARD) { r0 = n - 1; r1 = -1; rs = -1; }
    else return PAMG_E_ARG;
    return PAMG_OK;
}

bool square_ok(const pamg_matrix_s *A) { return A && A->nrows == A->ncols && A->R == A->C; }

// weighted Jacobi, ping-pong between *px and *palt (relaxation.py:349-420: the reference
// snapshots x into temp and rewrites x; we read the old iterate and write the new one into
// the partner buffer, which is the same arithmetic without the copy pass)
int jacobi_pp(pamg_matrix_s *A, void **px, void **palt, const void *b, double omega, int its, hipStream_t s)
{
    if (!square_ok(A)) return PAMG_E_ARG;
    if (A->nrows == 0) return PAMG_OK;
    for (int it = 0; it < its; ++it) {
        if (A->R > 1)
            PAMG_TRY(block_jacobi_step(A, PNT_JACOBI, nullptr, *px, *palt, b, omega, s));
        else
            PAMG_TRY(stream_launch(A, A->flavour == PAMG_BSR ? EPI_JACOBI_B : EPI_JACOBI, *px, b, *palt,
                                   0.0, omega, nullptr, s));
        std::swap(*px, *palt);
    }
    return PAMG_OK;
}

int block_jacobi_pp(pamg_matrix_s *A, void **px, void **palt, const void *b, const void *Dinv,
                    double omega, int its, hipStream_t s)
{
    if (!square_ok(A) || A->R < 2 || !Dinv) return PAMG_E_ARG;
    for (int it = 0; it < its; ++it) {
        PAMG_TRY(block_jacobi_step(A, BLK_JACOBI, Dinv, *px, *palt, b, omega, s));
        std::swap(*px, *palt);
    }
    return PAMG_OK;
}

// relaxation.gauss_seidel / relaxation.sor as the reference runs them (relaxation.py:265-346,
// :100-154).  Quirks mirrored on purpose: sweep='symmetric' drops omega (:326-330), the BSR
// flavour ignores omega (:343-346).
// r: a scratch vector of the operator's size (a solver's level residual) -- a symmetric sweep that is not announced to start from zero may then run in
// correction form (gs_sweep_correction, PAMG_TUNE_GS_CORRECTION); nullptr (a bare operator): never
int gs_apply(pamg_matrix_s *A, void *x, const void *b, int sweep, double omega, int its, hipStream_t s, bool x_zero = false, void *r = nullptr)
{
    if (!square_ok(A)) return PAMG_E_ARG;
    if (A->nrows == 0) return PAMG_OK;
    auto one = [&](int dir, double om) -> int {
        int r0, r1, rs;
        PAMG_TRY(sweep_bounds(A, dir, r0, r1, rs));
        int epi;
        if (A->R > 1 || A->flavour == PAMG_BSR) epi = EPI_GS_B;
        else epi = (om != 1.0) ? EPI_SOR : EPI_GS;
        return gs_sweep(A, epi, x, b, om, r0, r1, rs, s);
    };
    if (sweep == PAMG_SYMMETRIC) {
        for (int it = 0; it < its; ++it) {
            // one launch where both directions take the same fast form (x_zero holds for the first iteration only)
            bool ran = false;
            // a level that holds the dense block-triangular form (pamg_dtri.hip): from zero x = S b, else r = b - A x and x += S r
            PAMG_TRY(gs_sweep_dtri(A, x, b, r, x_zero && it == 0, s, &ran));
            if (ran) continue;
            // from x != 0 on a level that holds zero-iterate plans: r = b - A x, then x += sweep(0, r) on those plans
            if (r && !(x_zero && it == 0)) PAMG_TRY(gs_sweep_correction(A, x, b, r, false, s, &ran));
            if (ran) continue;
            PAMG_TRY(gs_sweep_symmetric(A, x, b, x_zero && it == 0, s, &ran));
            if (ran) continue;
            // two launches: from x = 0 on the operator's zero-iterate plans where it holds them (what the fused launch runs: the same bits)
            if (x_zero && it == 0) PAMG_TRY(gs_sweep_zero_pair(A, x, b, s, &ran));
            if (ran) continue;
            PAMG_TRY(one(PAMG_FORWARD, 1.0));
            PAMG_TRY(one(PAMG_BACKWARD, 1.0));
        }
        return PAMG_OK;
    }
    for (int it = 0; it < its; ++it) PAMG_TRY(one(sweep, omega));
    return PAMG_OK;
}

int block_gs_apply(pamg_matrix_s *A, void *x, const void *b, const void *Dinv, int sweep, int its,
                   hipStream_t s)
{
    if (!square_ok(A) || A->R < 2 || !Dinv) return PAMG_E_ARG;
    auto one = [&](int dir) -> int {
        int r0, r1, rs;
        PAMG_TRY(sweep_bounds(A, dir, r0, r1, rs));
        return block_gs_sweep(A, x, b, Dinv, r0, r1, rs, s);
    };
    for (int it = 0; it < its; ++it) {
        if (sweep == PAMG_SYMMETRIC) { PAMG_TRY(one(PAMG_FORWARD)); PAMG_TRY(one(PAMG_BACKWARD)); }
        else PAMG_TRY(one(sweep));
    }
    return PAMG_OK;
}

// relaxation.polynomial (relaxation.py:647-659).  work = 3n values: [res | h0 | h1].
// Horner steps are SpMVs with a fused c*res + A h epilogue; the last one also folds x += h.
int poly_apply(pamg_matrix_s *A, void *x, const void *b, void *work, const double *coeffs, int nc,
               int its, int x_is_zero, hipStream_t s)
{
    if (!A || A->nrows != A->ncols || nc < 1 || !coeffs) return PAMG_E_ARG;
    const int64_t n = A->nrows;
    if (n == 0) return PAMG_OK;
    const size_t ts = tsize(A->dtype);
    void *res_buf = work, *h0 = (char *)work + n * ts, *h1 = (char *)work + 2 * n * ts;
    for (int it = 0; it < its; ++it) {
        const void *res = b;
        bool have_h = false;
        if (!(x_is_zero && it == 0)) {
            // r = b - A x; with more than one coefficient the same launch writes h = c0 * r (epilogue of EPI_RESID, pamg_kernels.h: row_finish)
            PAMG_TRY(stream_launch(A, EPI_RESID, x, b, res_buf, nc > 1 ? coeffs[0] : 0.0, 0.0, nc > 1 ? (double *)h0 : nullptr, s));
            res = res_buf;
            have_h = nc > 1;
        }
        if (nc == 1) {
            PAMG_TRY(vec_axpy(A->dtype, n, coeffs[0], res, x, s));          // x += c0*res
            continue;
        }
        if (!have_h) PAMG_TRY(vec_scale(A->dtype, n, coeffs[0], res, h0, s));            // h = c0*res
        void *hc = h0, *hn = h1;
        for (int k = 1; k < nc - 1; ++k) {                                  // h = c*res + A h
            PAMG_TRY(stream_launch(A, EPI_AXPBY, hc, res, hn, coeffs[k], 0.0, nullptr, s));
            std::swap(hc, hn);
        }
        PAMG_TRY(stream_launch(A, EPI_ACC_AXPBY, hc, res, x, coeffs[nc - 1], 0.0, nullptr, s));
    }
    return PAMG_OK;
}

}  // namespace

// The tail of the hierarchy as one dense operator (pamg_solver_dense_tail).  A cycle enters every level below the finest with x = 0, and smoothers,
// transfers and the tabulated coarsest solve are linear and stationary: everything from the tail level t down is x_t = M b_t with one constant
// n_t x n_t matrix per kind of sub-cycle (key: the cycle type and cycles per level the recursion reaches level t with; 0 where t is the coarsest
// level).  M is tabulated column by column with the launches the cycle runs, outside any graph capture, and checked against them once.
enum { TAIL_OFF = 1, TAIL_NO_LEVEL, TAIL_AMLI, TAIL_SMOOTHER, TAIL_COARSE_HOST, TAIL_ORDER_EXACT, TAIL_DIST, TAIL_TIMEOUT, TAIL_GUARD, TAIL_FALLBACK };
struct DenseTail {
    int mode = 0;                         // 0 automatic, 1 off, 2 forced: the first level within max_rows
    int max_rows = DENSE_TAIL_MAX_ROWS;
    int level = -1;                       // t (chosen at finalize), -1 = none
    int declined = 0;                     // TAIL_* of the last decline, 0 = none
    bool dist = false;                    // the solver runs as the collapsed part of a sharded cycle: never
    bool active = false;                  // the cycle being enqueued uses the operators (set per run_cycle)
    std::map<int, void *> ops;            // key -> M (device, row-major, the solver's dtype)
    size_t bytes = 0;
    double tab_ms = 0.0, guard = 0.0;     // tabulation time of all operators; the largest plan-time guard figure
    long long applications = 0;           // launches enqueued (a captured cycle counts once, its replays do not: as the sweep counters)
};

struct pamg_solver_s {
    DenseTail tail;
    int dtype = PAMG_F64;
    std::vector<Level> levels;
    void *d_coarse = nullptr;     // dense coarse operator (row-major n_c x n_c)
    int n_c = 0;
    bool coarse_set = false, coarse_zero = false, coarse_relax = false;
    pamg_coarse_host_fn coarse_host = nullptr;   // coarsest solve on the HOST by the caller's own function (multilevel.py:752-762,786-788)
    void *coarse_host_user = nullptr;
    std::vector<unsigned char> coarse_hb, coarse_hx;
    bool finalized = false;
    bool use_graph = true;
    hipStream_t own_stream = nullptr;
    double *d_norms = nullptr;    // [norms_cap] per-iteration ||r||^2 + 2 aux slots
    int norms_cap = 0;
    double *d_slot = nullptr;     // 4 doubles: [0] current ||r||^2, [1] ||b||^2
    double *d_scratch = nullptr;  // 1032 doubles for vector reductions
    void *cg_r = nullptr, *cg_z = nullptr, *cg_p = nullptr, *cg_q = nullptr;   // device PCG work vectors
    void *kr_v[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // BiCGStab / CR / SD / MR work vectors (allocated on first use)
    double *kr_red = nullptr;     // KR_PARTIALS inner-product partials + 16 scalar slots of those accelerators
    std::map<int, hipGraphExec_t> graphs;   // key = cycle*1024 + cycles_per_level
    bool host_sync = false;       // a Krylov smoother / coarse solver reads scalars back inside the cycle: no graph capture
    int fallbacks = 0;            // times a persistent sweep timed out and the solver switched to per-level launches
    size_t bytes = 0;
};

namespace {

int krylov_smooth(pamg_solver_s *S, Level &L, const Smoother &sm, hipStream_t s);

int apply_smoother(pamg_solver_s *S, Level &L, const Smoother &sm, bool x_zero, hipStream_t s)
{
    switch (sm.kind) {
        case PAMG_SMOOTH_NONE: return PAMG_OK;
        case PAMG_SMOOTH_JACOBI: return jacobi_pp(L.A, &L.x, &L.xalt, L.b, sm.omega, sm.iterations, s);
        // (L.r is dead while a smoother runs: cycle_rec recomputes it before every restriction)
        case PAMG_SMOOTH_GS: return gs_apply(L.A, L.x, L.b, sm.sweep, 1.0, sm.iterations, s, x_zero, L.r);
        case PAMG_SMOOTH_SOR: return gs_apply(L.A, L.x, L.b, sm.sweep, sm.omega, sm.iterations, s, x_zero, L.r);
        case PAMG_SMOOTH_POLY:
            return poly_apply(L.A, L.x, L.b, L.work, sm.coeffs.data(), (int)sm.coeffs.size(),
                              sm.iterations, x_zero ? 1 : 0, s);
        case PAMG_SMOOTH_BLOCK_JACOBI:
            return block_jacobi_pp(L.A, &L.x, &L.xalt, L.b, sm.d_Dinv, sm.omega, sm.iterations, s);
        case PAMG_SMOOTH_BLOCK_GS:
            return block_gs_apply(L.A, L.x, L.b, sm.d_Dinv, sm.sweep, sm.iterations, s);
        case PAMG_SMOOTH_GS_NE: {
            const int n = (int)L.A->nrows;
            for (int it = 0; it < sm.iterations; ++it) {
                pamg_matrix_s *Ak = sm.Ar ? sm.Ar : L.A;
                if (sm.sweep != PAMG_BACKWARD) PAMG_TRY(kaczmarz_sweep(Ak, false, L.x, L.b, sm.d_Dinv, sm.omega, 0, n, 1, nullptr, s));
                if (sm.sweep != PAMG_FORWARD) PAMG_TRY(kaczmarz_sweep(Ak, false, L.x, L.b, sm.d_Dinv, sm.omega, n - 1, -1, -1, nullptr, s));
            }
            return PAMG_OK;
        }
        case PAMG_SMOOTH_GS_NR: {
            // relaxation.py:968-988: the residual is formed once per DIRECTIONAL call (symmetric = forward call
            // then backward call per iteration, each with iterations = 1), then swept `iterations` times
            const int n = (int)L.A->nrows;
            auto call = [&](bool fwd, int its) -> int {
                PAMG_TRY(stream_launch(sm.Ar ? sm.Ar : L.A, EPI_RESID, L.x, L.b, L.r, 0.0, 0.0, nullptr, s));
                for (int k = 0; k < its; ++k)
                    PAMG_TRY(kaczmarz_sweep(sm.At, true, L.r, nullptr, sm.d_Dinv, sm.omega, fwd ? 0 : n - 1, fwd ? n : -1, fwd ? 1 : -1, L.x, s));
                return PAMG_OK;
            };
            if (sm.sweep == PAMG_SYMMETRIC) {
                for (int it = 0; it < sm.iterations; ++it) { PAMG_TRY(call(true, 1)); PAMG_TRY(call(false, 1)); }
                return PAMG_OK;
            }
            return call(sm.sweep == PAMG_FORWARD, sm.iterations);
        }
        case PAMG_SMOOTH_JACOBI_NE:
            for (int it = 0; it < sm.iterations; ++it) {
                PAMG_TRY(stream_launch(sm.Ar ? sm.Ar : L.A, EPI_RESID, L.x, L.b, L.r, 0.0, 0.0, nullptr, s));   // r = b - A x
                PAMG_TRY(vec_mul(S->dtype, L.n, L.r, sm.d_Dinv, L.r, s));                           // delta = r .* Dinv
                PAMG_TRY(stream_launch(sm.At, EPI_ACC, L.r, nullptr, L.x, 0.0, 0.0, nullptr, s));   // x += (omega A)^T delta
            }
            return PAMG_OK;
        case PAMG_SMOOTH_CF_JACOBI:
        case PAMG_SMOOTH_FC_JACOBI:
            for (int it = 0; it < sm.iterations; ++it) {
                const bool f_first = sm.kind == PAMG_SMOOTH_FC_JACOBI;
                for (int half = 0; half < 2; ++half) {
                    const bool f = (half == 0) == f_first;
                    pamg_matrix_s *sub = f ? sm.AF : sm.AC;
                    void *w = f ? sm.wF : sm.wC;
                    const int reps = f ? sm.f_iterations : sm.c_iterations;
                    for (int k = 0; k < reps; ++k) PAMG_TRY(jacobi_indexed(sub, L.x, L.b, sm.omega, w, s));
                }
            }
            return PAMG_OK;
        case PAMG_SMOOTH_KRYLOV: return krylov_smooth(S, L, sm, s);
        case PAMG_SMOOTH_SCHWARZ: {
            // relaxation.py:240-262: forward / backward sweeps over the subdomains; symmetric = forward then backward per iteration
            int nsub = 0;
            { int64_t info[4]; PAMG_TRY(pamg_schwarz_info(sm.sw, info)); nsub = (int)info[0]; }
            for (int it = 0; it < sm.iterations; ++it) {
                if (sm.sweep != PAMG_BACKWARD) PAMG_TRY(schwarz_sweep(sm.sw, L.x, L.b, 0, nsub, 1, s));
                if (sm.sweep != PAMG_FORWARD) PAMG_TRY(schwarz_sweep(sm.sw, L.x, L.b, nsub - 1, -1, -1, s));
            }
            return PAMG_OK;
        }
        case PAMG_SMOOTH_CF_BLOCK_JACOBI:
        case PAMG_SMOOTH_FC_BLOCK_JACOBI:
            // relaxation.py:1271-1340 / :1342-1411: amg_core::block_jacobi_indexed (relaxation.h:1129-1199) on the C then the
            // F block rows (or F then C).  One full block-Jacobi step from the old iterate into the partner buffer -- the
            // per-row arithmetic of block_jacobi_indexed IS block_jacobi's -- then only the listed rows are taken over.
            for (int it = 0; it < sm.iterations; ++it) {
                const bool f_first = sm.kind == PAMG_SMOOTH_FC_BLOCK_JACOBI;
                for (int half = 0; half < 2; ++half) {
                    const bool f = (half == 0) == f_first;
                    const int reps = f ? sm.f_iterations : sm.c_iterations;
                    for (int k = 0; k < reps; ++k) {
                        PAMG_TRY(block_jacobi_step(L.A, BLK_JACOBI, sm.d_Dinv, L.x, L.xalt, L.b, sm.omega, s));
                        PAMG_TRY(vec_copy_indexed(S->dtype, f ? sm.nF : sm.nC, f ? sm.iF : sm.iC, L.xalt, L.x, s));
                    }
                }
            }
            return PAMG_OK;
    }
    (void)S;
    return PAMG_E_ARG;
}

void drop_graphs(pamg_solver_s *S);
int prebuild_schedules(Level &L, const Smoother &sm, bool zero = false);

// after a synchronising entry point: did any persistent sweep give up waiting?
int check_sweeps(pamg_solver_s *S)
{
    bool any = false;
    for (Level &L : S->levels) {
        if (!L.A) continue;
        bool e = false;
        PAMG_TRY(sweep_error(L.A, &e));
        any = any || e;
        // the Kaczmarz lane sweeps (pamg_kz.hip) run on the smoothers' own operators: A^T for gauss_seidel_nr, the row-sorted twin for
        // gauss_seidel_ne -- their spin time-outs are reported on THOSE operators' line schedules
        for (Smoother *sm : {&L.pre, &L.post}) {
            for (pamg_matrix_s *M : {sm->At, sm->Ar})
                if (M && M != L.A) {
                    bool e2 = false;
                    PAMG_TRY(sweep_error(M, &e2));
                    any = any || e2;
                }
            if (sm->sw) {                                     // the persistent Schwarz sweep (pamg_schwarz.hip)
                bool e3 = false;
                PAMG_TRY(schwarz_error(sm->sw, &e3));
                any = any || e3;
            }
        }
    }
    static int forced = [] { const char *e = getenv("PAMG_FORCE_TIMEOUT"); return e ? atoi(e) : 0; }();   // test hook: report the first N checks as timed out
    if (forced > 0) { --forced; any = true; }
    return any ? PAMG_E_TIMEOUT : PAMG_OK;
}

// A persistent sweep gave up waiting (PAMG_E_TIMEOUT): its workgroups were not all running -- another process on the
// device, a debugger, a tiny partition.  From then on this solver runs every order-exact sweep as one launch per
// dependency level (scheduler mode 1: no workgroup ever waits for another), slower and always live.  The captured graphs
// point at the persistent kernels and are dropped; level-permuted copies are built where only tile plans existed.
int fall_back_to_level_launches(pamg_solver_s *S)
{
    hipDeviceSynchronize();
    drop_graphs(S);
    for (Level &L : S->levels) {
        if (!L.A) continue;
        L.A->gs_mode = 1;
        L.A->tile_default = 0;
        PAMG_TRY(sym_reset(L.A));                             // (the fused symmetric sweep declines from here on: gs_mode 1)
        matrix_drop_zero_plans(L.A);                          // (so do the zero-iterate plans: every sweep takes the general path)
        matrix_drop_dtri(L.A);                                // (and the dense form, which asks for scheduler mode 0)
        for (Smoother *sm : {&L.pre, &L.post}) {
            // kz_lane_launch is gated on gs_mode == 0 of the operator the sweep runs on (pamg_matrix.hip: kaczmarz_sweep)
            if (sm->At) sm->At->gs_mode = 1;
            if (sm->Ar) sm->Ar->gs_mode = 1;
            if (sm->sw) schwarz_level_launches(sm->sw);
            PAMG_TRY(prebuild_schedules(L, *sm));
        }
    }
    S->fallbacks++;
    return PAMG_OK;
}

int coarse_solve(pamg_solver_s *S, const void *b, void *x, hipStream_t s)
{
    if (S->coarse_relax) {
        // multilevel.py:765-782: x = zeros_like(b); relax(A, x, b).  Always called on the coarsest level's own buffers.
        Level &L = S->levels.back();
        if (b != L.b || x != L.x) return PAMG_E_STATE;
        PAMG_HIP(hipMemsetAsync(L.x, 0, (size_t)L.n * tsize(S->dtype), s));
        PAMG_TRY(apply_smoother(S, L, L.pre, true, s));
        if (L.x != L.x_home) {
            PAMG_HIP(hipMemcpyAsync(L.x_home, L.x, (size_t)L.n * tsize(S->dtype), hipMemcpyDeviceToDevice, s));
            std::swap(L.x, L.xalt);
        }
        return PAMG_OK;
    }
    if (S->coarse_zero) return (int)hipMemsetAsync(x, 0, (size_t)S->n_c * tsize(S->dtype), s);
    if (S->coarse_host) {
        // the coarse right-hand side (a few hundred values at most) goes down, the caller's solver runs, the answer comes back
        const size_t vb = (size_t)S->n_c * tsize(S->dtype);
        PAMG_HIP(hipMemcpyAsync(S->coarse_hb.data(), b, vb, hipMemcpyDeviceToHost, s));
        PAMG_HIP(hipStreamSynchronize(s));
        if (S->coarse_host(S->coarse_host_user, S->coarse_hb.data(), S->coarse_hx.data(), (int64_t)S->n_c) != 0) return PAMG_E_STATE;
        PAMG_HIP(hipMemcpyAsync(x, S->coarse_hx.data(), vb, hipMemcpyHostToDevice, s));
        PAMG_HIP(hipStreamSynchronize(s));                     // the host buffer is reused by the next cycle
        return PAMG_OK;
    }
    return dense_gemv(S->dtype, S->n_c, S->d_coarse, b, x, s);
}

// ---- the dense tail: which operator a visit of level t takes
int tail_key(const pamg_solver_s *S, int t, int type, int cpl)
{
    if (t == (int)S->levels.size() - 1) return 0;                 // the coarsest solve: the same map under every cycle
    return 1 + type * 1024 + (type == PAMG_CYCLE_V ? 1 : cpl);
}

const void *tail_op(const pamg_solver_s *S, int lvl, int type, int cpl)
{
    const DenseTail &T = S->tail;
    if (!T.active || lvl != T.level) return nullptr;
    auto it = T.ops.find(tail_key(S, lvl, type, cpl));
    return it == T.ops.end() ? nullptr : it->second;
}

// multilevel.py:584-662
int cycle_rec(pamg_solver_s *S, int lvl, int type, int cpl, bool x_zero, hipStream_t s)
{
    Level &L = S->levels[lvl];
    Level &N = S->levels[lvl + 1];
    const int nlev = (int)S->levels.size();
    const size_t ts = tsize(S->dtype);
    PAMG_TRY(apply_smoother(S, L, L.pre, x_zero, s));
    PAMG_TRY(stream_launch(L.A, EPI_RESID, L.x, L.b, L.r, 0.0, 0.0, nullptr, s));      // r = b - A x
    // b_c = R r and x_c = 0 in one launch (multilevel.py:613-615)
    PAMG_TRY(stream_launch(L.R, EPI_SET, L.r, nullptr, N.b, 0.0, 0.0, reinterpret_cast<double *>(N.x), s));
    // the visit of level lvl + 1: the recursion (the coarsest solve on the last level), or -- where the dense tail starts there and holds the
    // operator of this kind of visit -- one launch: from zero x = M b; a second visit of a W / F cycle r = b - A x, x += M r (exact for a
    // stationary linear cycle)
    auto down = [&](int ty, int c, bool xz) -> int {
        const void *M = tail_op(S, lvl + 1, ty, c);
        if (!M) return lvl == nlev - 2 ? coarse_solve(S, N.b, N.x, s) : cycle_rec(S, lvl + 1, ty, c, xz, s);
        if (!xz) PAMG_TRY(stream_launch(N.A, EPI_RESID, N.x, N.b, N.r, 0.0, 0.0, nullptr, s));
        PAMG_TRY(dense_tail_apply(S->dtype, (int)N.n, M, xz ? N.b : N.r, N.x, !xz, s));
        S->tail.applications++;
        return PAMG_OK;
    };
    if (lvl == nlev - 2) {
        PAMG_TRY(down(type, cpl, true));
    } else if (type == PAMG_CYCLE_V) {
        PAMG_TRY(down(PAMG_CYCLE_V, 1, true));
    } else if (type == PAMG_CYCLE_W) {
        PAMG_TRY(down(PAMG_CYCLE_W, cpl, true));
        PAMG_TRY(down(PAMG_CYCLE_W, cpl, false));
    } else if (type == PAMG_CYCLE_F) {
        PAMG_TRY(down(PAMG_CYCLE_F, cpl, true));
        for (int k = 0; k < cpl; ++k) PAMG_TRY(down(PAMG_CYCLE_V, 1, false));
    } else if (type == PAMG_CYCLE_AMLI) {
        // multilevel.py:628-656: two inner corrections, each a recursive AMLI solve from an
        // initial guess of ones, A-orthogonalised against the previous one and line-searched.
        // Step sizes stay on the device (slot[8..11]) so the cycle remains capturable.
        if (!N.amli) return PAMG_E_STATE;
        const int64_t nc = N.n;
        const int dt = S->dtype;
        void *p[2] = {N.amli, (char *)N.amli + nc * ts};
        void *q = (char *)N.amli + 2 * nc * ts, *acc = (char *)N.amli + 3 * nc * ts;
        double *sl = S->d_slot + 8;
        PAMG_HIP(hipMemsetAsync(acc, 0, (size_t)nc * ts, s));
        for (int k = 0; k < 2; ++k) {
            PAMG_TRY(vec_fill(dt, nc, 1.0, N.x, s));                                     // p[k,:] = 1
            PAMG_TRY(cycle_rec(S, lvl + 1, PAMG_CYCLE_AMLI, cpl, false, s));
            PAMG_HIP(hipMemcpyAsync(p[k], N.x, (size_t)nc * ts, hipMemcpyDeviceToDevice, s));
            for (int j = 0; j < k; ++j) {
                PAMG_TRY(stream_launch(N.A, EPI_SET, p[k], nullptr, q, 0.0, 0.0, nullptr, s));
                PAMG_TRY(vec_dot(dt, nc, p[j], q, S->d_scratch, sl + 0, s));              // <p_j, Ac p_k>
                PAMG_TRY(stream_launch(N.A, EPI_SET, p[j], nullptr, q, 0.0, 0.0, nullptr, s));
                PAMG_TRY(vec_dot(dt, nc, p[j], q, S->d_scratch, sl + 1, s));              // <p_j, Ac p_j>
                PAMG_TRY(vec_axpy_ratio(dt, nc, sl + 0, sl + 1, -1.0, p[j], p[k], s));    // p_k -= beta p_j
            }
            PAMG_TRY(stream_launch(N.A, EPI_SET, p[k], nullptr, q, 0.0, 0.0, nullptr, s));    // Ap
            PAMG_TRY(vec_dot(dt, nc, p[k], N.b, S->d_scratch, sl + 2, s));
            PAMG_TRY(vec_dot(dt, nc, p[k], q, S->d_scratch, sl + 3, s));
            PAMG_TRY(vec_axpy_ratio(dt, nc, sl + 2, sl + 3, 1.0, p[k], acc, s));          // coarse_x += alpha p
            PAMG_TRY(vec_axpy_ratio(dt, nc, sl + 2, sl + 3, -1.0, q, N.b, s));            // coarse_b -= alpha Ap
        }
        PAMG_HIP(hipMemcpyAsync(N.x, acc, (size_t)nc * ts, hipMemcpyDeviceToDevice, s));
    } else {
        return PAMG_E_ARG;
    }
    PAMG_TRY(stream_launch(L.P, EPI_ACC, N.x, nullptr, L.x, 0.0, 0.0, nullptr, s));     // x += P x_c
    PAMG_TRY(apply_smoother(S, L, L.post, false, s));
    if (L.x != L.x_home) {          // odd number of ping-pong swaps: bring the iterate home
        PAMG_HIP(hipMemcpyAsync(L.x_home, L.x, (size_t)L.n * ts, hipMemcpyDeviceToDevice, s));
        std::swap(L.x, L.xalt);
    }
    return PAMG_OK;
}

// one full cycle on the internal level-0 buffers, optionally followed by ||b - A x||^2 -> d_slot[0]
int enqueue_cycle(pamg_solver_s *S, int type, int cpl, bool check, bool x_zero, hipStream_t s)
{
    Level &L0 = S->levels[0];
    if (S->levels.size() == 1) {
        PAMG_TRY(coarse_solve(S, L0.b, L0.x, s));                  // multilevel.py:559-561
    } else {
        PAMG_TRY(cycle_rec(S, 0, type, cpl, x_zero, s));
    }
    if (!check) return PAMG_OK;
    PAMG_TRY(stream_launch(L0.A, EPI_SUMSQ, L0.x, L0.b, nullptr, 0.0, 0.0, L0.A->d_partial, s));
    return reduce_partials(L0.A->d_partial, L0.A->nblk, S->d_slot, s);
}

// ---- the dense tail: level choice, tabulation, guard
void tail_free(pamg_solver_s *S)
{
    DenseTail &T = S->tail;
    for (auto &kv : T.ops) hipFree(kv.second);
    T.ops.clear();
    S->bytes -= std::min(S->bytes, T.bytes);
    T.bytes = 0;
    T.active = false;
}

// graphs captured earlier may hold launches that read the operators: they go first
void tail_decline(pamg_solver_s *S, int why)
{
    if (!S->tail.ops.empty() || !S->graphs.empty()) { hipDeviceSynchronize(); drop_graphs(S); }
    tail_free(S);
    S->tail.level = -1;
    S->tail.declined = why;
}

// what of the rule is known when the solver is finalized (or the mode changes): the level and the smoothers below it.
// Automatic: the first level of at most max_rows rows whose parent has more than TAIL_PARENT_MIN_ROWS rows; forced (mode 2): the first level below the
// finest within max_rows.  Why the parent's size: an operator costs n_t sub-cycles of the tail to tabulate and saves a fraction of one per cycle, so it
// pays back after some n_t cycles of that kind -- the automatic form is for hierarchies whose set-up already costs seconds (a parent of more than
// 4 x ONE_XCD_MAX_ROWS rows sits under fine levels of millions of rows) and leaves every smaller hierarchy's launches, level by level, as they are.
constexpr int64_t TAIL_PARENT_MIN_ROWS = 4 * ONE_XCD_MAX_ROWS;
void tail_choose(pamg_solver_s *S)
{
    DenseTail &T = S->tail;
    tail_decline(S, 0);
    if (T.mode == 1) { T.declined = TAIL_OFF; return; }
    if (T.dist) { T.declined = TAIL_DIST; return; }
    const int nlev = (int)S->levels.size();
    const int64_t lim = std::min<int64_t>(T.max_rows, DENSE_TAIL_HARD_MAX_ROWS);
    int t = -1;
    for (int l = 1; l < nlev && t < 0; ++l)
        if (S->levels[l].n >= 1 && S->levels[l].n <= lim && (T.mode == 2 || S->levels[l - 1].n > TAIL_PARENT_MIN_ROWS)) t = l;
    if (t < 0) { T.declined = TAIL_NO_LEVEL; return; }
    if (S->coarse_host) { T.declined = TAIL_COARSE_HOST; return; }
    if (S->fallbacks) { T.declined = TAIL_FALLBACK; return; }
    for (int l = t; l < nlev; ++l) {
        const Level &L = S->levels[l];
        if (l == nlev - 1 && !S->coarse_relax) break;
        for (const Smoother *sm : {&L.pre, &L.post}) {
            if (l == nlev - 1 && sm == &L.post) break;            // the coarsest level relaxes with its first slot only
            if (sm->kind == PAMG_SMOOTH_KRYLOV) { T.declined = TAIL_SMOOTHER; return; }
            const bool gs = sm->kind == PAMG_SMOOTH_GS || sm->kind == PAMG_SMOOTH_SOR || sm->kind == PAMG_SMOOTH_BLOCK_GS ||
                            sm->kind == PAMG_SMOOTH_GS_NE || sm->kind == PAMG_SMOOTH_GS_NR;
            // the order-exact mode keeps the reference's bits, and therefore its launches
            if (gs && L.A->gs_order != 1) { T.declined = TAIL_ORDER_EXACT; return; }
        }
    }
    T.level = t;
}

// the launches the operator replaces: the sub-cycle of level t from x_t = 0 on the level's own vectors
int tail_subcycle(pamg_solver_s *S, int t, int type, int cpl, hipStream_t s)
{
    Level &L = S->levels[t];
    PAMG_HIP(hipMemsetAsync(L.x, 0, (size_t)L.n * tsize(S->dtype), s));
    if (t == (int)S->levels.size() - 1) return coarse_solve(S, L.b, L.x, s);
    return cycle_rec(S, t, type, cpl, true, s);
}

// M of one key: column j = the sub-cycle's answer to b_t = e_j, then one seeded random b_t through both.  *why: 0 = built, else TAIL_*
int tail_build(pamg_solver_s *S, int type, int cpl, hipStream_t s, void **out, int *why)
{
    DenseTail &T = S->tail;
    const int t = T.level, dt = S->dtype;
    Level &L = S->levels[t];
    const int n = (int)L.n;
    const size_t ts = tsize(dt), vb = (size_t)n * ts;
    *out = nullptr; *why = 0;
    const auto t0 = std::chrono::steady_clock::now();
    void *Mt = nullptr, *M = nullptr;
    PAMG_HIP(hipMalloc(&Mt, std::max<size_t>(vb * n, 256)));
    const bool was_active = T.active;
    T.active = false;                                            // (the launches, whatever else is built already)
    int st = PAMG_OK;
    for (int j = 0; j < n && st == PAMG_OK; ++j) {
        st = (int)hipMemsetAsync(L.b, 0, vb, s);
        if (st == PAMG_OK) st = vec_fill(dt, 1, 1.0, (char *)L.b + (size_t)j * ts, s);
        if (st == PAMG_OK) st = tail_subcycle(S, t, type, cpl, s);
        if (st == PAMG_OK) st = (int)hipMemcpyAsync((char *)Mt + (size_t)j * vb, L.x, vb, hipMemcpyDeviceToDevice, s);
    }
    // (no dalloc: its clearing memset runs on the null stream, which this stream does not wait for; the transposition writes every entry)
    const size_t mbytes = std::max<size_t>(vb * n, 256);
    if (st == PAMG_OK) st = (int)hipMalloc(&M, mbytes);
    if (st == PAMG_OK) st = dense_transpose(dt, n, Mt, M, s);
    // the guard: the launched sub-cycle against M b_t for one seeded random b_t, relative max norm
    std::vector<double> hb((size_t)n), hx((size_t)n), hm((size_t)n);
    std::vector<float> fb, fx, fm;
    unsigned long long lcg = 0x9E3779B97F4A7C15ull;
    for (int i = 0; i < n; ++i) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        hb[i] = (double)(lcg >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
    }
    const void *src = hb.data();
    if (dt == PAMG_F32) { fb.assign(hb.begin(), hb.end()); fx.resize(n); fm.resize(n); src = fb.data(); }
    void *dst_x = dt == PAMG_F32 ? (void *)fx.data() : (void *)hx.data(), *dst_m = dt == PAMG_F32 ? (void *)fm.data() : (void *)hm.data();
    if (st == PAMG_OK) st = (int)hipMemcpyAsync(L.b, src, vb, hipMemcpyHostToDevice, s);
    if (st == PAMG_OK) st = tail_subcycle(S, t, type, cpl, s);
    if (st == PAMG_OK) st = (int)hipMemcpyAsync(dst_x, L.x, vb, hipMemcpyDeviceToHost, s);
    if (st == PAMG_OK) st = dense_tail_apply(dt, n, M, L.b, L.x, false, s);
    if (st == PAMG_OK) st = (int)hipMemcpyAsync(dst_m, L.x, vb, hipMemcpyDeviceToHost, s);
    if (st == PAMG_OK) st = (int)hipStreamSynchronize(s);
    T.active = was_active;
    hipFree(Mt);
    auto give_up = [&](int reason) { if (M) hipFree(M); *why = reason; };
    if (st != PAMG_OK) { give_up(0); return st; }
    // a sweep that timed out left garbage in a column: the solver switches schedulers as after a solve, the form is declined
    const int swept = check_sweeps(S);
    if (swept == PAMG_E_TIMEOUT) {
        give_up(TAIL_TIMEOUT);
        if (S->fallbacks == 0) PAMG_TRY(fall_back_to_level_launches(S));
        return PAMG_OK;
    }
    if (swept != PAMG_OK) { give_up(0); return swept; }
    if (dt == PAMG_F32) for (int i = 0; i < n; ++i) { hx[i] = fx[i]; hm[i] = fm[i]; }
    double dmax = 0.0, xmax = 0.0;
    bool finite = true;
    for (int i = 0; i < n; ++i) {
        finite = finite && std::isfinite(hx[i]) && std::isfinite(hm[i]);
        dmax = std::max(dmax, std::fabs(hx[i] - hm[i]));
        xmax = std::max(xmax, std::fabs(hx[i]));
    }
    const double fig = !finite ? INFINITY : xmax > 0.0 ? dmax / xmax : (dmax > 0.0 ? INFINITY : 0.0);
    T.guard = std::max(T.guard, fig);
    // the project's form-against-form bar: 1e-13 in f64 (as the dense block-triangular and merged forms), the same multiple of the unit round-off in f32
    const double bar = dt == PAMG_F64 ? 1e-13 : 1e-13 * ((double)FLT_EPSILON / DBL_EPSILON);
    if (!(fig <= bar)) { give_up(TAIL_GUARD); return PAMG_OK; }
    T.bytes += mbytes;
    S->bytes += mbytes;
    if (getenv("PAMG_TIMING"))
        fprintf(stderr, "[pamg timing] dense tail: level %d, %d rows, cycle type %d: tabulated in %.1f ms, guard %.2e, %zu bytes\n", t, n, type,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), fig, mbytes);
    T.tab_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = M;
    return PAMG_OK;
}

// before a cycle of (type, cpl) is enqueued or captured: build what it needs (never inside a capture) and say whether this cycle uses the form
int ensure_tail(pamg_solver_s *S, int type, int cpl, hipStream_t s)
{
    DenseTail &T = S->tail;
    T.active = false;
    if (T.level < 0) return PAMG_OK;
    if (T.dist) { tail_decline(S, TAIL_DIST); return PAMG_OK; }
    if (type == PAMG_CYCLE_AMLI) {                                 // not linear in b: this cycle keeps its launches
        if (T.ops.empty()) T.declined = TAIL_AMLI;
        return PAMG_OK;
    }
    if (S->fallbacks) { tail_decline(S, TAIL_FALLBACK); return PAMG_OK; }
    // an F cycle reaches level t as an F cycle first and as V cycles afterwards
    const int kinds[2][2] = {{type, cpl}, {PAMG_CYCLE_V, 1}};
    const int nk = (type == PAMG_CYCLE_F && T.level < (int)S->levels.size() - 1) ? 2 : 1;
    for (int k = 0; k < nk; ++k) {
        const int key = tail_key(S, T.level, kinds[k][0], kinds[k][1]);
        if (T.ops.count(key)) continue;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        PAMG_HIP(hipStreamIsCapturing(s, &cs));
        if (cs != hipStreamCaptureStatusNone) return PAMG_OK;      // somebody else's capture: this cycle runs its launches
        void *M = nullptr;
        int why = 0;
        PAMG_TRY(tail_build(S, kinds[k][0], kinds[k][1], s, &M, &why));
        if (!M) { tail_decline(S, why); return PAMG_OK; }
        T.ops[key] = M;
    }
    T.active = true;
    T.declined = 0;
    return PAMG_OK;
}

int run_cycle(pamg_solver_s *S, int type, int cpl, hipStream_t s, bool check = true, bool x_zero = false)
{
    PAMG_TRY(ensure_tail(S, type, cpl, s));
    if (!S->use_graph || S->host_sync) return enqueue_cycle(S, type, cpl, check, x_zero, s);
    const int key = ((type * 1024 + cpl) * 2 + (check ? 1 : 0)) * 2 + (x_zero ? 1 : 0);
    auto it = S->graphs.find(key);
    if (it == S->graphs.end()) {
        hipGraph_t g = nullptr;
        PAMG_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        const int st = enqueue_cycle(S, type, cpl, check, x_zero, s);
        const hipError_t e = hipStreamEndCapture(s, &g);
        if (st != PAMG_OK) { if (g) hipGraphDestroy(g); return st; }
        if (e != hipSuccess) return (int)e;
        hipGraphExec_t ex = nullptr;
        PAMG_HIP(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
        hipGraphDestroy(g);
        it = S->graphs.emplace(key, ex).first;
    }
    return (int)hipGraphLaunch(it->second, s);
}

int ensure_amli(pamg_solver_s *S, int cycle);

// SOR's relaxation parameter takes effect on this operator (gs_apply): the CSR flavour, a one-directional sweep, omega != 1 -- the
// reference's quirks make every other "SOR" a plain Gauss-Seidel sweep
static bool sor_takes_omega(const pamg_matrix_s *A, const Smoother &sm)
{
    return sm.kind == PAMG_SMOOTH_SOR && A->R == 1 && A->flavour != PAMG_BSR && sm.sweep != PAMG_SYMMETRIC && sm.omega != 1.0;
}

// Zero-iterate plans (PAMG_TUNE_ZERO_PLANS) for the pre-smoother of level l: a cycle enters every level below the finest with x = 0 (cycle_rec), so a
// symmetric Gauss-Seidel pre-smoother there sweeps half the operator per direction.  The finest level only on request (key = 2): its pre-smoother
// starts from zero in the preconditioning cycles alone.
static bool zero_plans_wanted(const pamg_matrix_s *A, const Smoother &pre, const Smoother &post, int l)
{
    if (A->zero_plans == 1 || (l == 0 && A->zero_plans != 2)) return false;
    if (pre.kind != PAMG_SMOOTH_GS || pre.sweep != PAMG_SYMMETRIC || pre.iterations < 1) return false;
    if (sor_takes_omega(A, post)) return false;              // the operator keeps the unmerged layout
    return A->R == 1 && A->dtype == PAMG_F64 && A->gs_order == 1 && A->gs_mode == 0 && A->nrows >= 2;
}

// The solver's side of the dense block-triangular form (pamg_matrix_dense_tri).  dtri_sweeps: a smoother of the level is symmetric Gauss-Seidel (switched on
// by name, the form is built only where it would run); dtri_automatic: a level below the finest whose pre- and post-smoother both are.  The operator's side
// (mode, size, memory proportion, growth) is dtri_claims / ensure_dtri
static bool dtri_sym_gs(const Smoother &sm) { return sm.kind == PAMG_SMOOTH_GS && sm.sweep == PAMG_SYMMETRIC && sm.iterations >= 1; }
static bool dtri_sweeps(const Smoother &pre, const Smoother &post) { return dtri_sym_gs(pre) || dtri_sym_gs(post); }
static bool dtri_automatic(const Smoother &pre, const Smoother &post, int l) { return l >= 1 && dtri_sym_gs(pre) && dtri_sym_gs(post); }

int prebuild_schedules(Level &L, const Smoother &sm, bool zero)
{
    if (sm.kind == PAMG_SMOOTH_GS_NE || sm.kind == PAMG_SMOOTH_GS_NR) {
        // the Kaczmarz line schedules allocate: build them here, never inside a graph capture
        pamg_matrix_s *Lm = sm.kind == PAMG_SMOOTH_GS_NE ? (sm.Ar ? sm.Ar : L.A) : sm.At;
        const int n = (int)Lm->nrows;
        if (n == 0) return PAMG_OK;
        if (sm.sweep != PAMG_BACKWARD) PAMG_TRY(ensure_line_schedule(Lm, 0, n, 1));
        if (sm.sweep != PAMG_FORWARD) PAMG_TRY(ensure_line_schedule(Lm, n - 1, -1, -1));
        return PAMG_OK;
    }
    const bool gs = sm.kind == PAMG_SMOOTH_GS || sm.kind == PAMG_SMOOTH_SOR || sm.kind == PAMG_SMOOTH_BLOCK_GS;
    if (!gs || L.A->nrows == 0) return PAMG_OK;
    // the merged lane form (pamg_lanem_plan.h) eliminates dependency levels with coefficients that would depend on SOR's relaxation
    // parameter: an operator swept by SOR keeps the unmerged layout (one layout per schedule)
    if (sor_takes_omega(L.A, sm) && L.A->lane_merge == 0) L.A->lane_merge = 1;
    int r0, r1, rs;
    if (sm.sweep == PAMG_FORWARD || sm.sweep == PAMG_SYMMETRIC) {
        PAMG_TRY(sweep_bounds(L.A, PAMG_FORWARD, r0, r1, rs));
        PAMG_TRY(ensure_schedule(L.A, r0, r1, rs, sm.kind == PAMG_SMOOTH_BLOCK_GS));
    }
    if (sm.sweep == PAMG_BACKWARD || sm.sweep == PAMG_SYMMETRIC) {
        PAMG_TRY(sweep_bounds(L.A, PAMG_BACKWARD, r0, r1, rs));
        PAMG_TRY(ensure_schedule(L.A, r0, r1, rs, sm.kind == PAMG_SMOOTH_BLOCK_GS));
    }
    // the fused symmetric sweep's hand-off buffers (allocated here: the first cycle may be a graph capture)
    if (sm.sweep == PAMG_SYMMETRIC && sm.kind != PAMG_SMOOTH_BLOCK_GS) PAMG_TRY(ensure_sym_parts(L.A));
    // the zero-iterate plans (found built where the schedule jobs ran) and their numerator vector: allocations, so here and never inside a capture
    if (zero) PAMG_TRY(ensure_zero_parts(L.A, true));
    return PAMG_OK;
}

// the order-exact schedules of all levels and both directions, built side by side on host threads (dependency analysis,
// tile planning and packing are host work: a 256^3 hierarchy spends seconds there).  Jobs are (operator, sweep bounds);
// duplicates (pre- and post-smoother of a level share theirs) are dropped.
struct SchedJob { pamg_matrix_s *A; int r0, r1, rs; int st; bool block_gs; int zero_dir; };      // zero_dir: 0 / 1 = the job goes on with that zero-iterate plan, -1 = none

// a schedule job's second half: the zero-iterate plan of its direction, on the thread that has just finished the general plan (the plans of the
// other levels and directions are being built beside it)
static int sched_job_run(SchedJob &j)
{
    PAMG_TRY(ensure_schedule(j.A, j.r0, j.r1, j.rs, j.block_gs));
    if (j.zero_dir < 0) return PAMG_OK;
    GsSchedule *g = nullptr;
    PAMG_TRY(get_schedule(j.A, j.r0, j.r1, j.rs, &g));
    if (!g || !g->lanem) return PAMG_OK;
    const int st = build_zero_plan(j.A, j.zero_dir);
    return st == PAMG_E_ARG ? PAMG_OK : st;                  // does not fit the form: the general plans keep the sweep
}

void sched_jobs_of(Level &L, const Smoother &sm, std::vector<SchedJob> &jobs, bool zero = false)
{
    const bool gs = sm.kind == PAMG_SMOOTH_GS || sm.kind == PAMG_SMOOTH_SOR || sm.kind == PAMG_SMOOTH_BLOCK_GS;
    if (!gs || L.A->nrows == 0) return;
    auto add = [&](int dir) {
        int r0, r1, rs;
        if (sweep_bounds(L.A, dir, r0, r1, rs)) return;
        for (const SchedJob &j : jobs) if (j.A == L.A && j.r0 == r0 && j.r1 == r1 && j.rs == rs && j.block_gs == (sm.kind == PAMG_SMOOTH_BLOCK_GS)) return;
        jobs.push_back({L.A, r0, r1, rs, PAMG_OK, sm.kind == PAMG_SMOOTH_BLOCK_GS, zero ? (dir == PAMG_BACKWARD ? 1 : 0) : -1});
    };
    if (sm.sweep == PAMG_FORWARD || sm.sweep == PAMG_SYMMETRIC) add(PAMG_FORWARD);
    if (sm.sweep == PAMG_BACKWARD || sm.sweep == PAMG_SYMMETRIC) add(PAMG_BACKWARD);
}

int run_sched_jobs(std::vector<SchedJob> &jobs)
{
    if (jobs.empty()) return PAMG_OK;
    int dev = 0;
    PAMG_HIP(hipGetDevice(&dev));
    const char *e = getenv("PAMG_SCHED_THREADS");
    const bool serial = (e && *e == '1' && !e[1]) || jobs.size() == 1;
    if (serial) {
        for (SchedJob &j : jobs) PAMG_TRY(sched_job_run(j));
        return PAMG_OK;
    }
    std::vector<std::thread> th;
    for (SchedJob &j : jobs)
        th.emplace_back([&j, dev] {
            j.st = (int)hipSetDevice(dev);
            if (!j.st) j.st = sched_job_run(j);
        });
    for (auto &t : th) t.join();
    for (const SchedJob &j : jobs) if (j.st) return j.st;
    return PAMG_OK;
}

int dalloc(pamg_solver_s *S, void **p, size_t bytes)
{
    PAMG_HIP(hipMalloc(p, std::max<size_t>(bytes, 256)));
    PAMG_HIP(hipMemset(*p, 0, std::max<size_t>(bytes, 256)));
    S->bytes += std::max<size_t>(bytes, 256);
    return PAMG_OK;
}

int ensure_amli(pamg_solver_s *S, int cycle)
{
    if (cycle != PAMG_CYCLE_AMLI) return PAMG_OK;
    for (size_t l = 1; l < S->levels.size(); ++l) {
        Level &L = S->levels[l];
        if (!L.amli) PAMG_TRY(dalloc(S, &L.amli, 4 * (size_t)L.n * tsize(S->dtype)));
    }
    return PAMG_OK;
}

void drop_graphs(pamg_solver_s *S)
{
    for (auto &kv : S->graphs) hipGraphExecDestroy(kv.second);
    S->graphs.clear();
}


// ------------------------------------------------------------------------------------------ Krylov cores
// CG exactly as the reference's krylov/_cg.py:87-200 runs it under criteria='rr': residual recomputed every 8th step,
// curvature checks, stopping rule ||r|| < tol ||b||.  precond = nullptr: M = identity (z IS r, as in the reference where
// the identity operator hands its argument back).  r / z / p / q: n-vectors of work.
int cg_core(pamg_solver_s *S, pamg_matrix_s *Aop, int64_t n, const std::function<int(const void *, void *)> *precond, void *r, void *z,
            void *p, void *q, void *x, const void *b, double tol, int maxiter, double *residuals, int *n_iter, int *info, hipStream_t s)
{
    const int dt = S->dtype;
    const size_t vb = (size_t)n * tsize(dt);
    if (maxiter <= 0) maxiter = (int)(1.3 * (double)n) + 2;                                // _cg.py:93-94
    if (!precond) z = r;
    double *slot = S->d_slot;                    // [0] cycle's norm slot (unused here), [1..3] scalars
    double h[3];
    auto fetch = [&](int k) -> int {             // h[0..k) <- slot[1..1+k)
        PAMG_HIP(hipMemcpyAsync(h, slot + 1, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, s));
        return (int)hipStreamSynchronize(s);
    };
    // setup (_cg.py:98-112)
    PAMG_TRY(stream_launch(Aop, EPI_RESID, x, b, r, 0.0, 0.0, nullptr, s));              // r = b - A x
    if (precond) PAMG_TRY((*precond)(r, z));
    PAMG_HIP(hipMemcpyAsync(p, z, vb, hipMemcpyDeviceToDevice, s));
    PAMG_TRY(vec_dot(dt, n, r, z, S->d_scratch, slot + 1, s));                           // rz
    PAMG_TRY(vec_sumsq(dt, n, r, S->d_scratch, slot + 2, s));                            // ||r||^2
    PAMG_TRY(vec_sumsq(dt, n, b, S->d_scratch, slot + 3, s));                            // ||b||^2
    PAMG_TRY(fetch(3));
    double rz = h[0], normr = std::sqrt(h[1]), normb = std::sqrt(h[2]);
    if (normb == 0.0) normb = 1.0;
    if (residuals) residuals[0] = normr;
    const double rtol = tol * normb;
    int it = 0, inf = -2;
    if (normr < rtol) inf = 0;
    while (inf == -2) {
        PAMG_TRY(stream_launch(Aop, EPI_SET, p, nullptr, q, 0.0, 0.0, nullptr, s));      // Ap
        PAMG_TRY(vec_dot(dt, n, q, p, S->d_scratch, slot + 1, s));                       // pAp
        PAMG_TRY(fetch(1));
        const double pAp = h[0];
        if (pAp < 0.0) { inf = -1; break; }                                              // indefinite A
        const double rz_old = rz, alpha = rz / pAp;
        PAMG_TRY(vec_axpy(dt, n, alpha, p, x, s));                                       // x += alpha p
        if ((it % 8) != 0 && it > 0) PAMG_TRY(vec_axpy(dt, n, -alpha, q, r, s));        // r -= alpha Ap
        else PAMG_TRY(stream_launch(Aop, EPI_RESID, x, b, r, 0.0, 0.0, nullptr, s));     // r = b - A x (every 8th)
        if (precond) PAMG_TRY((*precond)(r, z));
        PAMG_TRY(vec_dot(dt, n, r, z, S->d_scratch, slot + 1, s));
        PAMG_TRY(vec_sumsq(dt, n, r, S->d_scratch, slot + 2, s));
        PAMG_TRY(fetch(2));
        rz = h[0];
        if (rz < 0.0) { inf = -1; break; }                                               // indefinite M
        PAMG_TRY(vec_xpby(dt, n, rz / rz_old, z, p, s));                                 // p = beta p + z
        ++it;
        normr = std::sqrt(h[1]);
        if (residuals) residuals[it] = normr;
        if (normr < rtol) inf = 0;
        else if (it == maxiter) inf = it;
    }
    if (n_iter) *n_iter = it;
    if (info) *info = inf;
    return PAMG_OK;
}

// CGNE (krylov/_cgne.py:96-210) and CGNR (krylov/_cgnr.py:96-212), M = identity, criteria 'rr'.  At = A^H as an operator of its
// own (the reference applies A.H through SciPy's CSC product: the same per-output summation order as the CSR rows of A^T).
// r, p, w (and rhat for CGNR): n-vectors of work.
int cgn_core(pamg_solver_s *S, bool nr, pamg_matrix_s *Aop, pamg_matrix_s *At, int64_t n, void *r, void *rhat, void *p, void *w, void *x,
             const void *b, double tol, int maxiter, int *n_iter, int *info, hipStream_t s)
{
    const int dt = S->dtype;
    const size_t vb = (size_t)n * tsize(dt);
    if (maxiter <= 0 || (double)maxiter > 1.3 * (double)n) maxiter = (int)std::ceil(1.3 * (double)n) + 2;      // :108-115
    double *slot = S->d_slot;
    double h[3];
    auto fetch = [&](int k) -> int {
        PAMG_HIP(hipMemcpyAsync(h, slot + 1, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, s));
        return (int)hipStreamSynchronize(s);
    };
    PAMG_TRY(stream_launch(Aop, EPI_RESID, x, b, r, 0.0, 0.0, nullptr, s));              // r = b - A x
    if (nr) {
        PAMG_TRY(stream_launch(At, EPI_SET, r, nullptr, rhat, 0.0, 0.0, nullptr, s));    // rhat = A^H r; z = rhat; p = z
        PAMG_HIP(hipMemcpyAsync(p, rhat, vb, hipMemcpyDeviceToDevice, s));
        PAMG_TRY(vec_sumsq(dt, n, rhat, S->d_scratch, slot + 1, s));                     // (z, rhat)
    } else {
        PAMG_TRY(stream_launch(At, EPI_SET, r, nullptr, p, 0.0, 0.0, nullptr, s));       // z = r; p = A^H z
        PAMG_TRY(vec_sumsq(dt, n, r, S->d_scratch, slot + 1, s));                        // (z, r)
    }
    PAMG_TRY(vec_sumsq(dt, n, r, S->d_scratch, slot + 2, s));
    PAMG_TRY(vec_sumsq(dt, n, b, S->d_scratch, slot + 3, s));
    PAMG_TRY(fetch(3));
    double old_zr = h[0], normr = std::sqrt(h[1]), normb = std::sqrt(h[2]);
    if (normb == 0.0) normb = 1.0;
    const double rtol = tol * normb;
    int it = 0, inf = -2;
    if (normr < rtol) inf = 0;
    while (inf == -2) {
        double alpha;
        if (nr) {
            PAMG_TRY(stream_launch(Aop, EPI_SET, p, nullptr, w, 0.0, 0.0, nullptr, s));  // w = A p
            PAMG_TRY(vec_sumsq(dt, n, w, S->d_scratch, slot + 1, s));
        } else {
            PAMG_TRY(vec_sumsq(dt, n, p, S->d_scratch, slot + 1, s));
        }
        PAMG_TRY(fetch(1));
        alpha = old_zr / h[0];
        PAMG_TRY(vec_axpy(dt, n, alpha, p, x, s));                                       // x += alpha p
        if ((it % 8) != 0 && it > 0) {
            if (!nr) PAMG_TRY(stream_launch(Aop, EPI_SET, p, nullptr, w, 0.0, 0.0, nullptr, s));
            PAMG_TRY(vec_axpy(dt, n, -alpha, w, r, s));                                  // r -= alpha A p
        } else {
            PAMG_TRY(stream_launch(Aop, EPI_RESID, x, b, r, 0.0, 0.0, nullptr, s));
        }
        if (nr) {
            PAMG_TRY(stream_launch(At, EPI_SET, r, nullptr, rhat, 0.0, 0.0, nullptr, s));
            PAMG_TRY(vec_sumsq(dt, n, rhat, S->d_scratch, slot + 1, s));
        } else {
            PAMG_TRY(vec_sumsq(dt, n, r, S->d_scratch, slot + 1, s));
        }
        PAMG_TRY(vec_sumsq(dt, n, r, S->d_scratch, slot + 2, s));
        PAMG_TRY(fetch(2));
        const double new_zr = h[0], beta = new_zr / old_zr;
        old_zr = new_zr;
        if (nr) {
            PAMG_TRY(vec_xpby(dt, n, beta, rhat, p, s));                                 // p = beta p + z
        } else {
            PAMG_TRY(stream_launch(At, EPI_SET, r, nullptr, w, 0.0, 0.0, nullptr, s));   // p = beta p + A^H z
            PAMG_TRY(vec_xpby(dt, n, beta, w, p, s));
        }
        ++it;
        normr = std::sqrt(h[1]);
        if (normr < rtol) inf = 0;
        else if (it == maxiter) inf = it;
    }
    if (n_iter) *n_iter = it;
    if (info) *info = inf;
    return PAMG_OK;
}

// Flexible GMRES with the resident cycle as (right) preconditioner, all vectors on the device: a
// faithful restatement of the reference's krylov/_fgmres.py:120-345 as driven by
// MultilevelSolver.solve(accel='fgmres') (multilevel.py:479-535) -- Householder reflectors
// (amg_core::apply_householders, krylov.h:37-56), Givens rotations on the leading entries
// (apply_givens, krylov.h:158-183), the same stopping rules, residual history and return codes.  The
// Householder form is kept on purpose: its basis vectors differ from Gram-Schmidt ones by signs, which a
// linear preconditioner cannot see but the AMLI cycle (inner Krylov steps from a guess of ones) can.
// Only the n-vectors live on the device; the leading <= restart+1 entries the rotations work on are read
// back per iteration.
// flexible = true: FGMRES (right preconditioning, the preconditioned vectors Z are kept);
// flexible = false: the reference's default GMRES, krylov/_gmres_householder.py:120-330 (LEFT
// preconditioning: every norm is a preconditioned-residual norm, tolerance relative to ||M b||; the update
// is mapped back through the reflectors by amg_core::householder_hornerscheme, krylov.h:106-130).
// Aop / n: the operator the method runs on (level 0 for the accelerators, any level for a Krylov smoother or coarse solver);
// cycle < 0: no preconditioner (M = identity), else the resident cycle of the whole hierarchy.
int krylov_householder(pamg_solver_s *S, pamg_matrix_s *Aop, int64_t n, bool flexible, void *x, const void *b, double tol, int maxiter,
                       int restart, int cycle, int cycles_per_level, double *residuals, int residuals_cap, int *n_res,
                       int *n_iter, int *info, hipStream_t s)
{
    Level &L0 = S->levels[0];
    if (n < 2) return PAMG_E_UNSUPPORTED;              // the reference special-cases n == 1 on the host
    const int dt = S->dtype;
    const size_t ts = tsize(dt);
    const size_t vb = (size_t)n * ts;
    // iteration limits exactly as _fgmres.py:139-160
    int max_outer, max_inner;
    if (restart > 0) {
        max_outer = maxiter > 0 ? maxiter : 1;
        max_inner = (int)std::min<int64_t>(restart, n);
    } else {
        max_outer = 1;
        max_inner = maxiter > 0 ? (int)std::min<int64_t>(maxiter, n) : (int)std::min<int64_t>(n, 40);
    }
    const int m = max_inner;
    int nres = 0, inf = 0, nit = 0;
    auto push = [&](double v) { if (residuals && nres < residuals_cap) residuals[nres] = v; ++nres; };
    std::vector<void *> W((size_t)m, nullptr), Z((size_t)m, nullptr);
    void *v = nullptr, *u = nullptr, *r = nullptr;
    auto release = [&]() {
        for (void *p : W) if (p) hipFree(p);
        for (void *p : Z) if (p) hipFree(p);
        if (v) hipFree(v);
        if (u) hipFree(u);
        if (r) hipFree(r);
    };
    auto grab = [&](void **p) -> int { return *p ? PAMG_OK : (int)hipMalloc(p, vb + 64); };
    int st = grab(&v);
    if (!st) st = grab(&u);
    if (!st) st = grab(&r);
    if (!st) st = grab(&W[0]);
    if (st) { release(); return st; }
    double *slot = S->d_slot;
    double h1[2];
    std::vector<unsigned char> hbuf((size_t)(m + 2) * ts);
    auto fetch = [&](int k) -> int {
        PAMG_HIP(hipMemcpyAsync(h1, slot + 1, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, s));
        return (int)hipStreamSynchronize(s);
    };
    auto at = [&](void *p, int64_t idx) -> void * { return (unsigned char *)p + (size_t)idx * ts; };
    auto get = [&](void *p, int64_t idx, int cnt, double *out) -> int {     // out[0..cnt) = p[idx..idx+cnt)
        PAMG_HIP(hipMemcpyAsync(hbuf.data(), at(p, idx), (size_t)cnt * ts, hipMemcpyDeviceToHost, s));
        PAMG_HIP(hipStreamSynchronize(s));
        for (int k = 0; k < cnt; ++k)
            out[k] = dt == PAMG_F64 ? reinterpret_cast<const double *>(hbuf.data())[k] : (double)reinterpret_cast<const float *>(hbuf.data())[k];
        return PAMG_OK;
    };
    auto put = [&](void *p, int64_t idx, double val) -> int {
        double vd = val; float vf = (float)val;
        PAMG_HIP(hipMemcpyAsync(at(p, idx), dt == PAMG_F64 ? (const void *)&vd : (const void *)&vf, ts, hipMemcpyHostToDevice, s));
        return (int)hipStreamSynchronize(s);                               // the host scalar goes out of scope
    };
    auto norm2 = [&](const void *p, int64_t len, double *out) -> int {
        PAMG_TRY(vec_sumsq(dt, len, p, S->d_scratch, slot + 1, s));
        PAMG_TRY(fetch(1));
        *out = std::sqrt(h1[0]);
        return PAMG_OK;
    };
    auto reflect = [&](void *z, const void *wj) -> int {                   // z -= 2 (w_j . z) w_j
        PAMG_TRY(vec_dot(dt, n, wj, z, S->d_scratch, slot + 1, s));
        PAMG_TRY(fetch(1));
        return vec_axpy(dt, n, -2.0 * h1[0], wj, z, s);
    };
    auto precond = [&](const void *vin, void *zout) -> int {               // z = M v: one cycle from x = 0
        if (cycle < 0) return (int)hipMemcpyAsync(zout, vin, vb, hipMemcpyDeviceToDevice, s);
        PAMG_HIP(hipMemcpyAsync(L0.b, vin, vb, hipMemcpyDeviceToDevice, s));
        PAMG_HIP(hipMemsetAsync(L0.x, 0, vb, s));
        PAMG_TRY(run_cycle(S, cycle, cycles_per_level, s, false, true));
        return (int)hipMemcpyAsync(zout, L0.x, vb, hipMemcpyDeviceToDevice, s);
    };
    auto mysign = [](double t) { return t == 0.0 ? 1.0 : t / std::fabs(t); };
    auto body = [&]() -> int {
        double normr, normb;
        auto residual = [&]() -> int {                                                    // r = b - A x  (GMRES: M (b - A x))
            if (flexible) return stream_launch(Aop, EPI_RESID, x, b, r, 0.0, 0.0, nullptr, s);
            PAMG_TRY(stream_launch(Aop, EPI_RESID, x, b, v, 0.0, 0.0, nullptr, s));
            return precond(v, r);
        };
        PAMG_TRY(residual());
        PAMG_TRY(norm2(r, n, &normr));
        PAMG_TRY(norm2(b, n, &normb));
        push(normr);
        if (normb == 0.0) normb = 1.0;
        else if (!flexible) {                                                             // tolerance relative to ||M b||
            PAMG_TRY(precond(b, v));
            PAMG_TRY(norm2(v, n, &normb));
        }
        if (normr < tol * normb) { inf = 0; return PAMG_OK; }
        int niter = 0;
        std::vector<double> H((size_t)m * m), Q((size_t)4 * m), g((size_t)m + 1), y((size_t)m), hv((size_t)m + 2);
        auto Hx = [&](int i, int j) -> double & { return H[(size_t)j * m + i]; };
        for (int outer = 0; outer < max_outer; ++outer) {
            std::fill(H.begin(), H.end(), 0.0);
            std::fill(g.begin(), g.end(), 0.0);
            // first reflector from the residual (:184-197)
            double t, nw;
            PAMG_HIP(hipMemcpyAsync(W[0], r, vb, hipMemcpyDeviceToDevice, s));
            PAMG_TRY(get(W[0], 0, 1, &t));
            const double beta = mysign(t) * normr;
            PAMG_TRY(put(W[0], 0, t + beta));
            PAMG_TRY(norm2(W[0], n, &nw));
            PAMG_TRY(vec_scale(dt, n, 1.0 / nw, W[0], W[0], s));
            g[0] = -beta;
            int wi = 0, inner = 0;
            for (inner = 0; inner < m; ++inner) {
                void *w = W[wi];
                // v = e_inner - 2 w[inner] w, then the earlier reflectors in reverse (:209-214)
                PAMG_TRY(get(w, inner, 1, &t));
                PAMG_TRY(vec_scale(dt, n, -2.0 * t, w, v, s));
                PAMG_TRY(get(v, inner, 1, &t));
                PAMG_TRY(put(v, inner, t + 1.0));
                for (int j = inner - 1; j >= 0; --j) PAMG_TRY(reflect(v, W[j]));
                if (flexible) {
                    PAMG_TRY(grab(&Z[inner]));
                    PAMG_TRY(precond(v, Z[inner]));                                       // z = M v
                    PAMG_TRY(stream_launch(Aop, EPI_SET, Z[inner], nullptr, v, 0.0, 0.0, nullptr, s));   // v = A z
                } else {
                    PAMG_TRY(stream_launch(Aop, EPI_SET, v, nullptr, u, 0.0, 0.0, nullptr, s));          // v = M (A v)
                    PAMG_TRY(precond(u, v));
                }
                for (int j = 0; j <= inner; ++j) PAMG_TRY(reflect(v, W[j]));
                if (inner != n - 1) {                                                     // next reflector (:229-246)
                    if (inner < m - 1) wi = inner + 1;
                    double alpha;
                    PAMG_TRY(norm2(at(v, inner + 1), n - inner - 1, &alpha));
                    if (alpha != 0.0) {
                        PAMG_TRY(get(v, inner + 1, 1, &t));
                        alpha = mysign(t) * alpha;
                        if (inner < m - 1) {
                            PAMG_TRY(grab(&W[inner + 1]));
                            void *wn = W[inner + 1];
                            PAMG_HIP(hipMemsetAsync(wn, 0, (size_t)(inner + 1) * ts, s));
                            PAMG_HIP(hipMemcpyAsync(at(wn, inner + 1), at(v, inner + 1), (size_t)(n - inner - 1) * ts, hipMemcpyDeviceToDevice, s));
                            PAMG_TRY(put(wn, inner + 1, t + alpha));
                            PAMG_TRY(norm2(wn, n, &nw));
                            PAMG_TRY(vec_scale(dt, n, 1.0 / nw, wn, wn, s));
                        }
                        PAMG_TRY(put(v, inner + 1, -alpha));                              // v[inner+2:] = 0 is implied below
                    }
                }
                // the rotations work on the leading entries only (:248-266)
                const int lead = (int)std::min<int64_t>(inner + 2, n);
                std::fill(hv.begin(), hv.end(), 0.0);
                PAMG_TRY(get(v, 0, lead, hv.data()));
                for (int rot = 0; rot < inner; ++rot) {
                    const double xt = hv[rot];
                    hv[rot] = Q[4 * rot] * xt + Q[4 * rot + 1] * hv[rot + 1];
                    hv[rot + 1] = Q[4 * rot + 2] * xt + Q[4 * rot + 3] * hv[rot + 1];
                }
                if (inner != n - 1 && hv[inner + 1] != 0.0) {
                    const double f = hv[inner], gg = hv[inner + 1];                       // LAPACK lartg
                    double c, sn;
                    if (f == 0.0) { c = 0.0; sn = 1.0; }
                    else { const double rr = std::copysign(std::hypot(f, gg), f); c = f / rr; sn = gg / rr; }
                    Q[4 * inner] = c; Q[4 * inner + 1] = sn; Q[4 * inner + 2] = -sn; Q[4 * inner + 3] = c;
                    const double g0 = g[inner], g1 = g[inner + 1];
                    g[inner] = c * g0 + sn * g1;
                    g[inner + 1] = -sn * g0 + c * g1;
                    hv[inner] = c * f + sn * gg;
                    hv[inner + 1] = 0.0;
                }
                for (int i = 0; i < m; ++i) Hx(i, inner) = i < lead ? hv[i] : 0.0;
                if (!flexible) ++niter;                                                   // GMRES counts before the test
                if (inner < m - 1) {                                                      // :283-289
                    normr = std::fabs(g[inner + 1]);
                    if (normr < tol * normb) break;
                    push(normr);
                }
                if (flexible) ++niter;
            }
            const int k = std::min(inner + 1, m);
            for (int i = k - 1; i >= 0; --i) {                                            // H is upper triangular now
                double acc = g[i];
                for (int j = i + 1; j < k; ++j) acc -= Hx(i, j) * y[j];
                y[i] = acc / Hx(i, i);
            }
            if (flexible) {
                PAMG_TRY(vec_scale(dt, n, y[0], Z[0], u, s));                             // update = Z y
                for (int j = 1; j < k; ++j) PAMG_TRY(vec_axpy(dt, n, y[j], Z[j], u, s));
            } else {
                PAMG_HIP(hipMemsetAsync(u, 0, vb, s));                                    // Horner scheme through the reflectors
                for (int j = k - 1; j >= 0; --j) {
                    PAMG_TRY(get(u, j, 1, &t));
                    PAMG_TRY(put(u, j, t + y[j]));
                    PAMG_TRY(reflect(u, W[j]));
                }
            }
            PAMG_TRY(vec_axpy(dt, n, 1.0, u, x, s));
            PAMG_TRY(residual());
            PAMG_TRY(norm2(r, n, &normr));
            push(normr);
            PAMG_TRY(vec_maxratio(dt, n, u, x, S->d_scratch, slot + 1, s));               // stagnation, :316-322
            PAMG_TRY(fetch(1));
            nit = niter;
            if (h1[0] >= 0.0 && h1[0] < 1e-12) { inf = -1; return PAMG_OK; }
            if (normr < tol * normb) { inf = 0; return PAMG_OK; }
        }
        inf = niter;
        nit = niter;
        return PAMG_OK;
    };
    st = body();
    hipStreamSynchronize(s);
    release();
    if (info) *info = inf;
    if (n_iter) *n_iter = nit;
    if (n_res) *n_res = nres;
    return st;
}


// BiCGStab, CR, steepest descent and minimal residual with the resident cycle as preconditioner M (one cycle from x = 0), faithful
// restatements of the reference's krylov/_bicgstab.py, _cr.py, _steepest_descent.py and _minimal_residual.py under criteria 'rr' as
// MultilevelSolver.solve(accel=...) drives them (multilevel.py:479-535).  The operand of M is the fine level's right-hand side
// L0.b and its result the fine level's iterate L0.x: each method keeps the vector it preconditions there (r for CR and SD, s and
// then the new direction for BiCGStab, A z for MR), and the fused steps of pamg_krylov.hip clear L0.x behind the last reader of a
// cycle's result.  Per iteration the host reads back ONE group of scalars -- the residual norm and whatever breakdown test the
// reference makes -- everything else (step sizes, inner products) stays in device slots.
struct KrylovRun {
    pamg_solver_s *S;
    Level &L0;
    int dt;
    int64_t n;
    size_t vb;
    int cycle, cpl;
    hipStream_t s;
    double *part, *sl;              // partials, scalar slots (S->kr_red)
    double *residuals;
    int cap, nres = 0;
    double h[8];

    void push(double v) { if (residuals && nres < cap) residuals[nres] = v; ++nres; }
    int fetch(int first, int k)     // h[0..k) = sl[first .. first+k): the iteration's one read-back
    {
        PAMG_HIP(hipMemcpyAsync(h, sl + first, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, s));
        return (int)hipStreamSynchronize(s);
    }
    int precond() { return run_cycle(S, cycle, cpl, s, false, true); }   // L0.x = M L0.b (L0.x is zero on entry)
    int dots(int k, const void *a0, const void *b0, const void *a1, const void *b1, const void *a2, const void *b2, double *o0,
             double *o1 = nullptr, double *o2 = nullptr)
    {
        PAMG_TRY(kr_dots(dt, n, k, a0, b0, a1, b1, a2, b2, part, s));
        return kr_reduce(n, part, k, o0, o1, o2, s);
    }
    int reduce(int k, double *o0, double *o1 = nullptr) { return kr_reduce(n, part, k, o0, o1, nullptr, s); }
    int matvec(const void *v, void *out) { return stream_launch(L0.A, EPI_SET, v, nullptr, out, 0.0, 0.0, nullptr, s); }
    int residual(const void *x, const void *b, void *out) { return stream_launch(L0.A, EPI_RESID, x, b, out, 0.0, 0.0, nullptr, s); }
    int copy(void *dst, const void *src) { return (int)hipMemcpyAsync(dst, src, vb, hipMemcpyDeviceToDevice, s); }
};

// krylov/_bicgstab.py:84-188.  No breakdown test (the reference has none): a zero denominator gives inf / nan as NumPy's does.
// Work: r, r*, p, A M p, A M s.  Slots: [0,1] (r*, r) of this / the next iteration, [2] (r*, AMp), [3] alpha, [4] omega,
// [5] (AMs, s), [6] (AMs, AMs), [7] ||r||^2, [8] ||b||^2.
int bicgstab_core(KrylovRun &K, void *x, const void *b, double tol, int maxiter, int &it, int &inf)
{
    void **v = K.S->kr_v;
    void *r = v[0], *rstar = v[1], *p = v[2], *AMp = v[3], *AMs = v[4];
    void *bc = K.L0.b, *xc = K.L0.x;
    double *sl = K.sl;
    PAMG_TRY(K.residual(x, b, r));                                                        // r = b - A x
    PAMG_TRY(K.dots(3, r, r, b, b, r, r, sl + 7, sl + 8, sl + 0));                        // ||r||^2, ||b||^2, (r*, r) with r* = r
    PAMG_TRY(K.fetch(7, 2));
    const double normr0 = std::sqrt(K.h[0]);
    double normb = std::sqrt(K.h[1]);
    K.push(normr0);
    if (normb == 0.0) normb = 1.0;
    const double rtol = tol * normb;
    if (normr0 < rtol) { inf = 0; return PAMG_OK; }
    PAMG_TRY(K.copy(rstar, r));
    PAMG_TRY(K.copy(p, r));
    PAMG_TRY(K.copy(bc, r));                                                              // the first cycle's operand: p
    PAMG_HIP(hipMemsetAsync(xc, 0, K.vb, K.s));
    while (true) {
        double *rr_old = sl + (it & 1), *rr_new = sl + ((it + 1) & 1);
        PAMG_TRY(K.precond());                                                            // xc = M p
        PAMG_TRY(K.matvec(xc, AMp));
        PAMG_TRY(K.dots(1, rstar, AMp, nullptr, nullptr, nullptr, nullptr, sl + 2));
        PAMG_TRY(bicg_alpha(K.dt, K.n, rr_old, sl + 2, sl + 3, x, xc, r, AMp, bc, K.s));  // x += alpha Mp; bc = s; xc = 0
        PAMG_TRY(K.precond());                                                            // xc = M s
        PAMG_TRY(K.matvec(xc, AMs));
        PAMG_TRY(K.dots(2, AMs, bc, AMs, AMs, nullptr, nullptr, sl + 5, sl + 6));
        PAMG_TRY(bicg_omega(K.dt, K.n, sl + 5, sl + 6, sl + 4, x, xc, bc, AMs, r, rstar, K.part, K.s));   // x += omega Ms; r = s - omega AMs
        PAMG_TRY(K.reduce(2, rr_new, sl + 7));
        PAMG_TRY(bicg_dir(K.dt, K.n, rr_new, rr_old, sl + 3, sl + 4, r, p, AMp, bc, xc, K.s));          // p = r + beta (p - omega AMp); bc = p
        PAMG_TRY(K.fetch(7, 1));
        ++it;
        const double normr = std::sqrt(K.h[0]);
        K.push(normr);
        if (normr < rtol) { inf = 0; break; }
        if (it == maxiter) { inf = it; break; }
    }
    return PAMG_OK;
}

// krylov/_cr.py:87-199.  r lives in bc, z = M r in xc.  Work: p, Ap, Az.  Slots: [0,1] (r, Az) of this / the next iteration,
// [2] (Ap, Ap), [3] (z, z), [4] ||r||^2, [5] ||b||^2.
int cr_core(KrylovRun &K, void *x, const void *b, double tol, int maxiter, int &it, int &inf)
{
    void **v = K.S->kr_v;
    void *p = v[0], *Ap = v[1], *Az = v[2];
    void *r = K.L0.b, *xc = K.L0.x;
    double *sl = K.sl;
    PAMG_TRY(K.residual(x, b, r));                                                        // r = b - A x
    PAMG_HIP(hipMemsetAsync(xc, 0, K.vb, K.s));
    PAMG_TRY(K.precond());                                                                // z = M r
    PAMG_TRY(K.dots(2, r, r, b, b, nullptr, nullptr, sl + 4, sl + 5));
    PAMG_TRY(K.fetch(4, 2));
    const double normr0 = std::sqrt(K.h[0]);
    double normb = std::sqrt(K.h[1]);
    K.push(normr0);
    if (normb == 0.0) normb = 1.0;
    const double rtol = tol * normb;
    if (normr0 < rtol) { inf = 0; return PAMG_OK; }
    PAMG_TRY(K.matvec(xc, Az));                                                           // Az = A z
    PAMG_TRY(K.copy(p, xc));                                                              // p = z
    PAMG_TRY(K.copy(Ap, Az));                                                             // Ap = A p: the same product, the same bits
    PAMG_TRY(K.dots(2, r, Az, Ap, Ap, nullptr, nullptr, sl + 0, sl + 2));
    while (true) {
        double *rAz_old = sl + (it & 1), *rAz_new = sl + ((it + 1) & 1);
        const bool recompute = !((it % 8) != 0 && it > 0);                                // _cr.py:151-154
        PAMG_TRY(cr_update(K.dt, K.n, rAz_old, sl + 2, x, p, r, Ap, !recompute, xc, K.s));   // x += alpha p; [r -= alpha Ap]; xc = 0
        if (recompute) PAMG_TRY(K.residual(x, b, r));
        PAMG_TRY(K.precond());                                                            // z = M r
        PAMG_TRY(K.matvec(xc, Az));
        PAMG_TRY(K.dots(3, r, Az, xc, xc, r, r, rAz_new, sl + 3, sl + 4));
        PAMG_TRY(cr_dir(K.dt, K.n, rAz_new, rAz_old, p, xc, Ap, Az, K.part, K.s));        // p = beta p + z; Ap = beta Ap + Az
        PAMG_TRY(K.reduce(1, sl + 2));
        PAMG_TRY(K.fetch(3, 2));
        ++it;
        const double zz = K.h[0], normr = std::sqrt(K.h[1]);
        K.push(normr);
        if (normr < rtol) { inf = 0; break; }
        if (zz == 0.0) { inf = -1; break; }                                               // singular preconditioner
        if (it == maxiter) { inf = it; break; }
    }
    return PAMG_OK;
}

// krylov/_steepest_descent.py:92-197.  r lives in bc, z = M r in xc.  Work: q = A z.  Slots: [0] (r, z), [1] (z, A z),
// [2] ||r||^2, [3] ||b||^2.  The curvature test of A comes before the update of x in the reference: sd_update skips that write
// when (z, A z) < 0, and the host reports -1 from the same read-back as the residual.
int sd_core(KrylovRun &K, void *x, const void *b, double tol, int maxiter, int &it, int &inf)
{
    void *q = K.S->kr_v[0];
    void *r = K.L0.b, *xc = K.L0.x;
    double *sl = K.sl;
    PAMG_TRY(K.residual(x, b, r));
    PAMG_HIP(hipMemsetAsync(xc, 0, K.vb, K.s));
    PAMG_TRY(K.precond());                                                                // z = M r
    PAMG_TRY(K.dots(3, r, xc, r, r, b, b, sl + 0, sl + 2, sl + 3));
    PAMG_TRY(K.fetch(2, 2));
    double normb = std::sqrt(K.h[1]);
    K.push(std::sqrt(K.h[0]));
    if (normb == 0.0) normb = 1.0;
    const double rtol = tol * normb;                                                      // (the reference does not test the initial guess)
    while (true) {
        PAMG_TRY(K.matvec(xc, q));                                                        // q = A z
        PAMG_TRY(K.dots(1, xc, q, nullptr, nullptr, nullptr, nullptr, sl + 1));
        // The reference's recompute test is inverted (`if np.mod(it, recompute_r) and it > 0: r = b - A x`, it already
        // incremented): r is recomputed on every iteration EXCEPT multiples of 50, where it is updated.  Kept as it is.
        const bool recompute = ((it + 1) % 50) != 0;
        PAMG_TRY(sd_update(K.dt, K.n, sl + 0, sl + 1, x, xc, r, q, !recompute, K.s));     // x = x + alpha z; [r = r - alpha q]; xc = 0
        if (recompute) PAMG_TRY(K.residual(x, b, r));
        PAMG_TRY(K.precond());                                                            // z = M r
        PAMG_TRY(K.dots(2, r, xc, r, r, nullptr, nullptr, sl + 0, sl + 2));
        PAMG_TRY(K.fetch(0, 3));
        const double rz = K.h[0], zAz = K.h[1], normr = std::sqrt(K.h[2]);
        if (zAz < 0.0) { inf = -1; break; }                                               // indefinite A: x was not touched
        ++it;
        if (rz < 0.0) { inf = -1; break; }                                                // indefinite M (before the history entry)
        K.push(normr);
        if (normr < rtol) { inf = 0; break; }
        if (rz == 0.0) { inf = -1; break; }                                               // singular M
        if (it == maxiter) { inf = it; break; }
    }
    return PAMG_OK;
}

// krylov/_minimal_residual.py:95-163: residuals and the stopping test are preconditioned norms ||z|| = ||M r||, relative to
// ||M b|| (one more cycle at setup; 1 when b = 0).  Work: z.  A z is written straight into bc (the operand of M), p = M A z
// arrives in xc.  Slots: [0] (p, z), [1] (p, p), [2] ||z||^2, [3] ||b||^2, [4] ||M b||^2.
int mr_core(KrylovRun &K, void *x, const void *b, double tol, int maxiter, int &it, int &inf)
{
    void *z = K.S->kr_v[0];
    void *bc = K.L0.b, *xc = K.L0.x;
    double *sl = K.sl;
    PAMG_TRY(K.residual(x, b, bc));                                                       // r = b - A x
    PAMG_HIP(hipMemsetAsync(xc, 0, K.vb, K.s));
    PAMG_TRY(K.precond());
    PAMG_TRY(kr_take(K.dt, K.n, xc, z, K.part, K.s));                                     // z = M r; xc = 0
    PAMG_TRY(K.reduce(1, sl + 2));
    PAMG_TRY(K.dots(1, b, b, nullptr, nullptr, nullptr, nullptr, sl + 3));
    PAMG_TRY(K.fetch(2, 2));
    const double normr0 = std::sqrt(K.h[0]);
    K.push(normr0);
    double normMb = 1.0;
    if (K.h[1] != 0.0) {                                                                  // ||M b||
        PAMG_TRY(K.copy(bc, b));
        PAMG_TRY(K.precond());
        PAMG_TRY(K.dots(1, xc, xc, nullptr, nullptr, nullptr, nullptr, sl + 4));
        PAMG_HIP(hipMemsetAsync(xc, 0, K.vb, K.s));
        PAMG_TRY(K.fetch(4, 1));
        normMb = std::sqrt(K.h[0]);
    }
    const double rtol = tol * normMb;
    if (normr0 < rtol) { inf = 0; return PAMG_OK; }
    while (true) {
        PAMG_TRY(K.matvec(z, bc));                                                        // bc = A z
        PAMG_TRY(K.precond());                                                            // p = M A z
        PAMG_TRY(K.dots(2, xc, z, xc, xc, nullptr, nullptr, sl + 0, sl + 1));
        // the same inverted recompute test as steepest descent (_minimal_residual.py:145-149): on every iteration but multiples of
        // 50, r = b - A x and z = M r -- two cycles per iteration
        const bool recompute = ((it + 1) % 50) != 0;
        PAMG_TRY(mr_update(K.dt, K.n, sl + 0, sl + 1, x, z, xc, !recompute, K.part, K.s));    // x = x + alpha z; [z = z - alpha p]; xc = 0
        if (recompute) {
            PAMG_TRY(K.residual(x, b, bc));
            PAMG_TRY(K.precond());
            PAMG_TRY(kr_take(K.dt, K.n, xc, z, K.part, K.s));                             // z = M r; xc = 0
        }
        PAMG_TRY(K.reduce(1, sl + 2));
        PAMG_TRY(K.fetch(0, 3));
        if (K.h[0] < 0.0) { inf = -1; break; }                                            // indefinite M A: x was not touched
        ++it;
        const double normr = std::sqrt(K.h[2]);
        K.push(normr);
        if (normr < rtol) { inf = 0; break; }
        if (it == maxiter) { inf = it; break; }
    }
    return PAMG_OK;
}

// A Krylov method as smoother / coarse solver (smoothing.py:794-830, multilevel.py:752-762): x[:] = method(A, b, x0 = x, ...)[0].
// The iteration reads scalars back to the host (the reference's stopping rules are data dependent): such a cycle is not captured.
int krylov_smooth(pamg_solver_s *S, Level &L, const Smoother &sm, hipStream_t s)
{
    const int64_t n = L.n;
    if (n == 0) return PAMG_OK;
    const size_t ts = tsize(S->dtype);
    unsigned char *kw = (unsigned char *)sm.kw;
    void *w0 = kw, *w1 = kw + (size_t)n * ts, *w2 = kw + 2 * (size_t)n * ts, *w3 = kw + 3 * (size_t)n * ts;
    int it = 0, inf = 0;
    switch (sm.kmethod) {
        case PAMG_KRYLOV_CG:
            return cg_core(S, L.A, n, nullptr, w0, w0, w1, w2, L.x, L.b, sm.ktol, sm.kmaxiter, nullptr, &it, &inf, s);
        case PAMG_KRYLOV_CGNE:
            return cgn_core(S, false, L.A, sm.At, n, w0, w3, w1, w2, L.x, L.b, sm.ktol, sm.kmaxiter, &it, &inf, s);
        case PAMG_KRYLOV_CGNR:
            return cgn_core(S, true, L.A, sm.At, n, w0, w3, w1, w2, L.x, L.b, sm.ktol, sm.kmaxiter, &it, &inf, s);
        case PAMG_KRYLOV_GMRES: {
            int nres = 0;
            return krylov_householder(S, L.A, n, false, L.x, L.b, sm.ktol, sm.kmaxiter, sm.krestart, -1, 1, nullptr, 0, &nres, &it, &inf, s);
        }
    }
    return PAMG_E_ARG;
}

}  // namespace

extern "C" {

// ----------------------------------------------------------- smoothers on operator handles
int pamg_matrix_jacobi(pamg_matrix_t A, void *x, const void *b, void *work, double omega, int iterations,
                       pamg_stream_t s)
{
    if (!A || !x || !b || !work || iterations < 0) return PAMG_E_ARG;
    void *cur = x, *alt = work;
    PAMG_TRY(jacobi_pp(A, &cur, &alt, b, omega, iterations, (hipStream_t)s));
    if (cur != x)
        PAMG_HIP(hipMemcpyAsync(x, cur, (size_t)A->nrows * tsize(A->dtype), hipMemcpyDeviceToDevice, (hipStream_t)s));
    return PAMG_OK;
}

int pamg_matrix_jacobi_step(pamg_matrix_t A, const void *x_in, const void *b, void *x_out, double omega,
                            pamg_stream_t s)
{
    if (!A || !x_in || !b || !x_out) return PAMG_E_ARG;
    if (A->R != A->C || A->ncols < A->nrows) return PAMG_E_UNSUPPORTED;
    if (A->nrows == 0) return PAMG_OK;
    if (A->R > 1) return block_jacobi_step(A, PNT_JACOBI, nullptr, x_in, x_out, b, omega, (hipStream_t)s);
    return stream_launch(A, A->flavour == PAMG_BSR ? EPI_JACOBI_B : EPI_JACOBI, x_in, b, x_out, 0.0, omega,
                         nullptr, (hipStream_t)s);
}

int pamg_matrix_block_jacobi_step(pamg_matrix_t A, const void *Dinv, const void *x_in, const void *b, void *x_out,
                                  double omega, pamg_stream_t s)
{
    if (!A || !Dinv || !x_in || !b || !x_out) return PAMG_E_ARG;
    if (A->R != A->C || A->R < 2 || A->ncols < A->nrows) return PAMG_E_UNSUPPORTED;
    if (A->nrows == 0) return PAMG_OK;
    return block_jacobi_step(A, BLK_JACOBI, Dinv, x_in, x_out, b, omega, (hipStream_t)s);
}

int pamg_matrix_block_jacobi_indexed(pamg_matrix_t A, const void *Dinv, void *x, const void *b, const int32_t *idx,
                                     int64_t nidx, double omega, void *work, pamg_stream_t s)
{
    if (!A || !Dinv || !x || !b || !work || nidx < 0 || (nidx > 0 && !idx)) return PAMG_E_ARG;
    if (A->R != A->C || A->R < 2 || A->ncols != A->nrows) return PAMG_E_UNSUPPORTED;
    if (A->nrows == 0 || nidx == 0) return PAMG_OK;
    PAMG_TRY(block_jacobi_step(A, BLK_JACOBI, Dinv, x, work, b, omega, (hipStream_t)s));
    return vec_copy_indexed(A->dtype, nidx, idx, work, x, (hipStream_t)s);
}

int pamg_matrix_gauss_seidel(pamg_matrix_t A, void *x, const void *b, int sweep, double omega,
                             int iterations, pamg_stream_t s)
{
    if (!A || !x || !b || iterations < 0) return PAMG_E_ARG;
    if (sweep < PAMG_FORWARD || sweep > PAMG_SYMMETRIC) return PAMG_E_ARG;
    return gs_apply(A, x, b, sweep, omega, iterations, (hipStream_t)s);
}

int pamg_matrix_gauss_seidel_x0(pamg_matrix_t A, void *x, const void *b, int sweep, double omega,
                                int iterations, int x_is_zero, pamg_stream_t s)
{
    if (!A || !x || !b || iterations < 0) return PAMG_E_ARG;
    if (sweep < PAMG_FORWARD || sweep > PAMG_SYMMETRIC) return PAMG_E_ARG;
    return gs_apply(A, x, b, sweep, omega, iterations, (hipStream_t)s, x_is_zero != 0);
}

int pamg_matrix_gauss_seidel_correction(pamg_matrix_t A, void *x, const void *b, void *r, int iterations, pamg_stream_t s)
{
    if (!A || !x || !b || !r || iterations < 0) return PAMG_E_ARG;
    if (!square_ok(A)) return PAMG_E_ARG;
    for (int it = 0; it < iterations; ++it) {
        bool ran = false;
        PAMG_TRY(gs_sweep_dtri(A, x, b, r, false, (hipStream_t)s, &ran));
        if (!ran) PAMG_TRY(gs_sweep_correction(A, x, b, r, true, (hipStream_t)s, &ran));
        if (!ran) return PAMG_E_UNSUPPORTED;
    }
    return PAMG_OK;
}

int pamg_matrix_polynomial(pamg_matrix_t A, void *x, const void *b, void *work, const double *coeffs,
                           int ncoeffs, int iterations, int x_is_zero, pamg_stream_t s)
{
    if (!A || !x || !b || !work || iterations < 0) return PAMG_E_ARG;
    return poly_apply(A, x, b, work, coeffs, ncoeffs, iterations, x_is_zero, (hipStream_t)s);
}

int pamg_matrix_block_jacobi(pamg_matrix_t A, void *x, const void *b, void *work, const void *Dinv,
                             double omega, int iterations, pamg_stream_t s)
{
    if (!A || !x || !b || !work || iterations < 0) return PAMG_E_ARG;
    void *cur = x, *alt = work;
    PAMG_TRY(block_jacobi_pp(A, &cur, &alt, b, Dinv, omega, iterations, (hipStream_t)s));
    if (cur != x)
        PAMG_HIP(hipMemcpyAsync(x, cur, (size_t)A->nrows * tsize(A->dtype), hipMemcpyDeviceToDevice, (hipStream_t)s));
    return PAMG_OK;
}

int pamg_matrix_block_gauss_seidel(pamg_matrix_t A, void *x, const void *b, const void *Dinv, int sweep,
                                   int iterations, pamg_stream_t s)
{
    if (!A || !x || !b || iterations < 0) return PAMG_E_ARG;
    if (sweep < PAMG_FORWARD || sweep > PAMG_SYMMETRIC) return PAMG_E_ARG;
    return block_gs_apply(A, x, b, Dinv, sweep, iterations, (hipStream_t)s);
}

// ----------------------------------------------------------------------------- solver
int pamg_solver_create(pamg_solver_t *S, int dtype)
{
    if (!S) return PAMG_E_ARG;
    if (dtype != PAMG_F64 && dtype != PAMG_F32) return PAMG_E_UNSUPPORTED;
    pamg_solver_s *p = new (std::nothrow) pamg_solver_s();
    if (!p) return PAMG_E_ALLOC;
    p->dtype = dtype;
    *S = p;
    return PAMG_OK;
}

int pamg_solver_destroy(pamg_solver_t S)
{
    if (!S) return PAMG_OK;
    drop_graphs(S);
    tail_free(S);
    for (Level &L : S->levels) {
        if (L.A) L.A->borrowed--;
        if (L.P) L.P->borrowed--;
        if (L.R) L.R->borrowed--;
        hipFree(L.x); hipFree(L.xalt);
        hipFree(L.b); hipFree(L.r); hipFree(L.work); hipFree(L.amli);
        hipFree(L.pre.d_Dinv); hipFree(L.post.d_Dinv);
        for (Smoother *sm : {&L.pre, &L.post}) {
            if (sm->AF) pamg_matrix_destroy(sm->AF);
            if (sm->AC) pamg_matrix_destroy(sm->AC);
            hipFree(sm->wF); hipFree(sm->wC); hipFree(sm->iF); hipFree(sm->iC); hipFree(sm->kw);
            if (sm->sw) pamg_schwarz_destroy(sm->sw);
        }
    }
    hipFree(S->d_coarse); hipFree(S->d_norms); hipFree(S->d_slot); hipFree(S->d_scratch);
    hipFree(S->cg_r); hipFree(S->cg_z); hipFree(S->cg_p); hipFree(S->cg_q);
    for (void *v : S->kr_v) hipFree(v);
    hipFree(S->kr_red);
    if (S->own_stream) hipStreamDestroy(S->own_stream);
    delete S;
    return PAMG_OK;
}

int pamg_solver_add_level(pamg_solver_t S, pamg_matrix_t A, pamg_matrix_t P, pamg_matrix_t R)
{
    if (!S || !A) return PAMG_E_ARG;
    if (S->finalized) return PAMG_E_STATE;
    if (A->dtype != S->dtype || A->nrows != A->ncols) return PAMG_E_ARG;
    if ((P == nullptr) != (R == nullptr)) return PAMG_E_ARG;
    if (!S->levels.empty()) {
        const Level &prev = S->levels.back();
        if (!prev.P) return PAMG_E_STATE;                      // a coarsest level was already added
        if (prev.P->ncols != A->nrows || prev.R->nrows != A->nrows) return PAMG_E_ARG;
    }
    if (P && (P->dtype != S->dtype || R->dtype != S->dtype || P->nrows != A->nrows || R->ncols != A->nrows ||
              P->ncols != R->nrows))
        return PAMG_E_ARG;
    Level L;
    L.A = A; L.P = P; L.R = R; L.n = A->nrows;
    S->levels.push_back(L);
    // from here on captured graphs may point into the operators' plans and schedules: pamg_matrix_tune /
    // pamg_matrix_autotune refuse (PAMG_E_STATE) until the solver is destroyed
    A->borrowed++;
    if (P) P->borrowed++;
    if (R) R->borrowed++;
    return PAMG_OK;
}

int pamg_solver_set_smoother(pamg_solver_t S, int level, int which, int kind, int iterations, double omega,
                             int sweep, const double *coeffs, int ncoeffs, const void *Dinv, int blocksize)
{
    if (!S || level < 0 || level >= (int)S->levels.size() || (which != 0 && which != 1)) return PAMG_E_ARG;
    if (S->finalized) return PAMG_E_STATE;
    if (kind < PAMG_SMOOTH_NONE || kind > PAMG_SMOOTH_BLOCK_GS || iterations < 0) return PAMG_E_ARG;
    if (sweep < PAMG_FORWARD || sweep > PAMG_SYMMETRIC) return PAMG_E_ARG;
    Level &L = S->levels[level];
    Smoother &sm = which == 0 ? L.pre : L.post;
    if (sm.d_Dinv) { hipFree(sm.d_Dinv); sm.d_Dinv = nullptr; }
    if (sm.AF) pamg_matrix_destroy(sm.AF);
    if (sm.AC) pamg_matrix_destroy(sm.AC);
    hipFree(sm.wF); hipFree(sm.wC); hipFree(sm.iF); hipFree(sm.iC); hipFree(sm.kw);
    if (sm.sw) pamg_schwarz_destroy(sm.sw);
    sm = Smoother();
    sm.kind = kind; sm.iterations = iterations; sm.omega = omega; sm.sweep = sweep; sm.blocksize = blocksize;
    if (kind == PAMG_SMOOTH_POLY) {
        if (!coeffs || ncoeffs < 1) return PAMG_E_ARG;
        sm.coeffs.assign(coeffs, coeffs + ncoeffs);
    }
    if (kind == PAMG_SMOOTH_BLOCK_JACOBI || kind == PAMG_SMOOTH_BLOCK_GS) {
        if (!Dinv || blocksize < 2 || blocksize != L.A->R || L.A->R != L.A->C) return PAMG_E_ARG;
        const size_t sz = (size_t)L.A->n_brow * blocksize * blocksize * tsize(S->dtype);
        PAMG_HIP(hipMalloc(&sm.d_Dinv, std::max<size_t>(sz, 256)));
        PAMG_HIP(hipMemcpy(sm.d_Dinv, Dinv, sz, hipMemcpyHostToDevice));
        S->bytes += sz;
    }
    if ((kind == PAMG_SMOOTH_JACOBI || kind == PAMG_SMOOTH_GS || kind == PAMG_SMOOTH_SOR) && L.A->R != L.A->C)
        return PAMG_E_ARG;                                     // "BSR blocks must be square"
    return PAMG_OK;
}

int pamg_solver_set_cf_smoother(pamg_solver_t S, int level, int which, int kind, int iterations, int f_iterations,
                                int c_iterations, double omega, const int32_t *Fpts, int nF, const int32_t *Cpts, int nC)
{
    if (!S || level < 0 || level >= (int)S->levels.size() || (which != 0 && which != 1)) return PAMG_E_ARG;
    if (S->finalized) return PAMG_E_STATE;
    if (kind != PAMG_SMOOTH_CF_JACOBI && kind != PAMG_SMOOTH_FC_JACOBI) return PAMG_E_ARG;
    if (iterations < 0 || f_iterations < 0 || c_iterations < 0 || nF < 0 || nC < 0) return PAMG_E_ARG;
    Level &L = S->levels[level];
    Smoother &sm = which == 0 ? L.pre : L.post;
    if (sm.d_Dinv) { hipFree(sm.d_Dinv); sm.d_Dinv = nullptr; }
    if (sm.AF) pamg_matrix_destroy(sm.AF);
    if (sm.AC) pamg_matrix_destroy(sm.AC);
    hipFree(sm.wF); hipFree(sm.wC); hipFree(sm.iF); hipFree(sm.iC); hipFree(sm.kw);
    if (sm.sw) pamg_schwarz_destroy(sm.sw);
    sm = Smoother();
    sm.kind = kind; sm.iterations = iterations; sm.omega = omega;
    sm.f_iterations = f_iterations; sm.c_iterations = c_iterations;
    PAMG_TRY(matrix_row_subset(L.A, Fpts, nF, &sm.AF));
    PAMG_TRY(matrix_row_subset(L.A, Cpts, nC, &sm.AC));
    const size_t ts = tsize(S->dtype);
    PAMG_HIP(hipMalloc(&sm.wF, std::max<size_t>((size_t)nF * ts, 256)));
    PAMG_HIP(hipMalloc(&sm.wC, std::max<size_t>((size_t)nC * ts, 256)));
    S->bytes += sm.AF->bytes + sm.AC->bytes + (size_t)(nF + nC) * ts;
    return PAMG_OK;
}

int pamg_solver_set_cf_block_smoother(pamg_solver_t S, int level, int which, int kind, int iterations, int f_iterations,
                                      int c_iterations, double omega, const void *Dinv, int blocksize, const int32_t *Fpts,
                                      int nF, const int32_t *Cpts, int nC)
{
    if (!S || level < 0 || level >= (int)S->levels.size() || (which != 0 && which != 1) || !Dinv) return PAMG_E_ARG;
    if (S->finalized) return PAMG_E_STATE;
    if (kind != PAMG_SMOOTH_CF_BLOCK_JACOBI && kind != PAMG_SMOOTH_FC_BLOCK_JACOBI) return PAMG_E_ARG;
    if (iterations < 0 || f_iterations < 0 || c_iterations < 0 || nF < 0 || nC < 0) return PAMG_E_ARG;
    Level &L = S->levels[level];
    if (L.A->R != L.A->C || L.A->R != blocksize || blocksize < 2) return PAMG_E_UNSUPPORTED;
    const int nb = L.A->n_brow;
    for (int k = 0; k < nF; ++k) if (Fpts[k] < 0 || Fpts[k] >= nb) return PAMG_E_ARG;
    for (int k = 0; k < nC; ++k) if (Cpts[k] < 0 || Cpts[k] >= nb) return PAMG_E_ARG;
    Smoother &sm = which == 0 ? L.pre : L.post;
    if (sm.d_Dinv) { hipFree(sm.d_Dinv); sm.d_Dinv = nullptr; }
    if (sm.AF) pamg_matrix_destroy(sm.AF);
    if (sm.AC) pamg_matrix_destroy(sm.AC);
    hipFree(sm.wF); hipFree(sm.wC); hipFree(sm.iF); hipFree(sm.iC); hipFree(sm.kw);
    if (sm.sw) pamg_schwarz_destroy(sm.sw);
    sm = Smoother();
    sm.kind = kind; sm.iterations = iterations; sm.omega = omega; sm.blocksize = blocksize;
    sm.f_iterations = f_iterations; sm.c_iterations = c_iterations;
    const size_t sz = (size_t)nb * blocksize * blocksize * tsize(S->dtype);
    PAMG_HIP(hipMalloc(&sm.d_Dinv, std::max<size_t>(sz, 256)));
    PAMG_HIP(hipMemcpy(sm.d_Dinv, Dinv, sz, hipMemcpyHostToDevice));
    auto expand = [&](const int32_t *pts, int n, int **dptr, int64_t *cnt) -> int {
        std::vector<int> idx((size_t)n * blocksize);
        for (int k = 0; k < n; ++k) for (int c = 0; c < blocksize; ++c) idx[(size_t)k * blocksize + c] = pts[k] * blocksize + c;
        *cnt = (int64_t)idx.size();
        PAMG_HIP(hipMalloc((void **)dptr, std::max<size_t>(idx.size() * sizeof(int), 256)));
        if (!idx.empty()) PAMG_HIP(hipMemcpy(*dptr, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice));
        return PAMG_OK;
    };
    PAMG_TRY(expand(Fpts, nF, &sm.iF, &sm.nF));
    PAMG_TRY(expand(Cpts, nC, &sm.iC, &sm.nC));
    S->bytes += sz + (size_t)(sm.nF + sm.nC) * sizeof(int);
    return PAMG_OK;
}

int pamg_solver_set_schwarz_smoother(pamg_solver_t S, int level, int which, int iterations, int sweep, pamg_matrix_t Ar,
                                     int nsub, const int32_t *Sp, const int32_t *Sj, const int32_t *Tp, const void *Tx)
{
    if (!S || level < 0 || level >= (int)S->levels.size() || (which != 0 && which != 1)) return PAMG_E_ARG;
    if (S->finalized) return PAMG_E_STATE;
    if (iterations < 0 || sweep < PAMG_FORWARD || sweep > PAMG_SYMMETRIC) return PAMG_E_ARG;
    Level &L = S->levels[level];
    pamg_matrix_s *Aop = Ar ? Ar : L.A;
    if (Aop->dtype != S->dtype || Aop->nrows != L.A->nrows || Aop->ncols != L.A->ncols) return PAMG_E_ARG;
    Smoother &sm = which == 0 ? L.pre : L.post;
    if (sm.d_Dinv) { hipFree(sm.d_Dinv); sm.d_Dinv = nullptr; }
    if (sm.AF) pamg_matrix_destroy(sm.AF);
    if (sm.AC) pamg_matrix_destroy(sm.AC);
    hipFree(sm.wF); hipFree(sm.wC); hipFree(sm.iF); hipFree(sm.iC); hipFree(sm.kw);
    if (sm.sw) pamg_schwarz_destroy(sm.sw);
    sm = Smoother();
    sm.kind = PAMG_SMOOTH_SCHWARZ; sm.iterations = iterations; sm.sweep = sweep;
    PAMG_TRY(pamg_schwarz_create(&sm.sw, Aop, nsub, Sp, Sj, Tp, Tx));
    PAMG_TRY(schwarz_prepare(sm.sw, sweep));           // the sweeps run inside a graph capture: no allocation there
    return PAMG_OK;
}

int pamg_solver_set_ne_smoother(pamg_solver_t S, int level, int which, int kind, int iterations, double omega,
                                int sweep, const void *Dinv, pamg_matrix_t At, pamg_matrix_t Ar)
{
    if (!S || level < 0 || level >= (int)S->levels.size() || (which != 0 && which != 1) || !Dinv) return PAMG_E_ARG;
    if (S->finalized) return PAMG_E_STATE;
    if (kind != PAMG_SMOOTH_GS_NE && kind != PAMG_SMOOTH_GS_NR && kind != PAMG_SMOOTH_JACOBI_NE) return PAMG_E_ARG;
    if (iterations < 0 || sweep < PAMG_FORWARD || sweep > PAMG_SYMMETRIC) return PAMG_E_ARG;
    Level &L = S->levels[level];
    if (L.A->R != 1 || L.A->C != 1) return PAMG_E_UNSUPPORTED;
    if (kind != PAMG_SMOOTH_GS_NE) {
        if (!At || At->dtype != S->dtype || At->R != 1 || At->C != 1 || At->nrows != L.A->ncols || At->ncols != L.A->nrows)
            return PAMG_E_ARG;
    }
    if (Ar && (Ar->dtype != S->dtype || Ar->nrows != L.A->nrows || Ar->ncols != L.A->ncols)) return PAMG_E_ARG;
    Smoother &sm = which == 0 ? L.pre : L.post;
    if (sm.d_Dinv) { hipFree(sm.d_Dinv); sm.d_Dinv = nullptr; }
    if (sm.AF) pamg_matrix_destroy(sm.AF);
    if (sm.AC) pamg_matrix_destroy(sm.AC);
    hipFree(sm.wF); hipFree(sm.wC); hipFree(sm.iF); hipFree(sm.iC); hipFree(sm.kw);
    if (sm.sw) pamg_schwarz_destroy(sm.sw);
    sm = Smoother();
    sm.kind = kind; sm.iterations = iterations; sm.omega = omega; sm.sweep = sweep;
    sm.At = kind == PAMG_SMOOTH_GS_NE ? nullptr : At;
    sm.Ar = Ar;                                            // the level's operator with sorted rows, where the reference's wrapper sees one
    const size_t sz = (size_t)L.A->nrows * tsize(S->dtype);
    PAMG_HIP(hipMalloc(&sm.d_Dinv, std::max<size_t>(sz, 256)));
    PAMG_HIP(hipMemcpy(sm.d_Dinv, Dinv, sz, hipMemcpyHostToDevice));
    S->bytes += sz;
    return PAMG_OK;
}

int pamg_solver_set_krylov_smoother(pamg_solver_t S, int level, int which, int method, double tol, int maxiter, int restart,
                                    pamg_matrix_t At)
{
    if (!S || level < 0 || level >= (int)S->levels.size() || (which != 0 && which != 1)) return PAMG_E_ARG;
    if (S->finalized) return PAMG_E_STATE;
    if (method < PAMG_KRYLOV_CG || method > PAMG_KRYLOV_CGNR || maxiter < 0 || restart < 0 || !(tol >= 0.0)) return PAMG_E_ARG;
    Level &L = S->levels[level];
    if (method == PAMG_KRYLOV_CGNE || method == PAMG_KRYLOV_CGNR) {
        if (!At || At->dtype != S->dtype || At->nrows != L.A->ncols || At->ncols != L.A->nrows) return PAMG_E_ARG;
    }
    Smoother &sm = which == 0 ? L.pre : L.post;
    if (sm.d_Dinv) { hipFree(sm.d_Dinv); sm.d_Dinv = nullptr; }
    if (sm.AF) pamg_matrix_destroy(sm.AF);
    if (sm.AC) pamg_matrix_destroy(sm.AC);
    hipFree(sm.wF); hipFree(sm.wC); hipFree(sm.iF); hipFree(sm.iC); hipFree(sm.kw);
    if (sm.sw) pamg_schwarz_destroy(sm.sw);
    sm = Smoother();
    sm.kind = PAMG_SMOOTH_KRYLOV; sm.iterations = 1;
    sm.kmethod = method; sm.ktol = tol; sm.kmaxiter = maxiter; sm.krestart = restart;
    sm.At = (method == PAMG_KRYLOV_CGNE || method == PAMG_KRYLOV_CGNR) ? At : nullptr;
    const size_t sz = 4 * (size_t)L.A->nrows * tsize(S->dtype);
    PAMG_HIP(hipMalloc(&sm.kw, std::max<size_t>(sz, 256)));
    S->bytes += sz;
    S->host_sync = true;
    return PAMG_OK;
}

// the cycle synchronises with the host (no graph capture) exactly when a host coarse solver or a Krylov smoother is installed
static void recompute_host_sync(pamg_solver_s *S)
{
    bool hs = S->coarse_host != nullptr;
    for (const Level &L : S->levels) hs = hs || L.pre.kind == PAMG_SMOOTH_KRYLOV || L.post.kind == PAMG_SMOOTH_KRYLOV;
    S->host_sync = hs;
}

int pamg_solver_set_coarse_dense(pamg_solver_t S, const void *M, int n_c)
{
    if (!S || n_c < 0) return PAMG_E_ARG;
    if (S->finalized) return PAMG_E_STATE;
    if (S->d_coarse) { hipFree(S->d_coarse); S->d_coarse = nullptr; }
    // the last coarse solver installed wins: a host callback / relaxation set earlier must not keep running
    S->coarse_host = nullptr; S->coarse_host_user = nullptr; S->coarse_relax = false;
    recompute_host_sync(S);
    S->n_c = n_c; S->coarse_set = true; S->coarse_zero = (M == nullptr);
    if (M && n_c > 0) {
        const size_t sz = (size_t)n_c * n_c * tsize(S->dtype);
        PAMG_HIP(hipMalloc(&S->d_coarse, std::max<size_t>(sz, 256)));
        PAMG_HIP(hipMemcpy(S->d_coarse, M, sz, hipMemcpyHostToDevice));
        S->bytes += sz;
    }
    return PAMG_OK;
}

int pamg_solver_set_coarse_host(pamg_solver_t S, pamg_coarse_host_fn fn, void *user, int n_c)
{
    if (!S || !fn || n_c < 1) return PAMG_E_ARG;
    if (S->finalized) return PAMG_E_STATE;
    S->coarse_host = fn; S->coarse_host_user = user;
    S->n_c = n_c; S->coarse_set = true; S->coarse_zero = false; S->coarse_relax = false;
    S->coarse_hb.assign((size_t)n_c * tsize(S->dtype), 0);
    S->coarse_hx.assign((size_t)n_c * tsize(S->dtype), 0);
    S->host_sync = true;                                        // the cycle synchronises with the host: no graph capture
    return PAMG_OK;
}

int pamg_solver_set_coarse_relax(pamg_solver_t S)
{
    if (!S || S->levels.empty()) return PAMG_E_ARG;
    if (S->finalized) return PAMG_E_STATE;
    if (S->levels.back().P) return PAMG_E_STATE;
    if (S->levels.back().pre.kind == PAMG_SMOOTH_NONE) return PAMG_E_ARG;
    S->coarse_relax = true; S->coarse_set = true; S->coarse_zero = false;
    S->coarse_host = nullptr; S->coarse_host_user = nullptr;
    recompute_host_sync(S);
    S->n_c = (int)S->levels.back().n;
    return PAMG_OK;
}

int pamg_solver_finalize(pamg_solver_t S)
{
    if (!S || S->levels.empty()) return PAMG_E_ARG;
    if (S->finalized) return PAMG_OK;
    if (S->levels.back().P) return PAMG_E_STATE;               // last level must be the coarsest
    if (!S->coarse_set || S->n_c != S->levels.back().n) return PAMG_E_STATE;
    const size_t ts = tsize(S->dtype);
    const int nlev = (int)S->levels.size();
    for (int l = 0; l < nlev; ++l) {
        Level &L = S->levels[l];
        const size_t vb = (size_t)L.n * ts;
        PAMG_TRY(dalloc(S, &L.x, vb));
        PAMG_TRY(dalloc(S, &L.xalt, vb));
        PAMG_TRY(dalloc(S, &L.b, vb));
        L.x_home = L.x;
        if (l < nlev - 1 || S->coarse_relax) {
            PAMG_TRY(dalloc(S, &L.r, vb));
            if (L.pre.kind == PAMG_SMOOTH_POLY || L.post.kind == PAMG_SMOOTH_POLY) PAMG_TRY(dalloc(S, &L.work, 3 * vb));
        }
    }
    const int nsm = S->coarse_relax ? nlev : nlev - 1;      // levels that carry a relaxation method
    for (int l = 0; l < nsm; ++l) {
        // an operator swept by SOR in either slot keeps the unmerged lane layout (prebuild_schedules): decided from both smoothers
        // BEFORE the jobs build anything -- a merged layout built first would leave SOR to a lazy build at its first sweep
        Level &L = S->levels[l];
        if ((sor_takes_omega(L.A, L.pre) || sor_takes_omega(L.A, L.post)) && L.A->lane_merge == 0) L.A->lane_merge = 1;
    }
    {
        std::vector<SchedJob> jobs;
        for (int l = 0; l < nsm; ++l) {
            Level &L = S->levels[l];
            // a level the dense form claims builds no zero-iterate plans: they would never run
            sched_jobs_of(L, L.pre, jobs, zero_plans_wanted(L.A, L.pre, L.post, l) && !dtri_claims(L.A, dtri_sweeps(L.pre, L.post), dtri_automatic(L.pre, L.post, l)));
            sched_jobs_of(L, L.post, jobs);
        }
        PAMG_TRY(run_sched_jobs(jobs));
    }
    for (int l = 0; l < nsm; ++l) {            // whatever the jobs did not cover (Kaczmarz line schedules); the rest is found built
        Level &L = S->levels[l];
        PAMG_TRY(ensure_dtri(L.A, dtri_sweeps(L.pre, L.post), dtri_automatic(L.pre, L.post, l)));        // the block inverses (device kernels; where its planner declines, the zero-iterate plans are built below)
        PAMG_TRY(prebuild_schedules(L, L.pre, zero_plans_wanted(L.A, L.pre, L.post, l) && !L.A->dtri));
        PAMG_TRY(prebuild_schedules(L, L.post));
    }
    PAMG_TRY(dalloc(S, (void **)&S->d_slot, 16 * sizeof(double)));
    PAMG_TRY(dalloc(S, (void **)&S->d_scratch, 1032 * sizeof(double)));
    PAMG_HIP(hipStreamCreateWithFlags(&S->own_stream, hipStreamNonBlocking));
    S->finalized = true;
    tail_choose(S);                                            // the operators themselves: at the first cycle of each kind (ensure_tail)
    return PAMG_OK;
}

int pamg_solver_set_graph(pamg_solver_t S, int enable)
{
    if (!S) return PAMG_E_ARG;
    S->use_graph = enable != 0;
    if (!S->use_graph) drop_graphs(S);
    return PAMG_OK;
}

int pamg_solver_cycle(pamg_solver_t S, void *x, const void *b, int cycle, int cycles_per_level, pamg_stream_t s_)
{
    if (!S || !x || !b) return PAMG_E_ARG;
    if (!S->finalized) return PAMG_E_STATE;
    if (cycle < PAMG_CYCLE_V || cycle > PAMG_CYCLE_AMLI || cycles_per_level < 1 || cycles_per_level > 1023) return PAMG_E_ARG;
    hipStream_t s = s_ ? (hipStream_t)s_ : S->own_stream;
    PAMG_TRY(ensure_amli(S, cycle));
    if (!s_) PAMG_HIP(hipStreamSynchronize(nullptr));   // inputs may have been produced on the default stream
    Level &L0 = S->levels[0];
    const size_t vb = (size_t)L0.n * tsize(S->dtype);
    PAMG_HIP(hipMemcpyAsync(L0.x, x, vb, hipMemcpyDeviceToDevice, s));
    PAMG_HIP(hipMemcpyAsync(L0.b, b, vb, hipMemcpyDeviceToDevice, s));
    PAMG_TRY(run_cycle(S, cycle, cycles_per_level, s));
    PAMG_HIP(hipMemcpyAsync(x, L0.x, vb, hipMemcpyDeviceToDevice, s));
    if (!s_) PAMG_HIP(hipStreamSynchronize(s));
    return PAMG_OK;
}

}  // extern "C"

namespace pamg {
// one cycle on DEVICE x, b as part of a caller's stream-ordered sequence (the collapsed part of the sharded cycle,
// pamg_dist.hip): no synchronisation, no convergence-check norm; allow_graph = false launches the kernels one by one
// (the caller is capturing the stream into a graph of its own)
int solver_cycle_inline(pamg_solver_s *S, void *x, const void *b, int cycle, int cpl, hipStream_t s, bool allow_graph)
{
    if (!S || !x || !b || !s) return PAMG_E_ARG;
    if (!S->finalized) return PAMG_E_STATE;
    if (cycle == PAMG_CYCLE_AMLI) return PAMG_E_UNSUPPORTED;     // its work vectors are allocated on first use
    S->tail.dist = true;                                         // the dense tail is the resident solver's: here the launches stay
    S->tail.active = false;
    Level &L0 = S->levels[0];
    const size_t vb = (size_t)L0.n * tsize(S->dtype);
    PAMG_HIP(hipMemcpyAsync(L0.x, x, vb, hipMemcpyDeviceToDevice, s));
    PAMG_HIP(hipMemcpyAsync(L0.b, b, vb, hipMemcpyDeviceToDevice, s));
    if (allow_graph) PAMG_TRY(run_cycle(S, cycle, cpl, s, false, false));
    else PAMG_TRY(enqueue_cycle(S, cycle, cpl, false, false, s));
    PAMG_HIP(hipMemcpyAsync(x, L0.x, vb, hipMemcpyDeviceToDevice, s));
    return PAMG_OK;
}

// true when a cycle of S reads scalars back on the host (Krylov smoothers / coarse solvers): such a cycle cannot be
// part of somebody else's stream capture either (the sharded driver asks before capturing an iteration)
bool solver_needs_host_sync(const pamg_solver_s *S) { return S && S->host_sync; }
}  // namespace pamg

extern "C" {

int pamg_solver_solve(pamg_solver_t S, void *x, const void *b, double tol, int maxiter, int cycle,
                      int cycles_per_level, int check_every, double *residuals, int *n_iter, int *info,
                      pamg_stream_t s_)
{
    if (!S || !x || !b || maxiter < 1 || check_every < 1) return PAMG_E_ARG;
    if (!S->finalized) return PAMG_E_STATE;
    if (cycle < PAMG_CYCLE_V || cycle > PAMG_CYCLE_AMLI || cycles_per_level < 1 || cycles_per_level > 1023) return PAMG_E_ARG;
    hipStream_t s = s_ ? (hipStream_t)s_ : S->own_stream;
    PAMG_TRY(ensure_amli(S, cycle));
    if (!s_) PAMG_HIP(hipStreamSynchronize(nullptr));   // inputs may have been produced on the default stream
    Level &L0 = S->levels[0];
    const size_t vb = (size_t)L0.n * tsize(S->dtype);
    if (S->norms_cap < maxiter + 2) {
        if (S->d_norms) hipFree(S->d_norms);
        S->norms_cap = maxiter + 2;
        PAMG_HIP(hipMalloc((void **)&S->d_norms, sizeof(double) * (size_t)S->norms_cap));
    }
    PAMG_HIP(hipMemcpyAsync(L0.x, x, vb, hipMemcpyDeviceToDevice, s));
    PAMG_HIP(hipMemcpyAsync(L0.b, b, vb, hipMemcpyDeviceToDevice, s));
    // normb and the initial residual (multilevel.py:540-547)
    PAMG_TRY(vec_sumsq(S->dtype, L0.n, L0.b, S->d_scratch, S->d_slot + 1, s));
    PAMG_TRY(stream_launch(L0.A, EPI_SUMSQ, L0.x, L0.b, nullptr, 0.0, 0.0, L0.A->d_partial, s));
    PAMG_TRY(reduce_partials(L0.A->d_partial, L0.A->nblk, S->d_slot, s));
    double h2[2] = {0.0, 0.0};
    PAMG_HIP(hipMemcpyAsync(h2, S->d_slot, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    PAMG_HIP(hipStreamSynchronize(s));
    double normb = std::sqrt(h2[1]);
    if (normb == 0.0) normb = 1.0;
    if (residuals) residuals[0] = std::sqrt(h2[0]);
    std::vector<double> hn((size_t)maxiter + 1, 0.0);
    int it = 0, checked = 0, converged_at = -1;
    while (true) {
        PAMG_TRY(run_cycle(S, cycle, cycles_per_level, s));
        PAMG_HIP(hipMemcpyAsync(S->d_norms + it, S->d_slot, sizeof(double), hipMemcpyDeviceToDevice, s));
        ++it;
        if (it % check_every == 0 || it == maxiter) {
            PAMG_HIP(hipMemcpyAsync(hn.data() + checked, S->d_norms + checked, sizeof(double) * (size_t)(it - checked),
                                    hipMemcpyDeviceToHost, s));
            PAMG_HIP(hipStreamSynchronize(s));
            for (int k = checked; k < it; ++k) {
                const double nr = std::sqrt(hn[k]);
                if (residuals) residuals[k + 1] = nr;
                if (converged_at < 0 && nr < tol * normb) converged_at = k + 1;
            }
            checked = it;
            if (converged_at >= 0) break;
        }
        if (it == maxiter) break;
    }
    PAMG_HIP(hipStreamSynchronize(s));
    const int swept = check_sweeps(S);
    if (swept == PAMG_E_TIMEOUT && S->fallbacks == 0) {
        // the iterate is invalid; the caller's x still holds the initial guess: switch schedulers and run the solve again
        PAMG_TRY(fall_back_to_level_launches(S));
        return pamg_solver_solve(S, x, b, tol, maxiter, cycle, cycles_per_level, check_every, residuals, n_iter, info, s_);
    }
    PAMG_HIP(hipMemcpyAsync(x, L0.x, vb, hipMemcpyDeviceToDevice, s));
    PAMG_HIP(hipStreamSynchronize(s));
    if (n_iter) *n_iter = it;
    if (info) *info = converged_at >= 0 ? 0 : it;
    return swept;
}

int pamg_solver_load(pamg_solver_t S, const void *x, const void *b, pamg_stream_t s_)
{
    if (!S || !x || !b) return PAMG_E_ARG;
    if (!S->finalized) return PAMG_E_STATE;
    hipStream_t s = s_ ? (hipStream_t)s_ : S->own_stream;
    if (!s_) PAMG_HIP(hipStreamSynchronize(nullptr));   // inputs may have been produced on the default stream
    Level &L0 = S->levels[0];
    const size_t vb = (size_t)L0.n * tsize(S->dtype);
    PAMG_HIP(hipMemcpyAsync(L0.x, x, vb, hipMemcpyDeviceToDevice, s));
    PAMG_HIP(hipMemcpyAsync(L0.b, b, vb, hipMemcpyDeviceToDevice, s));
    return PAMG_OK;
}

int pamg_solver_iterate(pamg_solver_t S, int k, int cycle, int cycles_per_level, double *residuals, pamg_stream_t s_)
{
    if (!S || k < 0) return PAMG_E_ARG;
    if (!S->finalized) return PAMG_E_STATE;
    if (cycle < PAMG_CYCLE_V || cycle > PAMG_CYCLE_AMLI || cycles_per_level < 1 || cycles_per_level > 1023) return PAMG_E_ARG;
    hipStream_t s = s_ ? (hipStream_t)s_ : S->own_stream;
    PAMG_TRY(ensure_amli(S, cycle));
    if (residuals && S->norms_cap < k + 2) {
        if (S->d_norms) hipFree(S->d_norms);
        S->norms_cap = k + 2;
        PAMG_HIP(hipMalloc((void **)&S->d_norms, sizeof(double) * (size_t)S->norms_cap));
    }
    for (int it = 0; it < k; ++it) {
        PAMG_TRY(run_cycle(S, cycle, cycles_per_level, s));
        if (residuals)
            PAMG_HIP(hipMemcpyAsync(S->d_norms + it, S->d_slot, sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    if (residuals && k > 0) {
        PAMG_HIP(hipMemcpyAsync(residuals, S->d_norms, sizeof(double) * (size_t)k, hipMemcpyDeviceToHost, s));
        PAMG_HIP(hipStreamSynchronize(s));
        for (int it = 0; it < k; ++it) residuals[it] = std::sqrt(residuals[it]);
        const int swept = check_sweeps(S);
        // the resident iterate cannot be restored here: report, but make the NEXT load / iterate safe
        if (swept == PAMG_E_TIMEOUT && S->fallbacks == 0) PAMG_TRY(fall_back_to_level_launches(S));
        return swept;
    }
    return PAMG_OK;
}

int pamg_solver_store(pamg_solver_t S, void *x, pamg_stream_t s_)
{
    if (!S || !x) return PAMG_E_ARG;
    if (!S->finalized) return PAMG_E_STATE;
    hipStream_t s = s_ ? (hipStream_t)s_ : S->own_stream;
    Level &L0 = S->levels[0];
    PAMG_HIP(hipMemcpyAsync(x, L0.x, (size_t)L0.n * tsize(S->dtype), hipMemcpyDeviceToDevice, s));
    return (int)hipStreamSynchronize(s);
}

int pamg_solver_stream(pamg_solver_t S, pamg_stream_t *s)
{
    if (!S || !s) return PAMG_E_ARG;
    if (!S->finalized) return PAMG_E_STATE;
    *s = (pamg_stream_t)S->own_stream;
    return PAMG_OK;
}

// Preconditioned conjugate gradients with the resident cycle as preconditioner, entirely on
// the device (reference: pyamg/krylov/_cg.py:98-198 with criteria 'rr', driven by
// MultilevelSolver.solve(accel='cg'), multilevel.py:479-535).  z = M r is exactly one cycle
// from a zero initial guess (multilevel.py:390-396) without the two wasted fine-level
// residual norms of the reference's matvec.  Only the scalars cross PCIe.
int pamg_solver_pcg(pamg_solver_t S, void *x, const void *b, double tol, int maxiter, int cycle,
                    int cycles_per_level, double *residuals, int *n_iter, int *info, pamg_stream_t s_)
{
    if (!S || !x || !b || maxiter < 1) return PAMG_E_ARG;
    if (!S->finalized) return PAMG_E_STATE;
    if (cycle < PAMG_CYCLE_V || cycle > PAMG_CYCLE_AMLI || cycles_per_level < 1 || cycles_per_level > 1023) return PAMG_E_ARG;
    hipStream_t s = s_ ? (hipStream_t)s_ : S->own_stream;
    PAMG_TRY(ensure_amli(S, cycle));
    if (!s_) PAMG_HIP(hipStreamSynchronize(nullptr));
    Level &L0 = S->levels[0];
    const int64_t n = L0.n;
    const size_t vb = (size_t)n * tsize(S->dtype);
    if (!S->cg_p) { PAMG_TRY(dalloc(S, &S->cg_p, vb)); PAMG_TRY(dalloc(S, &S->cg_q, vb)); }
    // CG's residual LIVES in the fine level's right-hand side and its preconditioned residual in the fine level's iterate: z = M r is then
    // "x = 0, one cycle" with nothing copied in or out (three full-vector passes per iteration around the cycle)
    const std::function<int(const void *, void *)> precond = [&](const void *rin, void *zout) -> int {   // z = M r: one cycle from x = 0
        if (rin != L0.b) PAMG_HIP(hipMemcpyAsync(L0.b, rin, vb, hipMemcpyDeviceToDevice, s));
        PAMG_HIP(hipMemsetAsync(L0.x, 0, vb, s));
        PAMG_TRY(run_cycle(S, cycle, cycles_per_level, s, false, true));
        if (zout != L0.x) PAMG_HIP(hipMemcpyAsync(zout, L0.x, vb, hipMemcpyDeviceToDevice, s));
        return PAMG_OK;
    };
    PAMG_TRY(cg_core(S, L0.A, n, &precond, L0.b, L0.x, S->cg_p, S->cg_q, x, b, tol, maxiter, residuals, n_iter, info, s));
    PAMG_HIP(hipStreamSynchronize(s));
    return check_sweeps(S);
}

static int krylov_accel(pamg_solver_t S, bool flexible, void *x, const void *b, double tol, int maxiter, int restart, int cycle,
                        int cycles_per_level, double *residuals, int residuals_cap, int *n_res, int *n_iter, int *info, pamg_stream_t s_)
{
    if (!S || !x || !b) return PAMG_E_ARG;
    if (!S->finalized) return PAMG_E_STATE;
    if (cycle < PAMG_CYCLE_V || cycle > PAMG_CYCLE_AMLI || cycles_per_level < 1 || cycles_per_level > 1023) return PAMG_E_ARG;
    hipStream_t s = s_ ? (hipStream_t)s_ : S->own_stream;
    PAMG_TRY(ensure_amli(S, cycle));
    if (!s_) PAMG_HIP(hipStreamSynchronize(nullptr));
    PAMG_TRY(krylov_householder(S, S->levels[0].A, S->levels[0].n, flexible, x, b, tol, maxiter, restart, cycle, cycles_per_level,
                                residuals, residuals_cap, n_res, n_iter, info, s));
    return check_sweeps(S);
}

int pamg_solver_fgmres(pamg_solver_t S, void *x, const void *b, double tol, int maxiter, int restart, int cycle,
                       int cycles_per_level, double *residuals, int residuals_cap, int *n_res, int *n_iter,
                       int *info, pamg_stream_t s)
{
    return krylov_accel(S, true, x, b, tol, maxiter, restart, cycle, cycles_per_level, residuals, residuals_cap,
                        n_res, n_iter, info, s);
}

int pamg_solver_gmres(pamg_solver_t S, void *x, const void *b, double tol, int maxiter, int restart, int cycle,
                      int cycles_per_level, double *residuals, int residuals_cap, int *n_res, int *n_iter,
                      int *info, pamg_stream_t s)
{
    return krylov_accel(S, false, x, b, tol, maxiter, restart, cycle, cycles_per_level, residuals, residuals_cap,
                        n_res, n_iter, info, s);
}

int pamg_solver_krylov(pamg_solver_t S, int method, void *x, const void *b, double tol, int maxiter, int cycle, int cycles_per_level,
                       double *residuals, int residuals_cap, int *n_res, int *n_iter, int *info, pamg_stream_t s_)
{
    if (!S || !x || !b) return PAMG_E_ARG;
    if (!S->finalized) return PAMG_E_STATE;
    if (cycle < PAMG_CYCLE_V || cycle > PAMG_CYCLE_AMLI || cycles_per_level < 1 || cycles_per_level > 1023) return PAMG_E_ARG;
    if (method < PAMG_ACCEL_BICGSTAB || method > PAMG_ACCEL_MINIMAL_RESIDUAL) return PAMG_E_ARG;
    Level &L0 = S->levels[0];
    const int64_t n = L0.n;
    if (n < 2) return PAMG_E_UNSUPPORTED;              // the reference special-cases n == 1 (bicgstab) on the host
    static const int nvec[4] = {5, 3, 1, 1};           // work vectors per method
    if (maxiter <= 0) {                                // the methods' own defaults
        const int64_t d = method == PAMG_ACCEL_BICGSTAB ? n + 5 : method == PAMG_ACCEL_STEEPEST_DESCENT ? n : (int64_t)(1.3 * (double)n) + 2;
        maxiter = (int)std::min<int64_t>(d, INT32_MAX);
    }
    hipStream_t s = s_ ? (hipStream_t)s_ : S->own_stream;
    PAMG_TRY(ensure_amli(S, cycle));
    if (!s_) PAMG_HIP(hipStreamSynchronize(nullptr));
    const size_t vb = (size_t)n * tsize(S->dtype);
    for (int k = 0; k < nvec[method]; ++k)
        if (!S->kr_v[k]) PAMG_TRY(dalloc(S, &S->kr_v[k], vb));
    if (!S->kr_red) PAMG_TRY(dalloc(S, (void **)&S->kr_red, sizeof(double) * (KR_PARTIALS + 16)));
    KrylovRun K{S, L0, S->dtype, n, vb, cycle, cycles_per_level, s, S->kr_red, S->kr_red + KR_PARTIALS, residuals, residuals_cap};
    int it = 0, inf = 0, st = PAMG_OK;
    switch (method) {
        case PAMG_ACCEL_BICGSTAB: st = bicgstab_core(K, x, b, tol, maxiter, it, inf); break;
        case PAMG_ACCEL_CR: st = cr_core(K, x, b, tol, maxiter, it, inf); break;
        case PAMG_ACCEL_STEEPEST_DESCENT: st = sd_core(K, x, b, tol, maxiter, it, inf); break;
        default: st = mr_core(K, x, b, tol, maxiter, it, inf); break;
    }
    PAMG_HIP(hipStreamSynchronize(s));
    PAMG_TRY(st);
    if (n_res) *n_res = K.nres;
    if (n_iter) *n_iter = it;
    if (info) *info = inf;
    return check_sweeps(S);
}

int pamg_solver_stats(pamg_solver_t S, int64_t stats[8])
{
    if (!S || !stats) return PAMG_E_ARG;
    for (int k = 0; k < 8; ++k) stats[k] = 0;
    stats[0] = (int64_t)S->levels.size();
    size_t bytes = S->bytes;
    int64_t launches = 0;
    for (const Level &L : S->levels) {
        bytes += L.A->bytes + (L.P ? L.P->bytes : 0) + (L.R ? L.R->bytes : 0);
        for (int k = 0; k < 4; ++k) if (L.A->gs[k]) launches += L.A->gs[k]->nlevels;
    }
    stats[1] = launches;           // GS level launches per directional sweep pair (informative)
    stats[2] = (int64_t)bytes;
    stats[3] = (int64_t)S->graphs.size();
    stats[4] = S->fallbacks;
    stats[5] = -1; stats[6] = 0;   // (round 3's hierarchy tail in one launch: retired in round 5 -- slower than the replayed graph of small launches)
    return PAMG_OK;
}

int pamg_solver_dense_tail(pamg_solver_t S, int mode, int max_rows)
{
    if (!S || mode < 0 || mode > 2 || max_rows < 0) return PAMG_E_ARG;
    S->tail.mode = mode;
    S->tail.max_rows = max_rows == 0 ? DENSE_TAIL_MAX_ROWS : max_rows;
    if (S->finalized) tail_choose(S);                          // (drops the operators and the graphs that hold their launches)
    return PAMG_OK;
}

int pamg_solver_dense_tail_info(pamg_solver_t S, int64_t info[16], double figures[2])
{
    if (!S || !info) return PAMG_E_ARG;
    const DenseTail &T = S->tail;
    for (int k = 0; k < 16; ++k) info[k] = 0;
    info[0] = (int64_t)T.ops.size();
    info[1] = T.declined;
    info[2] = T.level;
    info[3] = T.level >= 0 ? S->levels[T.level].n : 0;
    info[4] = (int64_t)T.bytes;
    info[5] = T.applications;
    info[6] = T.mode;
    info[7] = T.max_rows;
    if (figures) { figures[0] = T.tab_ms; figures[1] = T.guard; }
    return PAMG_OK;
}

}  // extern "C"
