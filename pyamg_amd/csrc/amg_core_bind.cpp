// amg_core_bind.cpp -- the pybind11 face of Layer 1: a module with the names, argument order and overload behaviour
// of the reference's pyamg.amg_core relaxation bindings (pyamg/amg_core/relaxation_bind.cpp:681-715: one overload per
// value type, every array `.noconvert()` so a dtype mismatch is a TypeError, sizes taken from the arrays) whose
// bodies do nothing but hand the host pointers to the C ABI of libpyamg_amd.so (include/pyamg_amd.h, pamg_*_f32 /
// pamg_*_f64).  Plain g++ builds it (no HIP here); pyamg_amd/amg_core.py is the ctypes twin of the same surface.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pyamg_amd.h"

namespace py = pybind11;

namespace {

using Idx = py::array_t<int32_t, py::array::c_style>;
template <typename T> using Vec = py::array_t<T, py::array::c_style>;

void done(int status, const char *what)
{
    if (status != PAMG_OK) throw std::runtime_error(std::string(what) + ": pyamg_amd status " + std::to_string(status));
}

template <typename A> int len(const A &a) { return (int)a.size(); }

// the C entry points of one value type
template <typename T> struct L1;
#define PAMG_L1(T, S)                                                                      \
    template <> struct L1<T> {                                                             \
        static constexpr auto csr_matvec = pamg_csr_matvec_##S;                            \
        static constexpr auto bsr_matvec = pamg_bsr_matvec_##S;                            \
        static constexpr auto gauss_seidel = pamg_gauss_seidel_##S;                        \
        static constexpr auto sor_gauss_seidel = pamg_sor_gauss_seidel_##S;                \
        static constexpr auto bsr_gauss_seidel = pamg_bsr_gauss_seidel_##S;                \
        static constexpr auto jacobi = pamg_jacobi_##S;                                    \
        static constexpr auto bsr_jacobi = pamg_bsr_jacobi_##S;                            \
        static constexpr auto jacobi_indexed = pamg_jacobi_indexed_##S;                    \
        static constexpr auto gauss_seidel_ne = pamg_gauss_seidel_ne_##S;                  \
        static constexpr auto gauss_seidel_nr = pamg_gauss_seidel_nr_##S;                  \
        static constexpr auto jacobi_ne = pamg_jacobi_ne_##S;                              \
        static constexpr auto block_jacobi = pamg_block_jacobi_##S;                        \
        static constexpr auto block_gauss_seidel = pamg_block_gauss_seidel_##S;            \
        static constexpr auto block_jacobi_indexed = pamg_block_jacobi_indexed_##S;        \
        static constexpr auto gauss_seidel_indexed = pamg_gauss_seidel_indexed_##S;        \
        static constexpr auto overlapping_schwarz_csr = pamg_overlapping_schwarz_csr_##S;  \
        static constexpr auto pinv_array = pamg_pinv_array_##S;                            \
        static constexpr auto extract_subblocks = pamg_extract_subblocks_##S;              \
        static constexpr auto fit_candidates = pamg_fit_candidates_##S;                    \
    };
PAMG_L1(double, f64)
PAMG_L1(float, f32)
#undef PAMG_L1

template <typename T>
void bind(py::module_ &m)
{
    using F = L1<T>;
    auto nc = [](const char *n) { return py::arg(n).noconvert(); };
    m.def("csr_matvec", [](int n_row, int n_col, Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &Xx, Vec<T> &Yx) {
        done(F::csr_matvec(n_row, n_col, Ap.data(), Aj.data(), Ax.data(), Xx.data(), Yx.mutable_data()), "csr_matvec");
    }, py::arg("n_row"), py::arg("n_col"), nc("Ap"), nc("Aj"), nc("Ax"), nc("Xx"), nc("Yx"));
    m.def("bsr_matvec", [](int n_brow, int n_bcol, int R, int C, Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &Xx, Vec<T> &Yx) {
        done(F::bsr_matvec(n_brow, n_bcol, R, C, Ap.data(), Aj.data(), Ax.data(), Xx.data(), Yx.mutable_data()), "bsr_matvec");
    }, py::arg("n_brow"), py::arg("n_bcol"), py::arg("R"), py::arg("C"), nc("Ap"), nc("Aj"), nc("Ax"), nc("Xx"), nc("Yx"));
    m.def("gauss_seidel", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &x, Vec<T> &b, int row_start, int row_stop, int row_step) {
        done(F::gauss_seidel(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), x.mutable_data(), len(x), b.data(), len(b),
                             row_start, row_stop, row_step), "gauss_seidel");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("x"), nc("b"), py::arg("row_start"), py::arg("row_stop"), py::arg("row_step"));
    m.def("sor_gauss_seidel", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &x, Vec<T> &b, int row_start, int row_stop, int row_step, T omega) {
        done(F::sor_gauss_seidel(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), x.mutable_data(), len(x), b.data(), len(b),
                                 row_start, row_stop, row_step, omega), "sor_gauss_seidel");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("x"), nc("b"), py::arg("row_start"), py::arg("row_stop"), py::arg("row_step"), py::arg("omega"));
    m.def("bsr_gauss_seidel", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &x, Vec<T> &b, int row_start, int row_stop, int row_step, int blocksize) {
        done(F::bsr_gauss_seidel(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), x.mutable_data(), len(x), b.data(), len(b),
                                 row_start, row_stop, row_step, blocksize), "bsr_gauss_seidel");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("x"), nc("b"), py::arg("row_start"), py::arg("row_stop"), py::arg("row_step"), py::arg("blocksize"));
    m.def("jacobi", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &x, Vec<T> &b, Vec<T> &temp, int row_start, int row_stop, int row_step, Vec<T> &omega) {
        done(F::jacobi(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), x.mutable_data(), len(x), b.data(), len(b),
                       temp.mutable_data(), len(temp), row_start, row_stop, row_step, omega.data(), len(omega)), "jacobi");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("x"), nc("b"), nc("temp"), py::arg("row_start"), py::arg("row_stop"), py::arg("row_step"), nc("omega"));
    m.def("bsr_jacobi", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &x, Vec<T> &b, Vec<T> &temp, int row_start, int row_stop, int row_step,
                           int blocksize, Vec<T> &omega) {
        done(F::bsr_jacobi(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), x.mutable_data(), len(x), b.data(), len(b),
                           temp.mutable_data(), len(temp), row_start, row_stop, row_step, blocksize, omega.data(), len(omega)), "bsr_jacobi");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("x"), nc("b"), nc("temp"), py::arg("row_start"), py::arg("row_stop"), py::arg("row_step"),
       py::arg("blocksize"), nc("omega"));
    m.def("jacobi_indexed", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &x, Vec<T> &b, Idx &indices, Vec<T> &omega) {
        done(F::jacobi_indexed(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), x.mutable_data(), len(x), b.data(), len(b),
                               indices.data(), len(indices), omega.data(), len(omega)), "jacobi_indexed");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("x"), nc("b"), nc("indices"), nc("omega"));
    m.def("gauss_seidel_ne", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &x, Vec<T> &b, int row_start, int row_stop, int row_step, Vec<T> &Tx, T omega) {
        done(F::gauss_seidel_ne(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), x.mutable_data(), len(x), b.data(), len(b),
                                row_start, row_stop, row_step, Tx.data(), len(Tx), omega), "gauss_seidel_ne");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("x"), nc("b"), py::arg("row_start"), py::arg("row_stop"), py::arg("row_step"), nc("Tx"), py::arg("omega"));
    m.def("gauss_seidel_nr", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &x, Vec<T> &z, int col_start, int col_stop, int col_step, Vec<T> &Tx, T omega) {
        done(F::gauss_seidel_nr(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), x.mutable_data(), len(x), z.mutable_data(), len(z),
                                col_start, col_stop, col_step, Tx.data(), len(Tx), omega), "gauss_seidel_nr");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("x"), nc("z"), py::arg("col_start"), py::arg("col_stop"), py::arg("col_step"), nc("Tx"), py::arg("omega"));
    m.def("jacobi_ne", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &x, Vec<T> &b, Vec<T> &Tx, Vec<T> &temp, int row_start, int row_stop, int row_step,
                          Vec<T> &omega) {
        done(F::jacobi_ne(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), x.mutable_data(), len(x), b.data(), len(b),
                          Tx.data(), len(Tx), temp.mutable_data(), len(temp), row_start, row_stop, row_step, omega.data(), len(omega)), "jacobi_ne");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("x"), nc("b"), nc("Tx"), nc("temp"), py::arg("row_start"), py::arg("row_stop"), py::arg("row_step"), nc("omega"));
    m.def("block_jacobi", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &x, Vec<T> &b, Vec<T> &Tx, Vec<T> &temp, int row_start, int row_stop, int row_step,
                             Vec<T> &omega, int blocksize) {
        done(F::block_jacobi(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), x.mutable_data(), len(x), b.data(), len(b),
                             Tx.data(), len(Tx), temp.mutable_data(), len(temp), row_start, row_stop, row_step, omega.data(), len(omega),
                             blocksize), "block_jacobi");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("x"), nc("b"), nc("Tx"), nc("temp"), py::arg("row_start"), py::arg("row_stop"), py::arg("row_step"),
       nc("omega"), py::arg("blocksize"));
    m.def("overlapping_schwarz_csr", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &x, Vec<T> &b, Vec<T> &Tx, Idx &Tp, Idx &Sj, Idx &Sp, int nsdomains,
                                        int nrows, int row_start, int row_stop, int row_step) {
        done(F::overlapping_schwarz_csr(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), x.mutable_data(), len(x), b.data(), len(b),
                                        Tx.data(), len(Tx), Tp.data(), len(Tp), Sj.data(), len(Sj), Sp.data(), len(Sp), nsdomains, nrows,
                                        row_start, row_stop, row_step), "overlapping_schwarz_csr");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("x"), nc("b"), nc("Tx"), nc("Tp"), nc("Sj"), nc("Sp"), py::arg("nsdomains"), py::arg("nrows"),
       py::arg("row_start"), py::arg("row_stop"), py::arg("row_step"));
    m.def("extract_subblocks", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &Tx, Idx &Tp, Idx &Sj, Idx &Sp, int nsdomains, int nrows) {
        done(F::extract_subblocks(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), Tx.mutable_data(), len(Tx), Tp.data(), len(Tp),
                                  Sj.data(), len(Sj), Sp.data(), len(Sp), nsdomains, nrows), "extract_subblocks");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("Tx"), nc("Tp"), nc("Sj"), nc("Sp"), py::arg("nsdomains"), py::arg("nrows"));
    m.def("gauss_seidel_indexed", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &x, Vec<T> &b, Idx &Id, int row_start, int row_stop, int row_step) {
        done(F::gauss_seidel_indexed(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), x.mutable_data(), len(x), b.data(), len(b),
                                     Id.data(), len(Id), row_start, row_stop, row_step), "gauss_seidel_indexed");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("x"), nc("b"), nc("Id"), py::arg("row_start"), py::arg("row_stop"), py::arg("row_step"));
    m.def("block_jacobi_indexed", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &x, Vec<T> &b, Vec<T> &Tx, Idx &indices, Vec<T> &omega, int blocksize) {
        done(F::block_jacobi_indexed(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), x.mutable_data(), len(x), b.data(), len(b),
                                     Tx.data(), len(Tx), indices.data(), len(indices), omega.data(), len(omega), blocksize), "block_jacobi_indexed");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("x"), nc("b"), nc("Tx"), nc("indices"), nc("omega"), py::arg("blocksize"));
    m.def("block_gauss_seidel", [](Idx &Ap, Idx &Aj, Vec<T> &Ax, Vec<T> &x, Vec<T> &b, Vec<T> &Tx, int row_start, int row_stop, int row_step,
                                   int blocksize) {
        done(F::block_gauss_seidel(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), x.mutable_data(), len(x), b.data(), len(b),
                                   Tx.data(), len(Tx), row_start, row_stop, row_step, blocksize), "block_gauss_seidel");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("x"), nc("b"), nc("Tx"), py::arg("row_start"), py::arg("row_stop"), py::arg("row_step"), py::arg("blocksize"));
    // amg_core.pinv_array (linalg_bind.cpp:12-30): AA ravelled, (m, n, n), TransA 'T' / 'F'
    m.def("pinv_array", [](Vec<T> &AA, int m_, int n, char TransA) {
        done(F::pinv_array(AA.mutable_data(), len(AA), m_, n, TransA), "pinv_array");
    }, nc("AA"), py::arg("m"), py::arg("n"), py::arg("TransA"));
    // amg_core.fit_candidates, real overloads (smoothed_aggregation_bind.cpp:134-170)
    m.def("fit_candidates", [](int n_row, int n_col, int K1, int K2, Idx &Ap, Idx &Ai, Vec<T> &Ax, Vec<T> &B, Vec<T> &R, T tol) {
        done(F::fit_candidates(n_row, n_col, K1, K2, Ap.data(), len(Ap), Ai.data(), len(Ai), Ax.mutable_data(), len(Ax), B.data(), len(B),
                               R.mutable_data(), len(R), tol), "fit_candidates");
    }, py::arg("n_row"), py::arg("n_col"), py::arg("K1"), py::arg("K2"), nc("Ap"), nc("Ai"), nc("Ax"), nc("B"), nc("R"), py::arg("tol"));
}

}  // namespace

PYBIND11_MODULE(_amg_core_pybind, m)
{
    m.doc() = "pybind11 bindings of the MI355X relaxation / SpMV entry points (Layer 1 of include/pyamg_amd.h), "
              "signature-compatible with pyamg.amg_core";
    bind<float>(m);
    bind<double>(m);
    // amg_core.standard_aggregation (smoothed_aggregation_bind.cpp:49-75): returns the number of aggregates
    m.def("standard_aggregation", [](int n_row, Idx &Ap, Idx &Aj, Idx &x, Idx &y) {
        int naggs = 0;
        done(pamg_standard_aggregation(n_row, Ap.data(), len(Ap), Aj.data(), len(Aj), x.mutable_data(), len(x), y.mutable_data(), len(y), &naggs),
             "standard_aggregation");
        return naggs;
    }, py::arg("n_row"), py::arg("Ap").noconvert(), py::arg("Aj").noconvert(), py::arg("x").noconvert(), py::arg("y").noconvert());
    // the classical (Ruge-Stuben) setup, float64 (ruge_stuben_bind.cpp, graph_bind.cpp): csrc/pamg_classical.hip
    using D = Vec<double>;
    auto nc = [](const char *n) { return py::arg(n).noconvert(); };
    m.def("classical_strength_of_connection_abs", [](int n_row, double theta, Idx &Ap, Idx &Aj, D &Ax, Idx &Sp, Idx &Sj, D &Sx) {
        done(pamg_classical_strength_of_connection_abs(n_row, theta, Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), Sp.mutable_data(),
                                                       len(Sp), Sj.mutable_data(), len(Sj), Sx.mutable_data(), len(Sx)),
             "classical_strength_of_connection_abs");
    }, py::arg("n_row"), py::arg("theta"), nc("Ap"), nc("Aj"), nc("Ax"), nc("Sp"), nc("Sj"), nc("Sx"));
    m.def("classical_strength_of_connection_min", [](int n_row, double theta, Idx &Ap, Idx &Aj, D &Ax, Idx &Sp, Idx &Sj, D &Sx) {
        done(pamg_classical_strength_of_connection_min(n_row, theta, Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), Sp.mutable_data(),
                                                       len(Sp), Sj.mutable_data(), len(Sj), Sx.mutable_data(), len(Sx)),
             "classical_strength_of_connection_min");
    }, py::arg("n_row"), py::arg("theta"), nc("Ap"), nc("Aj"), nc("Ax"), nc("Sp"), nc("Sj"), nc("Sx"));
    m.def("maximal_independent_set_parallel", [](int num_rows, Idx &Ap, Idx &Aj, int active, int C, int F, Idx &x, D &y, int max_iters) {
        int n_mis = 0, rounds = 0;
        done(pamg_maximal_independent_set(num_rows, Ap.data(), len(Ap), Aj.data(), len(Aj), active, C, F, x.mutable_data(), len(x), y.data(), len(y),
                                          max_iters, &n_mis, &rounds), "maximal_independent_set_parallel");
        return n_mis;
    }, py::arg("num_rows"), nc("Ap"), nc("Aj"), py::arg("active"), py::arg("C"), py::arg("F"), nc("x"), nc("y"), py::arg("max_iters") = -1);
    m.def("pmis_splitting", [](int n_nodes, Idx &Sp, Idx &Sj, D &rnd, Idx &splitting) {
        int rounds = 0;
        done(pamg_pmis_splitting(n_nodes, Sp.data(), len(Sp), Sj.data(), len(Sj), rnd.data(), len(rnd), splitting.mutable_data(), len(splitting),
                                 &rounds), "pmis_splitting");
        return rounds;
    }, py::arg("n_nodes"), nc("Sp"), nc("Sj"), nc("rnd"), nc("splitting"));
    m.def("cljp_naive_splitting", [](int n, Idx &Sp, Idx &Sj, Idx &Tp, Idx &Tj, Idx &splitting, int colorflag) {
        int info[4] = {0, 0, 0, 0};                          // Tp / Tj: the reference's argument order; the device builds the transpose itself
        done(pamg_cljp_splitting(n, Sp.data(), len(Sp), Sj.data(), len(Sj), colorflag, splitting.mutable_data(), len(splitting), info),
             "cljp_naive_splitting");
        return py::make_tuple(info[0], info[1], info[2], info[3]);
    }, py::arg("n"), nc("Sp"), nc("Sj"), nc("Tp"), nc("Tj"), nc("splitting"), py::arg("colorflag"));
    m.def("vertex_coloring_mis", [](int num_rows, Idx &Ap, Idx &Aj, Idx &x) {
        int info[2] = {0, 0};
        done(pamg_vertex_coloring_mis(num_rows, Ap.data(), len(Ap), Aj.data(), len(Aj), x.mutable_data(), len(x), info), "vertex_coloring_mis");
        return info[0];                                      // the number of colours, as the reference returns it
    }, py::arg("num_rows"), nc("Ap"), nc("Aj"), nc("x"));
    m.def("bellman_ford", [](int num_nodes, Idx &Ap, Idx &Aj, Vec<double> &Ax, Idx &c, Vec<double> &d, Idx &mm, Idx &p) {
        int info[2] = {0, 0};
        done(pamg_bellman_ford(num_nodes, Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), c.data(), len(c), d.mutable_data(), len(d),
                               mm.mutable_data(), len(mm), p.mutable_data(), len(p), info), "bellman_ford");
    }, py::arg("num_nodes"), nc("Ap"), nc("Aj"), nc("Ax"), nc("c"), nc("d"), nc("m"), nc("p"));
    m.def("most_interior_nodes", [](int num_nodes, Idx &Ap, Idx &Aj, Vec<double> &Ax, Idx &c, Vec<double> &d, Idx &mm, Idx &p) {
        int info[3] = {0, 0, 0};
        done(pamg_most_interior_nodes(num_nodes, Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), c.mutable_data(), len(c),
                                      d.mutable_data(), len(d), mm.mutable_data(), len(mm), p.mutable_data(), len(p), info), "most_interior_nodes");
        return info[2] != 0;                                 // whether a centre moved, as the reference returns it
    }, py::arg("num_nodes"), nc("Ap"), nc("Aj"), nc("Ax"), nc("c"), nc("d"), nc("m"), nc("p"));
    m.def("lloyd_cluster", [](int num_nodes, Idx &Ap, Idx &Aj, Vec<double> &Ax, Idx &c, int maxiter, Idx &clusters) {
        int info[4] = {0, 0, 0, 0};
        done(pamg_lloyd_cluster(num_nodes, Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), c.mutable_data(), len(c), maxiter,
                                clusters.mutable_data(), len(clusters), info), "lloyd_cluster");
        return py::make_tuple(info[0], info[1], info[2], info[3]);
    }, py::arg("num_nodes"), nc("Ap"), nc("Aj"), nc("Ax"), nc("c"), py::arg("maxiter"), nc("clusters"));
    m.def("rs_direct_interpolation_pass1", [](int n_nodes, Idx &Sp, Idx &Sj, Idx &splitting, Idx &Pp) {
        done(pamg_rs_direct_interpolation_pass1(n_nodes, Sp.data(), len(Sp), Sj.data(), len(Sj), splitting.data(), len(splitting), Pp.mutable_data(),
                                                len(Pp)), "rs_direct_interpolation_pass1");
    }, py::arg("n_nodes"), nc("Sp"), nc("Sj"), nc("splitting"), nc("Pp"));
    m.def("rs_classical_interpolation_pass1", [](int n_nodes, Idx &Sp, Idx &Sj, Idx &splitting, Idx &Pp) {
        done(pamg_rs_classical_interpolation_pass1(n_nodes, Sp.data(), len(Sp), Sj.data(), len(Sj), splitting.data(), len(splitting),
                                                   Pp.mutable_data(), len(Pp)), "rs_classical_interpolation_pass1");
    }, py::arg("n_nodes"), nc("Sp"), nc("Sj"), nc("splitting"), nc("Pp"));
    m.def("rs_direct_interpolation_pass2", [](int n_nodes, Idx &Ap, Idx &Aj, D &Ax, Idx &Sp, Idx &Sj, D &Sx, Idx &splitting, Idx &Pp, Idx &Pj, D &Px) {
        done(pamg_rs_direct_interpolation_pass2(n_nodes, Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), Sp.data(), len(Sp), Sj.data(),
                                                len(Sj), Sx.data(), len(Sx), splitting.data(), len(splitting), Pp.data(), len(Pp),
                                                Pj.mutable_data(), len(Pj), Px.mutable_data(), len(Px)), "rs_direct_interpolation_pass2");
    }, py::arg("n_nodes"), nc("Ap"), nc("Aj"), nc("Ax"), nc("Sp"), nc("Sj"), nc("Sx"), nc("splitting"), nc("Pp"), nc("Pj"), nc("Px"));
    m.def("rs_classical_interpolation_pass2", [](int n_nodes, Idx &Ap, Idx &Aj, D &Ax, Idx &Sp, Idx &Sj, D &Sx, Idx &splitting, Idx &Pp, Idx &Pj,
                                                  D &Px, bool modified) {
        done(pamg_rs_classical_interpolation_pass2(n_nodes, Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), Sp.data(), len(Sp), Sj.data(),
                                                   len(Sj), Sx.data(), len(Sx), splitting.data(), len(splitting), Pp.data(), len(Pp),
                                                   Pj.mutable_data(), len(Pj), Px.mutable_data(), len(Px), modified ? 1 : 0),
             "rs_classical_interpolation_pass2");
    }, py::arg("n_nodes"), nc("Ap"), nc("Aj"), nc("Ax"), nc("Sp"), nc("Sj"), nc("Sx"), nc("splitting"), nc("Pp"), nc("Pj"), nc("Px"),
       py::arg("modified"));
    m.def("remove_strong_FF_connections", [](int n_nodes, Idx &Sp, Idx &Sj, D &Sx, Idx &splitting) {
        done(pamg_remove_strong_FF_connections(n_nodes, Sp.data(), len(Sp), Sj.data(), len(Sj), Sx.mutable_data(), len(Sx), splitting.data(),
                                               len(splitting)), "remove_strong_FF_connections");
    }, py::arg("n_nodes"), nc("Sp"), nc("Sj"), nc("Sx"), nc("splitting"));
    // the approximate ideal restriction (AIR) setup, float64 (air_bind.cpp): csrc/pamg_air.hip
    m.def("one_point_interpolation", [](Idx &Pp, Idx &Pj, D &Px, Idx &Cp, Idx &Cj, D &Cx, Idx &splitting) {
        done(pamg_one_point_interpolation(Pp.mutable_data(), len(Pp), Pj.mutable_data(), len(Pj), Px.mutable_data(), len(Px), Cp.data(), len(Cp),
                                          Cj.data(), len(Cj), Cx.data(), len(Cx), splitting.data(), len(splitting)), "one_point_interpolation");
    }, nc("Pp"), nc("Pj"), nc("Px"), nc("Cp"), nc("Cj"), nc("Cx"), nc("splitting"));
    m.def("approx_ideal_restriction_pass1", [](Idx &Rp, Idx &Cp, Idx &Cj, Idx &Cpts, Idx &splitting, int distance) {
        done(pamg_approx_ideal_restriction_pass1(Rp.mutable_data(), len(Rp), Cp.data(), len(Cp), Cj.data(), len(Cj), Cpts.data(), len(Cpts),
                                                 splitting.data(), len(splitting), distance), "approx_ideal_restriction_pass1");
    }, nc("Rp"), nc("Cp"), nc("Cj"), nc("Cpts"), nc("splitting"), py::arg("distance") = 2);
    m.def("approx_ideal_restriction_pass2", [](Idx &Rp, Idx &Rj, D &Rx, Idx &Ap, Idx &Aj, D &Ax, Idx &Cp, Idx &Cj, D &Cx, Idx &Cpts, Idx &splitting,
                                                int distance, int use_gmres, int maxiter, int precondition) {
        done(pamg_approx_ideal_restriction_pass2(Rp.data(), len(Rp), Rj.mutable_data(), len(Rj), Rx.mutable_data(), len(Rx), Ap.data(), len(Ap),
                                                 Aj.data(), len(Aj), Ax.data(), len(Ax), Cp.data(), len(Cp), Cj.data(), len(Cj), Cx.data(), len(Cx),
                                                 Cpts.data(), len(Cpts), splitting.data(), len(splitting), distance, use_gmres, maxiter, precondition),
             "approx_ideal_restriction_pass2");
    }, nc("Rp"), nc("Rj"), nc("Rx"), nc("Ap"), nc("Aj"), nc("Ax"), nc("Cp"), nc("Cj"), nc("Cx"), nc("Cpts"), nc("splitting"),
       py::arg("distance") = 2, py::arg("use_gmres") = 0, py::arg("maxiter") = 10, py::arg("precondition") = 1);
    // the block (BSR) AIR setup, float64 (air_bind.cpp): csrc/pamg_air_block.hip.  norm: 0 'abs', 1 'min', 2 'fro'
    m.def("block_strength_measure", [](int blocksize, int norm, D &Ax, D &out) {
        done(pamg_block_strength_measure(len(out), blocksize, norm, Ax.data(), len(Ax), out.mutable_data(), len(out)), "block_strength_measure");
    }, py::arg("blocksize"), py::arg("norm"), nc("Ax"), nc("out"));
    m.def("block_approx_ideal_restriction_pass2", [](Idx &Rp, Idx &Rj, D &Rx, Idx &Ap, Idx &Aj, D &Ax, Idx &Cp, Idx &Cj, D &Cx, Idx &Cpts,
                                                      Idx &splitting, int blocksize, int distance, int use_gmres, int maxiter, int precondition) {
        done(pamg_block_approx_ideal_restriction_pass2(Rp.data(), len(Rp), Rj.mutable_data(), len(Rj), Rx.mutable_data(), len(Rx), Ap.data(), len(Ap),
                                                       Aj.data(), len(Aj), Ax.data(), len(Ax), Cp.data(), len(Cp), Cj.data(), len(Cj), Cx.data(),
                                                       len(Cx), Cpts.data(), len(Cpts), splitting.data(), len(splitting), blocksize, distance,
                                                       use_gmres, maxiter, precondition),
             "block_approx_ideal_restriction_pass2");
    }, nc("Rp"), nc("Rj"), nc("Rx"), nc("Ap"), nc("Aj"), nc("Ax"), nc("Cp"), nc("Cj"), nc("Cx"), nc("Cpts"), nc("splitting"), py::arg("blocksize"),
       py::arg("distance") = 2, py::arg("use_gmres") = 0, py::arg("maxiter") = 10, py::arg("precondition") = 1);
    // the evolution strength measure, float64 (evolution_strength_bind.cpp): csrc/pamg_evolution.hip
    m.def("incomplete_mat_mult_csr", [](Idx &Ap, Idx &Aj, D &Ax, Idx &Bp, Idx &Bj, D &Bx, Idx &Sp, Idx &Sj, D &Sx, int num_rows) {
        done(pamg_incomplete_mat_mult_csr_f64(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), Bp.data(), len(Bp), Bj.data(), len(Bj),
                                              Bx.data(), len(Bx), Sp.data(), len(Sp), Sj.data(), len(Sj), Sx.mutable_data(), len(Sx), num_rows),
             "incomplete_mat_mult_csr");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("Bp"), nc("Bj"), nc("Bx"), nc("Sp"), nc("Sj"), nc("Sx"), py::arg("num_rows"));
    m.def("evolution_strength_helper", [](D &Sx, Idx &Sp, Idx &Sj, int nrows, D &x, D &y, D &b, int BDBCols, int NullDim, double tol) {
        done(pamg_evolution_strength_helper_f64(Sx.mutable_data(), len(Sx), Sp.data(), len(Sp), Sj.data(), len(Sj), nrows, x.data(), len(x), y.data(),
                                                len(y), b.data(), len(b), BDBCols, NullDim, tol), "evolution_strength_helper");
    }, nc("Sx"), nc("Sp"), nc("Sj"), py::arg("nrows"), nc("x"), nc("y"), nc("b"), py::arg("BDBCols"), py::arg("NullDim"), py::arg("tol"));
    m.def("apply_distance_filter", [](int n_row, double epsilon, Idx &Sp, Idx &Sj, D &Sx) {
        done(pamg_apply_distance_filter_f64(n_row, epsilon, Sp.data(), len(Sp), Sj.data(), len(Sj), Sx.mutable_data(), len(Sx)), "apply_distance_filter");
    }, py::arg("n_row"), py::arg("epsilon"), nc("Sp"), nc("Sj"), nc("Sx"));
    m.def("apply_absolute_distance_filter", [](int n_row, double epsilon, Idx &Sp, Idx &Sj, D &Sx) {
        done(pamg_apply_absolute_distance_filter_f64(n_row, epsilon, Sp.data(), len(Sp), Sj.data(), len(Sj), Sx.mutable_data(), len(Sx)),
             "apply_absolute_distance_filter");
    }, py::arg("n_row"), py::arg("epsilon"), nc("Sp"), nc("Sj"), nc("Sx"));
    m.def("min_blocks", [](int n_blocks, int blocksize, D &Sx, D &Tx) {
        done(pamg_min_blocks_f64(n_blocks, blocksize, Sx.data(), len(Sx), Tx.mutable_data(), len(Tx)), "min_blocks");
    }, py::arg("n_blocks"), py::arg("blocksize"), nc("Sx"), nc("Tx"));
    m.def("evolution_strength_vector", [](D &Sx, Idx &Sp, Idx &Sj, int nrows, D &d, D &b) {
        done(pamg_evolution_strength_vector_f64(Sx.mutable_data(), len(Sx), Sp.data(), len(Sp), Sj.data(), len(Sj), nrows, d.data(), len(d), b.data(),
                                                len(b)), "evolution_strength_vector");
    }, nc("Sx"), nc("Sp"), nc("Sj"), py::arg("nrows"), nc("d"), nc("b"));
    // the relaxation-vector and vertex-distance strength measures, float64 (composed in Python by the reference): csrc/pamg_distance.hip
    m.def("relaxation_vectors", [](Idx &Ap, Idx &Aj, D &Ax, D &X, int n, int R, int k, double omega) {
        done(pamg_relaxation_vectors_f64(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), X.mutable_data(), len(X), n, R, k, omega),
             "relaxation_vectors");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("X"), py::arg("n"), py::arg("R"), py::arg("k"), py::arg("omega"));
    m.def("distance_measure", [](int measure, Idx &Ap, Idx &Aj, D &Ax, D &X, int n, int R, D &Dx) {
        done(pamg_distance_measure_f64(measure, Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), X.data(), len(X), n, R, Dx.mutable_data(),
                                       len(Dx)), "distance_measure");
    }, py::arg("measure"), nc("Ap"), nc("Aj"), nc("Ax"), nc("X"), py::arg("n"), py::arg("R"), nc("Dx"));
    m.def("distance_strength", [](int measure, Idx &Ap, Idx &Aj, D &Ax, D &X, int n, int R, int k, double omega, double epsilon, D &Dx) {
        done(pamg_distance_strength_f64(measure, Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), X.mutable_data(), len(X), n, R, k, omega,
                                        epsilon, Dx.mutable_data(), len(Dx)), "distance_strength");
    }, py::arg("measure"), nc("Ap"), nc("Aj"), nc("Ax"), nc("X"), py::arg("n"), py::arg("R"), py::arg("k"), py::arg("omega"), py::arg("epsilon"),
       nc("Dx"));
    m.def("vertex_distance", [](Idx &Ap, Idx &Aj, D &V, int n, int dim, D &Cx) {
        done(pamg_vertex_distance_f64(Ap.data(), len(Ap), Aj.data(), len(Aj), V.data(), len(V), n, dim, Cx.mutable_data(), len(Cx)), "vertex_distance");
    }, nc("Ap"), nc("Aj"), nc("V"), py::arg("n"), py::arg("dim"), nc("Cx"));
    // energy-minimisation prolongation smoothing, float64 (smoothed_aggregation_bind.cpp): csrc/pamg_energy.hip
    m.def("incomplete_mat_mult_bsr", [](Idx &Ap, Idx &Aj, D &Ax, Idx &Bp, Idx &Bj, D &Bx, Idx &Sp, Idx &Sj, D &Sx, int n_brow, int n_bcol, int brow_A,
                                        int bcol_A, int bcol_B) {
        done(pamg_incomplete_mat_mult_bsr_f64(Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), len(Ax), Bp.data(), len(Bp), Bj.data(), len(Bj),
                                              Bx.data(), len(Bx), Sp.data(), len(Sp), Sj.data(), len(Sj), Sx.mutable_data(), len(Sx), n_brow, n_bcol,
                                              brow_A, bcol_A, bcol_B), "incomplete_mat_mult_bsr");
    }, nc("Ap"), nc("Aj"), nc("Ax"), nc("Bp"), nc("Bj"), nc("Bx"), nc("Sp"), nc("Sj"), nc("Sx"), py::arg("n_brow"), py::arg("n_bcol"),
       py::arg("brow_A"), py::arg("bcol_A"), py::arg("bcol_B"));
    m.def("satisfy_constraints_helper", [](int rows_per_block, int cols_per_block, int num_block_rows, int NullDim, D &x, D &y, D &z, Idx &Sp,
                                           Idx &Sj, D &Sx) {
        done(pamg_satisfy_constraints_helper_f64(rows_per_block, cols_per_block, num_block_rows, NullDim, x.data(), len(x), y.data(), len(y),
                                                 z.data(), len(z), Sp.data(), len(Sp), Sj.data(), len(Sj), Sx.mutable_data(), len(Sx)),
             "satisfy_constraints_helper");
    }, py::arg("rows_per_block"), py::arg("cols_per_block"), py::arg("num_block_rows"), py::arg("NullDim"), nc("x"), nc("y"), nc("z"), nc("Sp"),
       nc("Sj"), nc("Sx"));
    m.def("satisfy_constraints", [](int rows_per_block, int cols_per_block, int num_block_rows, int NullDim, D &B, D &BtBinv, Idx &Sp, Idx &Sj,
                                    D &Sx) {
        done(pamg_satisfy_constraints_f64(rows_per_block, cols_per_block, num_block_rows, NullDim, B.data(), len(B), BtBinv.data(), len(BtBinv),
                                          Sp.data(), len(Sp), Sj.data(), len(Sj), Sx.mutable_data(), len(Sx)), "satisfy_constraints");
    }, py::arg("rows_per_block"), py::arg("cols_per_block"), py::arg("num_block_rows"), py::arg("NullDim"), nc("B"), nc("BtBinv"), nc("Sp"), nc("Sj"),
       nc("Sx"));
    // cmask / PIx: None without root nodes.  Returns (iterations, the newsum of every iteration)
    m.def("energy_cg", [](int n_brow, int n_bcol, int r, int c, int NullDim, Idx &Ap, Idx &Aj, D &Ax, Idx &Sp, Idx &Sj, D &Tx, D &B, D &BtBinv, D &Dinv,
                          std::optional<py::array_t<unsigned char, py::array::c_style>> cmask, std::optional<D> PIx, int maxiter, double tol) {
        if (cmask.has_value() != PIx.has_value() || (cmask && (cmask->size() != (py::ssize_t)n_brow * r || PIx->size() != Tx.size())))
            throw py::type_error("energy_cg(): cmask (one byte per row) and PIx (like Tx) go together");
        std::vector<double> sums((size_t)std::max(maxiter, 1));
        int its = 0, ns = 0;
        done(pamg_energy_cg_f64(n_brow, n_bcol, r, c, NullDim, Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), (int64_t)Ax.size(), Sp.data(), len(Sp),
                                Sj.data(), len(Sj), Tx.mutable_data(), (int64_t)Tx.size(), B.data(), len(B), BtBinv.data(), (int64_t)BtBinv.size(),
                                Dinv.data(), len(Dinv), cmask ? cmask->data() : nullptr, PIx ? PIx->data() : nullptr, maxiter, tol, &its, sums.data(),
                                &ns), "energy_cg");
        return py::make_tuple(its, py::array_t<double>(ns, sums.data()));
    }, py::arg("n_brow"), py::arg("n_bcol"), py::arg("r"), py::arg("c"), py::arg("NullDim"), nc("Ap"), nc("Aj"), nc("Ax"), nc("Sp"), nc("Sj"), nc("Tx"),
       nc("B"), nc("BtBinv"), nc("Dinv"), py::arg("cmask").noconvert().none(true), py::arg("PIx").noconvert().none(true), py::arg("maxiter"),
       py::arg("tol"));
    // Returns (iterations, the normr history: the initial norm first); H, if given, receives the rotated Hessenberg matrix
    m.def("energy_gmres", [](int n_brow, int n_bcol, int r, int c, int NullDim, Idx &Ap, Idx &Aj, D &Ax, Idx &Sp, Idx &Sj, D &Tx, D &B, D &BtBinv, D &Dinv,
                             std::optional<py::array_t<unsigned char, py::array::c_style>> cmask, std::optional<D> PIx, int maxiter, double tol,
                             std::optional<D> H) {
        if (cmask.has_value() != PIx.has_value() || (cmask && (cmask->size() != (py::ssize_t)n_brow * r || PIx->size() != Tx.size())))
            throw py::type_error("energy_gmres(): cmask (one byte per row) and PIx (like Tx) go together");
        const py::ssize_t ld = std::max(maxiter, 0) + 1;
        if (H && H->size() != ld * ld) throw py::type_error("energy_gmres(): H takes (maxiter + 1)^2 values");
        std::vector<double> normrs((size_t)ld);
        int its = 0, ns = 0;
        done(pamg_energy_gmres_f64(n_brow, n_bcol, r, c, NullDim, Ap.data(), len(Ap), Aj.data(), len(Aj), Ax.data(), (int64_t)Ax.size(), Sp.data(),
                                   len(Sp), Sj.data(), len(Sj), Tx.mutable_data(), (int64_t)Tx.size(), B.data(), len(B), BtBinv.data(),
                                   (int64_t)BtBinv.size(), Dinv.data(), len(Dinv), cmask ? cmask->data() : nullptr, PIx ? PIx->data() : nullptr, maxiter,
                                   tol, &its, normrs.data(), &ns, H ? H->mutable_data() : nullptr), "energy_gmres");
        return py::make_tuple(its, py::array_t<double>(ns, normrs.data()));
    }, py::arg("n_brow"), py::arg("n_bcol"), py::arg("r"), py::arg("c"), py::arg("NullDim"), nc("Ap"), nc("Aj"), nc("Ax"), nc("Sp"), nc("Sj"), nc("Tx"),
       nc("B"), nc("BtBinv"), nc("Dinv"), py::arg("cmask").noconvert().none(true), py::arg("PIx").noconvert().none(true), py::arg("maxiter"),
       py::arg("tol"), py::arg("H").noconvert().none(true) = py::none());
    // the setup of rootnode_solver, float64 (smoothed_aggregation_bind.cpp for calc_BtB; the other two have no amg_core twin): csrc/pamg_rootnode.hip
    m.def("calc_BtB", [](int NullDim, int Nnodes, int cols_per_block, D &b, int BsqCols, D &x, Idx &Sp, Idx &Sj) {
        done(pamg_calc_BtB_f64(NullDim, Nnodes, cols_per_block, b.data(), len(b), BsqCols, x.mutable_data(), len(x), Sp.data(), len(Sp), Sj.data(),
                               len(Sj)), "calc_BtB");
    }, py::arg("NullDim"), py::arg("Nnodes"), py::arg("cols_per_block"), nc("b"), py::arg("BsqCols"), nc("x"), nc("Sp"), nc("Sj"));
    m.def("compute_BtBinv", [](int NullDim, int Nnodes, int cols_per_block, D &B, Idx &Sp, Idx &Sj, D &BtBinv) {
        done(pamg_compute_BtBinv_f64(NullDim, Nnodes, cols_per_block, B.data(), (int64_t)B.size(), Sp.data(), len(Sp), Sj.data(), len(Sj),
                                     BtBinv.mutable_data(), (int64_t)BtBinv.size()), "compute_BtBinv");
    }, py::arg("NullDim"), py::arg("Nnodes"), py::arg("cols_per_block"), nc("B"), nc("Sp"), nc("Sj"), nc("BtBinv"));
    m.def("filter_constraints", [](int rows_per_block, int cols_per_block, int num_block_rows, int NullDim, D &B, D &Bf, D &BtBinv, Idx &Sp, Idx &Sj,
                                   D &Sx) {
        done(pamg_filter_constraints_f64(rows_per_block, cols_per_block, num_block_rows, NullDim, B.data(), len(B), Bf.data(), len(Bf), BtBinv.data(),
                                         len(BtBinv), Sp.data(), len(Sp), Sj.data(), len(Sj), Sx.mutable_data(), len(Sx)), "filter_constraints");
    }, py::arg("rows_per_block"), py::arg("cols_per_block"), py::arg("num_block_rows"), py::arg("NullDim"), nc("B"), nc("Bf"), nc("BtBinv"), nc("Sp"),
       nc("Sj"), nc("Sx"));
    m.def("scale_T", [](int n_brow, int n_bcol, int blocksize, Idx &Tp, Idx &Tj, D &Tx, Idx &Cnodes) {
        done(pamg_scale_T_f64(n_brow, n_bcol, blocksize, Tp.data(), len(Tp), Tj.data(), len(Tj), Tx.mutable_data(), (int64_t)Tx.size(), Cnodes.data(),
                              len(Cnodes)), "scale_T");
    }, py::arg("n_brow"), py::arg("n_bcol"), py::arg("blocksize"), nc("Tp"), nc("Tj"), nc("Tx"), nc("Cnodes"));
    m.def("version", [] { return std::string(pamg_version()); });
}
