// pamg_cljp.h -- the per-node and per-edge rules of the CLJP / CLJP-c coarse-grid selection and of the MIS vertex colouring, shared by
// the kernels of pamg_cljp.hip and the host replay tests/cljp_emul.cpp (lanes, groups, rounds and passes as loops), as
// pamg_classical.h is shared by the classical setup.
//
//   colour_node     one synchronous round of amg_core::vertex_coloring_mis (graph.h:218-235) for one node and one colour: repeated
//                   maximal_independent_set_serial (graph.h:70-97)
//   random_weights  the reference's srand(2448422) / rand() draw (ruge_stuben.h:617-621), host only
//   initial_weight  the in-degree added ONE AT A TIME, as the reference's weight[j]++ (ruge_stuben.h:624-631)
//   selects, p5_edge, apply_node, stages, p6_edge
//                   one pass of amg_core::cljp_naive_splitting (ruge_stuben.h:634-727)
//
// Why synchronous passes give the reference's array although it sweeps in place.  Selection is synchronous in the reference too: Dlist is
// collected against the unchanged splitting.  P5 and P6 only mark edges dead and decrement the weights of undecided (U) nodes; a node that
// drops below 1 turns F in the middle of the loop, and from then on nothing reads its weight or the marks of the edges into it (every read
// is guarded by splitting[..] == U_NODE).  So for the nodes that are still U when a pass ends, the set of dead edges and the number of
// decrements do not depend on the order of the C-points.  P6 in closed form: a live edge (j -> k), k still U after P5, dies in this pass
// exactly when Srow(j) and Srow(k) share a node selected in this pass.  The arithmetic is exact: w - 1 is exact for a double w >= 1, so
// w - count in one subtraction is `count` decrements, and "fell below 1 at some point" is "is below 1 at the end".
//
// The diagonal is skipped everywhere (the reference removes it first); rows need not be sorted; no row may hold a column twice.
#pragma once
#include <cstdlib>

#if defined(__HIPCC__)
#define PAMG_CLJP_HD __host__ __device__ __forceinline__
#else
#define PAMG_CLJP_HD inline
#endif

namespace pamg {
namespace cljp {

constexpr int F_NODE = 0, C_NODE = 1, U_NODE = 2;           // ruge_stuben.h:15-17
constexpr int UNDECIDED = -1, OUT = -2;                     // colouring: not coloured yet / not coloured yet and out for the current colour
constexpr unsigned SEED = 2448422u;                         // ruge_stuben.h:618
constexpr int NCLASS = 5;                                   // lane-group widths 8 / 16 / 32 / 64 by the row's length, and the rows beyond 64
PAMG_CLJP_HD int size_class(int n) { return n <= 8 ? 0 : n <= 16 ? 1 : n <= 32 ? 2 : n <= 64 ? 3 : 4; }

// The state of the uncoloured, undecided node i after one round of colour K.  Tp / Tj: the transposed pattern, i.e. the j with i in row(j).
// The serial sweep gives i the colour K exactly when no j < i with i in row(j) takes K: such a j that took K puts i out, one that is
// still undecided makes i wait, and everything else (coloured earlier, out, j >= i) has no say.
PAMG_CLJP_HD int colour_node(int i, const int *Tp, const int *Tj, const int *prev, int K)
{
    bool wait = false;
    for (int p = Tp[i]; p < Tp[i + 1]; ++p) {
        const int j = Tj[p];
        if (j >= i) continue;
        const int xj = prev[j];
        if (xj == K) return OUT;
        if (xj == UNDECIDED) wait = true;
    }
    return wait ? UNDECIDED : K;
}

// the reference's draw, with its side effect: the C library's stream is left reseeded and advanced by n
inline void random_weights(int n, double *w)
{
    srand(SEED);
    for (int i = 0; i < n; ++i) w[i] = double(rand()) / RAND_MAX;
}

PAMG_CLJP_HD double colour_weight(int colour, int ncolors) { return double(colour) / double(ncolors); }

// a single base + double(indegree) rounds differently
PAMG_CLJP_HD double initial_weight(double base, int indegree)
{
    for (int d = 0; d < indegree; ++d) base += 1.0;
    return base;
}

// SELECT: the U node i joins the set when no U neighbour in its row of S or of S^T has a strictly larger weight (ties select both)
PAMG_CLJP_HD bool selects(int i, const int *Sp, const int *Sj, const int *Tp, const int *Tj, const double *w, const int *prev)
{
    const double wi = w[i];
    for (int pass = 0; pass < 2; ++pass) {
        const int *P = pass ? Tp : Sp, *J = pass ? Tj : Sj;
        for (int p = P[i]; p < P[i + 1]; ++p) {
            const int j = J[p];
            if (j != i && prev[j] == U_NODE && w[j] > wi) return false;
        }
    }
    return true;
}

// P5, entry jj of the row of a node c selected in this pass: the live edge to a U node dies and costs that node one decrement
PAMG_CLJP_HD bool p5_edge(int c, int jj, const int *Sj, const int *state, const unsigned char *edgemark)
{
    const int j = Sj[jj];
    return j != c && state[j] == U_NODE && edgemark[jj] != 0;
}

// APPLY: `count` decrements at once; a U node that was decremented and is below 1 turns F.  (A node that was never decremented stays U
// whatever its weight, as in the reference.)
PAMG_CLJP_HD int apply_node(int state, int count, double *w)
{
    if (state != U_NODE || count == 0) return state;
    *w -= double(count);
    return *w < 1 ? F_NODE : U_NODE;
}

// P6, row j: entry c of the row is staged when it was selected in this pass
PAMG_CLJP_HD bool stages(int j, int c, const int *selpass, int pass) { return c != j && selpass[c] == pass; }

// P6, entry kk of row j, with the row's nst staged entries: the live edge (j -> k), k still U, dies when Srow(k) holds a staged node
PAMG_CLJP_HD bool p6_edge(int j, int kk, const int *Sp, const int *Sj, const int *state, const unsigned char *edgemark, const int *selpass,
                          int pass, const int *stage, int nst)
{
    const int k = Sj[kk];
    if (k == j || state[k] != U_NODE || edgemark[kk] == 0) return false;
    for (int q = Sp[k]; q < Sp[k + 1]; ++q) {
        const int c = Sj[q];
        if (c == k || selpass[c] != pass) continue;
        for (int s = 0; s < nst; ++s)
            if (stage[s] == c) return true;
    }
    return false;
}

}  // namespace cljp
}  // namespace pamg
