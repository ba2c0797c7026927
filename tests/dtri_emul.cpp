// dtri_emul.cpp -- CPU replay of the dense block-triangular form of the symmetric Gauss-Seidel sweep from zero, through the project's own plan
// header (pyamg_amd/csrc/pamg_dtri_plan.h): partition, off-block slices, reference block inverses, growth guard, and the phases in launch order.
// A stand-alone program (tests/test_dtri_plan.py builds and runs it, once more under the address and undefined-behaviour sanitizers):
//
//     dtri_emul <case file> <result file>
//
// case file  : int32 {n, nnz, B, acc}, Ap[n + 1] int32, Aj[nnz] int32, Ax[nnz] f64, b[n] f64, x[n] f64
// result file: int32 {status, blocks}, int64 {off-block entries, triangle slots of one direction}, f64 growth, x[n] f64
//              status 0: x = S b (acc = 0) or x + S b (acc = 1); otherwise the planner's reason (DTRI_E_*), x unchanged
#include "../pyamg_amd/csrc/pamg_dtri_plan.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace pamg;

template <typename T>
static bool rd(FILE *f, std::vector<T> &v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: dtri_emul <case> <result>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int hdr[4];
    if (fread(hdr, sizeof(int), 4, f) != 4 || hdr[0] < 0 || hdr[1] < 0) { fclose(f); return 2; }
    const int n = hdr[0], nnz = hdr[1], B = hdr[2], acc = hdr[3];
    std::vector<int> Ap, Aj;
    std::vector<double> Ax, b, x;
    const bool ok = rd(f, Ap, (size_t)n + 1) && rd(f, Aj, (size_t)nnz) && rd(f, Ax, (size_t)nnz) && rd(f, b, (size_t)n) && rd(f, x, (size_t)n);
    fclose(f);
    if (!ok || Ap[0] != 0 || Ap[(size_t)n] != nnz) return 2;

    DtriPlan P;
    int status = build_dtri_plan(n, Ap.data(), Aj.data(), Ax.data(), B, P);
    double growth = 0.0;
    int64_t slots = 0;
    if (status == DTRI_OK) {
        slots = P.woff[(size_t)P.nb];
        std::vector<double> Wf((size_t)slots), Wb((size_t)slots);
        for (int k = 0; k < P.nb; ++k) {
            dtri_host_inverse(P, Ap.data(), Aj.data(), Ax.data(), k, 0, Wf.data() + P.woff[(size_t)k]);
            dtri_host_inverse(P, Ap.data(), Aj.data(), Ax.data(), k, 1, Wb.data() + P.woff[(size_t)k]);
            growth = std::max(growth, std::max(dtri_host_growth(P, k, 0, Wf.data() + P.woff[(size_t)k]), dtri_host_growth(P, k, 1, Wb.data() + P.woff[(size_t)k])));
        }
        if (!(growth <= DTRI_GROWTH_CAP)) status = DTRI_E_GROWTH;
        else dtri_host_apply(P, Wf.data(), Wb.data(), b.data(), x.data(), acc != 0);
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const int head[2] = {status, status == DTRI_E_SHAPE ? 0 : P.nb};
    const int64_t counts[2] = {P.off_block_entries(), slots};
    fwrite(head, sizeof(int), 2, o);
    fwrite(counts, sizeof(int64_t), 2, o);
    fwrite(&growth, sizeof(double), 1, o);
    if (n) fwrite(x.data(), sizeof(double), (size_t)n, o);
    fclose(o);
    return 0;
}
