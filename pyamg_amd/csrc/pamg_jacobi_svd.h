// pamg_jacobi_svd.h -- the reference's one-sided Jacobi SVD (svd_jacobi, pyamg/amg_core/linalg.h:546-812) of a square real block, all of
// it in the registers / scratch of one lane.  Shared by pinv_array (pamg_aggregate.hip, CAP = 6) and by the constrained least-squares
// solve of the evolution strength measure (pamg_evolution.h, CAP = 7), and by the host replays of both.
// The arithmetic follows the reference expression by expression (separate multiply and add, IEEE divide and square root, the same loop
// nests), so with -ffp-contract=off the factors come out bit for bit.
#pragma once
#include <cmath>
#include <limits>

#if defined(__HIPCC__)
#define PAMG_SVD_HD __host__ __device__
#else
#define PAMG_SVD_HD
#endif

namespace pamg {

template <typename T, int CAP>
struct JacobiSvd {
    // column-major n x n factors (leading dimension n), n <= CAP
    T U[CAP * CAP], V[CAP * CAP], S[CAP];
    int n;

    PAMG_SVD_HD T coldot(int a, int b) const
    {
        T s = T(0);
        for (int i = 0; i < n; ++i) s += U[a * n + i] * U[b * n + i];
        return s;
    }
    PAMG_SVD_HD T colnorm(int a) const { return std::sqrt(coldot(a, a)); }

    // linalg.h:546-812 for a square real block held column-major in A
    PAMG_SVD_HD void run(const T *A)
    {
        const int nn = n * n;
        if (n == 1) {                                    // :559-571
            const T na = std::fabs(A[0]);
            V[0] = T(1);
            S[0] = na;
            U[0] = (na == T(0)) ? T(1) : A[0] / na;
            return;
        }
        const T eps = std::numeric_limits<T>::epsilon();
        int count = 1, sweep = 0;
        const int sweepmax = 15 * n > 30 ? 15 * n : 30;
        const T tolerance = std::sqrt((T)n) * eps;
        for (int i = 0; i < nn; ++i) V[i] = T(0);
        for (int i = 0; i < nn; i += n + 1) V[i] = T(1);
        for (int i = 0; i < nn; ++i) U[i] = A[i];
        for (int j = 0; j < n; ++j) S[j] = eps * colnorm(j);                  // column error estimates, :598-603
        while (count > 0 && sweep <= sweepmax) {
            count = n * (n - 1) / 2;
            for (int j = 0; j < n - 1; ++j) {
                for (int k = j + 1; k < n; ++k) {
                    const T a = colnorm(j), b = colnorm(k);
                    const T d = coldot(j, k);
                    const T nd = std::fabs(d);
                    const T ea = S[j], eb = S[k];
                    const bool sorted = a >= b;
                    const bool orthog = nd <= tolerance * a * b;
                    const bool noisya = a < ea, noisyb = b < eb;
                    if (sorted && (orthog || noisya || noisyb)) {
                        --count;
                    } else if (!sorted || (nd == T(0) && a == b)) {
                        // swap the columns with one sign flip, :651-686
                        S[j] = eb;
                        S[k] = ea;
                        for (int i = 0; i < n; ++i) {
                            const T uj = U[j * n + i], uk = U[k * n + i];
                            U[j * n + i] = -uk;
                            U[k * n + i] = uj;
                        }
                        for (int i = 0; i < n; ++i) {
                            const T vj = V[j * n + i], vk = V[k * n + i];
                            V[j * n + i] = -vk;
                            V[k * n + i] = vj;
                        }
                    } else {
                        // Jacobi rotation, :689-732
                        const T tau = (b * b - a * a) / (T(2) * nd);
                        const T sg = tau < T(0) ? T(-1) : T(1);
                        // the reference's literals are doubles: with T = float these two expressions are evaluated in double
                        // and rounded once (1.0 + tau*tau, 1.0 + t*t); with T = double nothing changes
                        const T t = (T)((double)sg / ((double)std::fabs(tau) + std::sqrt(1.0 + (double)(tau * tau))));
                        const T c = (T)(1.0 / std::sqrt(1.0 + (double)(t * t)));
                        const T s = d * (t * c / nd);
                        const T ms = -s;
                        const T ns = std::fabs(s);
                        S[j] = std::fabs(c) * ea + ns * eb;
                        S[k] = ns * ea + std::fabs(c) * eb;
                        for (int i = 0; i < n; ++i) {
                            const T uj = U[j * n + i], uk = U[k * n + i];
                            U[j * n + i] = uj * c + ms * uk;
                            U[k * n + i] = s * uj + uk * c;
                        }
                        for (int i = 0; i < n; ++i) {
                            const T vj = V[j * n + i], vk = V[k * n + i];
                            V[j * n + i] = vj * c + ms * vk;
                            V[k * n + i] = s * vj + vk * c;
                        }
                    }
                }
            }
            ++sweep;
        }
        // singular values, :745-790
        T sigma_tol = T(0);
        int iszero = n;
        for (int j = 0; j < n; ++j) {
            const T cn = colnorm(j);
            if (j == 0) {
                const T alpha = T(50) / std::sqrt(std::sqrt(eps));
                sigma_tol = alpha * cn * eps;
            }
            if (cn <= sigma_tol) {
                --iszero;
                S[j] = T(0);
                for (int i = 0; i < n; ++i) U[j * n + i] = T(0);
            } else {
                S[j] = cn;
                for (int i = 0; i < n; ++i) U[j * n + i] = U[j * n + i] / cn;
            }
        }
        if (iszero == 0) {                                // the zero matrix: U = V = I, :792-805
            for (int i = 0; i < nn; ++i) V[i] = T(0);
            for (int i = 0; i < nn; i += n + 1) V[i] = T(1);
            for (int i = 0; i < nn; i += n + 1) U[i] = T(1);
        }
    }
};

}  // namespace pamg
