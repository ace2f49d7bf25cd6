// est_init_bodies.h -- body of k_est_init (est_kernels.hip): the estimator half of initstate! for every member of a batch.
//
// init_estimate! (src/estimator/execute.jl:246-259) solves  [I - Â; Ĉm] x̂0 = [B̂u u0 + B̂d d0 + f̂op - x̂op; y0m - D̂dm d0]  with
// `\` on a rectangular matrix, i.e. by QR.  Here: Householder QR without pivoting, one member per wavefront.  Lane r owns row r
// of the m x n matrix (m = nx̂ + nym <= 64, n = nx̂ <= 32) and of the right-hand side; the row's entries are NX registers
// (NX = n rounded up to 4, 8, 16 or 32: the column loops are unrolled over NX with wave-uniform predicates, so a register is
// never indexed by a run-time value; the loop over the pivot column is not unrolled, its column is picked by a select chain).
// A reflection of column k costs one wave reduction for the norm and one per column to its right and for the right-hand
// side; the reductions and broadcasts are the wave interface's (mpcqp_devwave.h: DPP inside a 16-lane row, v_readlane across
// rows), so the CPU emulator runs this body unchanged.  Back-substitution: lane k divides, the value is broadcast, the lanes
// above subtract their entry of column k.
//
// No full column rank (a diagonal entry of R below 64 eps max|R_jj|, or a NaN): status 1 and x̂0 is NOT written.  The reference
// returns LAPACK's minimum-norm solution there (pivoted QR); this kernel does not pivot and refuses instead.
#pragma once
#include <math.h>

#include "est_init_launch.h"
#include "mpcqp_types.h"

namespace mpcqp {
namespace est {

template <int NX, class W>
MPCQP_HD void est_init_body(W& w, const InitArgs& a, int b) {
    const int r = w.lane, nx = a.nx, nym = a.nym, ny = a.ny, nu = a.nu, nd = a.nd, m = nx + nym;
    const double* A = a.Ahat + (size_t)b * nx * nx;
    const double* Cm = a.C + (size_t)b * ny * nx;
    double col[NX];
    double rhs = 0.0;
    MPCQP_UNROLL
    for (int j = 0; j < NX; ++j) col[j] = 0.0;
    if (r < nx) {                   // rows of I - Â
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j)
            if (j < nx) col[j] = (j == r ? 1.0 : 0.0) - A[r + nx * j];
        rhs = a.fx ? a.fx[(size_t)b * nx + r] : 0.0;
        for (int c = 0; c < nu; ++c) rhs += a.Bu[(size_t)b * nx * nu + r + nx * c] * a.u0[(size_t)b * nu + c];
        for (int e = 0; e < nd; ++e) rhs += a.Bd[(size_t)b * nx * nd + r + nx * e] * a.d0[(size_t)b * nd + e];
    } else if (r < m) {             // rows of Ĉm
        const int q = a.i_ym[r - nx];
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j)
            if (j < nx) col[j] = Cm[q + ny * j];
        rhs = a.y0m[(size_t)b * nym + (r - nx)];
        for (int e = 0; e < nd; ++e) rhs -= a.Dd[(size_t)b * ny * nd + q + ny * e] * a.d0[(size_t)b * nd + e];
    }

    // Householder reflections H_k = I - beta v v', v = x - alpha e_k with x the column from its diagonal down
    MPCQP_NOUNROLL
    for (int k = 0; k < nx; ++k) {
        double ck = 0.0;
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j)
            if (j == k) ck = col[j];
        const double x = r >= k ? ck : 0.0;
        const double sigma = w.sum(x * x);
        const double akk = w.bcast(ck, k);
        const double nrm = sqrt(sigma);
        const double alpha = akk >= 0.0 ? -nrm : nrm;       // (the sign that avoids cancellation in v_k)
        const double v = r == k ? akk - alpha : x;
        const double den = sigma - alpha * akk;              // v'v / 2 = sigma + |akk| nrm
        const double beta = den > 0.0 ? 1.0 / den : 0.0;     // (a zero column: nothing to reflect, R_kk = 0)
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j) {
            if (j < nx && j > k) {
                const double s = w.sum(v * col[j]);
                col[j] -= beta * s * v;
            } else if (j == k) {
                col[j] = r == k ? alpha : (r > k ? 0.0 : col[j]);
            }
        }
        const double s = w.sum(v * rhs);
        rhs -= beta * s * v;
    }

    // rank test on the diagonal of R (lane j holds R_jj)
    double dg = 0.0;
    MPCQP_UNROLL
    for (int j = 0; j < NX; ++j)
        if (j == r) dg = col[j];
    const double ad = fabs(dg);
    const double dmax = w.maxv(r < nx ? ad : 0.0);
    const double tol = 64.0 * 2.220446049250313e-16 * dmax;
    const bool sing = w.any(r < nx && !(ad >= tol && ad > 0.0));

    if (!sing) {                    // (wave-uniform)
        double acc = rhs, xs = 0.0;
        MPCQP_NOUNROLL
        for (int k = nx - 1; k >= 0; --k) {
            double ck = 0.0;
            MPCQP_UNROLL
            for (int j = 0; j < NX; ++j)
                if (j == k) ck = col[j];
            const double xk = w.bcast(acc / ck, k);          // (lane k's quotient; the other lanes' is not used)
            if (r == k) xs = xk;
            if (r < k) acc -= ck * xk;
        }
        if (r < nx) a.xhat0[(size_t)b * nx + r] = xs;
    }
    if (r == 0) a.status[b] = sing ? 1 : 0;
}

}  // namespace est
}  // namespace mpcqp
