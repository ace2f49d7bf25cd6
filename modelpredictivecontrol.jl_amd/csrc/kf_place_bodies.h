// kf_place_bodies.h -- body of k_kf_place (kf_place_kernels.hip): the gain of a Luenberger observer from its poles, for every
// member of a batch.
//
// The reference builds K̂ = place(Â, Ĉ, poles, :o; direct) on the host (src/estimator/luenberger.jl:38-42).  Here: the robust
// placement of Kautsky, Nichols and Van Dooren ("method 0") on the dual pair F = Â', G = (Ĉm Â)', so that the poles are the
// eigenvalues of Â (I - K̂ Ĉm) = (F - G K̂')' -- the filter-form gain of mpcqp_kf_set.  All arithmetic is real.
//
//   1. G = [U0 U1][Z; 0] by Householder QR; Q = [U0 U1] is formed and kept in LDS.
//   2. nym >= nx̂: X = I.  Otherwise, for every pole j, T_j = (F - λ_j I)' U1 = (Â - λ_j I) U1 is factored; the projector on the
//      admissible subspace S_j = null(T_j') is "reflect, zero the first nx̂ - nym entries, reflect back".
//   3. x_j = P_j e_j normalised (the next e_i, cyclically, where that projection vanishes).
//   4. Sweeps: x_j <- P_j y / |P_j y| with y the unit vector orthogonal to the other columns (last column of Q of a QR of X
//      without column j), until |det X| moves by no more than 1e-3 of its value or the cap is reached.
//   5. X = Q_X R;  M' = Q_X R'^-1 Λ X';  K̂ = (Â - M') U0 Z'^-1.
//
// One member per wavefront.  Lane r owns row r of every matrix (n = nx̂ <= 32 rows; lanes from n on hold zeros); the row's
// entries are NX registers (NX = max(nx̂, nym) rounded up to 4, 8, 16 or 32: the column loops are unrolled over NX with
// wave-uniform predicates, the pivot column is picked by a select chain) -- the mapping and the Householder step of
// est_init_bodies.h.  Reductions and broadcasts are the wave interface's (mpcqp_devwave.h), so the CPU emulator runs this body
// unchanged.  Every branch is wave-uniform.  A reflector is stored normalised (H = I - v v'), one double per lane, in LDS; a
// lane reads back its own entry only.  Â, Q, Â U1, Z and the triangle of X are read across lanes (kf_place_launch.h:
// place_carve).  The reflectors of the T_j are kept for all j where that fits (PlaceArgs::stored) and rebuilt at each visit
// where it does not: the same arithmetic either way.
//
// Breakdown (status 2, K̂ not written): a diagonal entry of a triangle at or below 64 eps times the largest (or a NaN) in G
// (no full column rank), in a T_j (an unobservable mode) or in the final X (a pole repeated more often than there are
// outputs), or a gain that is not finite.  nym > nx̂: the first nx̂ measured outputs carry the gain, the others get zero columns.
#pragma once
#include <math.h>

#include "kf_place_launch.h"
#include "mpcqp_types.h"

namespace mpcqp {
namespace kf {

struct PlaceQr {
    double dmax, dmin, prod;    // largest and smallest |R_kk| and their product
    bool bad;                   // a NaN among them
    int nref;                   // reflectors written
    MPCQP_HD bool singular() const { return bad || !(dmin > 64.0 * 2.220446049250313e-16 * dmax); }
};

// Householder QR of the columns c[k], k < ncols and k != skip, in that order, of an n-row matrix.  The p-th of them pivots on
// row p; its reflector goes to refl[p * n + lane].  Afterwards c holds the triangle (rows above and on the pivots).
template <int NX, class W>
MPCQP_HD void place_qr(W& w, double (&c)[NX], int n, int ncols, int skip, double* refl, PlaceQr& qi) {
    const int r = w.lane;
    qi.dmax = 0.0; qi.dmin = 1.7976931348623157e308; qi.prod = 1.0; qi.bad = false;
    int p = 0;
    MPCQP_NOUNROLL
    for (int k = 0; k < ncols; ++k) {
        if (k == skip) continue;
        double ck = 0.0;
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j)
            if (j == k) ck = c[j];
        const double x = r >= p ? ck : 0.0;
        const double sigma = w.sum(x * x);
        const double akk = w.bcast(ck, p);
        const double nrm = sqrt(sigma);
        const double alpha = akk >= 0.0 ? -nrm : nrm;       // (the sign that avoids cancellation in v_p)
        const double v = r == p ? akk - alpha : x;
        const double den = sigma - alpha * akk;              // v'v / 2
        const double vs = den > 0.0 ? v / sqrt(den) : 0.0;   // (a zero column: nothing to reflect, R_pp = 0)
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j) {
            if (j < ncols && j > k && j != skip) {
                const double s = w.sum(vs * c[j]);
                c[j] -= s * vs;
            } else if (j == k) {
                c[j] = r == p ? alpha : (r > p ? 0.0 : c[j]);
            }
        }
        if (r < n) refl[p * n + r] = vs;
        qi.dmax = fmax(qi.dmax, nrm);
        qi.dmin = fmin(qi.dmin, nrm);
        qi.prod *= nrm;
        qi.bad = qi.bad || !(nrm == nrm);
        ++p;
    }
    qi.nref = p;
}

// y <- H_(nref-1) ... H_0 y (Q'y) and y <- H_0 ... H_(nref-1) y (Q y)
template <class W>
MPCQP_HD double place_apply_fwd(W& w, const double* refl, int n, int nref, double y) {
    const int r = w.lane;
    MPCQP_NOUNROLL
    for (int k = 0; k < nref; ++k) {
        const double v = r < n ? refl[k * n + r] : 0.0;
        y -= w.sum(v * y) * v;
    }
    return y;
}
template <class W>
MPCQP_HD double place_apply_rev(W& w, const double* refl, int n, int nref, double y) {
    const int r = w.lane;
    MPCQP_NOUNROLL
    for (int k = nref - 1; k >= 0; --k) {
        const double v = r < n ? refl[k * n + r] : 0.0;
        y -= w.sum(v * y) * v;
    }
    return y;
}

template <int NX, class W>
MPCQP_HD int place_member(W& w, const PlaceArgs& a, int b, double* sm, int& sweeps) {
    const int r = w.lane, n = a.nx, m = a.nym, ny = a.ny, mm = m < n ? m : n, q = n - mm;
    const bool act = r < n, stored = a.stored != 0;
    const int rr = act ? r : 0;
    const PlaceCarve cv = place_carve(n, m, stored);
    const double* Ab = a.Ahat + (size_t)b * n * n;
    const double* Cb = a.C + (size_t)b * ny * n;
    const double* lam = a.poles + (size_t)b * n;
    double *sA = sm + cv.A, *sQ = sm + cv.Q, *sAU = sm + cv.AU, *sZ = sm + cv.Z, *sXR = sm + cv.XR, *sR = sm + cv.R, *sWT = sm + cv.WT;
    sweeps = 0;
    PlaceQr qi;
    double c[NX], x[NX];

    // ---- Â to LDS; G = (Ĉm Â)', row r in registers
    if (act)
        for (int j = 0; j < n; ++j) sA[r + n * j] = Ab[r + n * j];
    w.sync();
    MPCQP_UNROLL
    for (int k = 0; k < NX; ++k) {
        c[k] = 0.0;
        if (k < mm && act) {
            const int row = a.i_ym[k];
            double acc = 0.0;
            for (int j = 0; j < n; ++j) acc += Cb[row + ny * j] * sA[j + n * r];
            c[k] = acc;
        }
    }
    place_qr<NX>(w, c, n, mm, -1, sXR, qi);
    if (qi.singular()) return PLACE_BROKE_DOWN;
    if (r < mm) {
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j)
            if (j < mm && j >= r) sZ[r + mm * j] = c[j];
    }
    MPCQP_NOUNROLL
    for (int j = 0; j < n; ++j) {                            // Q = H_0 ... H_(mm-1), column by column
        const double y = place_apply_rev(w, sXR, n, mm, r == j ? 1.0 : 0.0);
        if (act) sQ[r + n * j] = y;
    }
    w.sync();
    if (q > 0) {                                             // Â U1
        if (act)
            for (int i = 0; i < q; ++i) {
                double acc = 0.0;
                for (int j = 0; j < n; ++j) acc += sA[r + n * j] * sQ[j + n * (mm + i)];
                sAU[r + n * i] = acc;
            }
        w.sync();
    }

    MPCQP_UNROLL
    for (int j = 0; j < NX; ++j) x[j] = (act && j == r) ? 1.0 : 0.0;

    // ---- pass 0: the admissible subspaces and the start; pass s >= 1: sweep s.  Column index n: the QR of all of X, whose
    // triangle (c), reflectors (sXR) and diagonal (qi) the gain is computed from after the last pass
    double detp = 0.0;
    const int cap = q > 0 ? a.cap : 0;
    MPCQP_NOUNROLL
    for (int pass = 0;; ++pass) {
        MPCQP_NOUNROLL
        for (int j = 0; j <= n; ++j) {
            const bool col = j < n && q > 0;
            if (j < n && !col) continue;
            double* wt = sWT + (stored && col ? j * n * q : 0);
            if (col && (pass == 0 || !stored)) {
                const double lj = lam[j];
                MPCQP_UNROLL
                for (int i = 0; i < NX; ++i) c[i] = (i < q && act) ? sAU[rr + n * i] - lj * sQ[rr + n * (mm + i)] : 0.0;
                place_qr<NX>(w, c, n, q, -1, wt, qi);
                if (pass == 0 && qi.singular()) return PLACE_BROKE_DOWN;
            }
            if (!col || pass > 0) {
                MPCQP_UNROLL
                for (int i = 0; i < NX; ++i) c[i] = x[i];
                place_qr<NX>(w, c, n, n, col ? j : -1, sXR, qi);
            }
            if (col) {
                // pass 0: e_j, e_(j+1), ... until one has a projection; a sweep: the unit vector orthogonal to the other columns
                const double yx = pass > 0 ? place_apply_rev(w, sXR, n, n - 1, r == n - 1 ? 1.0 : 0.0) : 0.0;
                const int tries = pass == 0 ? n : 1;
                double v = 0.0, nv = 0.0;
                MPCQP_NOUNROLL
                for (int t = 0; t < tries; ++t) {
                    const int i = j + t < n ? j + t : j + t - n;
                    v = pass == 0 ? (r == i ? 1.0 : 0.0) : yx;
                    v = place_apply_fwd(w, wt, n, q, v);
                    if (r < q) v = 0.0;
                    v = place_apply_rev(w, wt, n, q, v);
                    nv = sqrt(w.sum(v * v));
                    if (nv >= PLACE_VEC_TOL) break;
                }
                const bool ok = nv >= PLACE_VEC_TOL;
                if (ok || pass == 0) {
                    const double xj = ok ? v / nv : 0.0;
                    MPCQP_UNROLL
                    for (int i = 0; i < NX; ++i)
                        if (i == j) x[i] = xj;
                }
            }
        }
        const double det = qi.prod;
        if (pass > 0) {
            sweeps = pass;
            if (fabs(det - detp) <= PLACE_DET_RTOL * det) break;
        }
        detp = det;
        if (pass >= cap) break;
    }
    if (qi.singular()) return PLACE_BROKE_DOWN;

    // ---- the gain.  R (in c) to LDS; lane l solves R' s = (Λ X')(:, l) = (λ_i X[l][i])_i in its registers
    if (act) {
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j)
            if (j < n && j >= r) sR[r + n * j] = c[j];
    }
    w.sync();
    double s[NX];
    MPCQP_UNROLL
    for (int i = 0; i < NX; ++i) {
        s[i] = 0.0;
        if (i < n) {
            double acc = lam[i] * x[i];
            MPCQP_UNROLL
            for (int k = 0; k < NX; ++k)
                if (k < i) acc -= sR[k + n * i] * s[k];
            s[i] = acc / sR[i + n * i];
        }
    }
    w.sync();
    if (act) {                                               // S to LDS, lane l its column; back as rows
        MPCQP_UNROLL
        for (int i = 0; i < NX; ++i)
            if (i < n) sR[i + n * r] = s[i];
    }
    w.sync();
    MPCQP_UNROLL
    for (int j = 0; j < NX; ++j) c[j] = (j < n && act) ? sR[rr + n * j] : 0.0;
    MPCQP_NOUNROLL
    for (int k = n - 1; k >= 0; --k) {                       // M' = Q_X S
        const double v = act ? sXR[k * n + rr] : 0.0;
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j)
            if (j < n) c[j] -= w.sum(v * c[j]) * v;
    }
    MPCQP_UNROLL
    for (int j = 0; j < NX; ++j) c[j] = (j < n && act) ? sA[rr + n * j] - c[j] : 0.0;      // (F - M)' = Â - M'
    double wr[NX], kh[NX];
    MPCQP_UNROLL
    for (int i = 0; i < NX; ++i) {                           // ((F - M)' U0)(r, i)
        double acc = 0.0;
        if (i < mm) {
            MPCQP_UNROLL
            for (int j = 0; j < NX; ++j)
                if (j < n) acc += c[j] * sQ[j + n * i];
        }
        wr[i] = acc;
    }
    bool fin = true;
    MPCQP_UNROLL
    for (int i = NX - 1; i >= 0; --i) {                      // K̂ Z' = (F - M)' U0, row r
        kh[i] = 0.0;
        if (i < mm) {
            double acc = wr[i];
            MPCQP_UNROLL
            for (int k = 0; k < NX; ++k)
                if (k > i && k < mm) acc -= kh[k] * sZ[i + mm * k];
            kh[i] = acc / sZ[i + mm * i];
            fin = fin && fabs(kh[i]) <= 1.7976931348623157e308;
        }
    }
    if (w.any(act && !fin)) return PLACE_BROKE_DOWN;
    if (act) {
        double* Kb = a.K + (size_t)b * n * m;
        MPCQP_UNROLL
        for (int i = 0; i < NX; ++i)
            if (i < m) Kb[r + n * i] = kh[i];
    }
    return PLACE_OK;
}

template <int NX, class W>
MPCQP_HD void kf_place_body(W& w, const PlaceArgs& a, int b, double* sm) {
    int sweeps = 0;
    const int st = place_member<NX>(w, a, b, sm, sweeps);
    if (w.lane == 0) {
        a.status[b] = st;
        a.sweeps[b] = sweeps;
    }
}

}  // namespace kf
}  // namespace mpcqp
