// c2d_bodies.h -- body of k_c2d (c2d_kernels.hip): LinModel(sys, Ts) and augment_model for every member of a batch of
// continuous-time models.
//
// The reference discretises on the host (src/model/linmodel.jl:165-198): c2d(sysu, Ts, :zoh) for the manipulated inputs,
// c2d(sysd, Ts, :tustin) for the measured disturbances, the two stacked as [sysu_dis sysd_dis]; augment_model
// (src/estimator/construct.jl:305-323) then appends the integrators of nint_u / nint_ym.  Here, per member:
//
//   ZOH block     exp([[A, Bu(, Bd)], [0, 0]] Ts) = [[Φ, Γu(, Γd)], [0, I]]   (Bd only with d_method = ZOH)
//   Tustin block  a = Ts/2, W = (I - aA)^-1:  At = W (I + aA),  Bt = W Bd Ts,  Ct = C W,  Dt = Dd + a C W Bd
//   plant         x = [xu; xd]:  A = blkdiag(Φ, At), Bu = [Γu; 0], Bd = [0; Bt], C = [C, Ct], Dd = Dt   (nx_dis = 2 nx); without
//                 the Tustin block A = Φ, Bu = Γu, Bd = Γd, C = C, Dd = Dd (nx_dis = nx)
//   augmentation  Â = [A, Bu Cs_u; 0, As], B̂u = [Bu; 0], Ĉ = [C, Cs_y], B̂d = [Bd; 0], D̂d = Dd, f̂op - x̂op padded with zeros
//
// The reference's sminreal / minreal afterwards are NOT done: they change the realisation, not the input-output map.  Nor is
// an integrator pruned (default_nint) or observability verified: nint_u / nint_ym are what the caller gives.
//
// The exponential: scaling and squaring around the [13/13] Padé approximant (Higham 2005), coefficients divided by b0 so that
// A = 0 gives Φ = I, Γ = Ts B exactly.  The number of squarings comes from min(|M|, max(|M^4|^(1/4), |M^6|^(1/6))) in the
// infinity norm (Al-Mohy and Higham 2009: the powers that the approximant needs anyway bound the truncation error of a
// non-normal matrix far below what its norm does): s = the least integer with that value / 2^s <= 5.37.  Six products for the
// approximant, one solve, s squarings.
//
// One member per wavefront.  Lane r owns row r of every working matrix (block order N = nx + nu (+ nd) <= 32); the row it
// accumulates lives in NX registers (NX = 4, 8, 16 or 32, every loop over them unrolled: no register is indexed by a
// run-time value).  Operands live in LDS, column-major with leading dimension NX (c2d_launch.h): a product reads its left
// operand's entry (r, k) at a lane's own address (consecutive lanes, consecutive words) and row k of its right operand at
// wave-uniform addresses, and is NX in-lane multiply-adds per k -- there is no wave reduction in a product.  Reductions: the
// three norms, two per column of a solve (pivot search), the finiteness votes.
//
// The solves ((V - U) X = V + U of the approximant; (I - aA) W = I) are Gauss-Jordan eliminations with partial pivoting and
// no row exchange: the lane with the largest entry of column k among those that have not pivoted yet hands its row round
// through LDS, every other lane eliminates, and at the end the lane that pivoted on column k holds row k of the solution.
//
// Status 2, nothing written for the member: an input that is not finite, Ts not finite or <= 0, a pivot at or below 64 eps
// times the largest (est_init_bodies.h's rule), more than 64 squarings, a result that is not finite.
#pragma once
#include <math.h>

#include "c2d_launch.h"
#include "mpcqp_types.h"

namespace mpcqp {
namespace c2d {

MPCQP_HD inline bool c2d_fin(double x) { return fabs(x) <= 1.7976931348623157e308; }

// acc = L R: row r of L (entries (r, k), k < kn) times the rows k of R, columns j < jn rounded up to a multiple of four (both
// operands are zero beyond their live part)
template <int NX>
MPCQP_HD void c2d_mul(const double* sL, const double* sR, int rr, int kn, int jn, double (&acc)[NX]) {
    MPCQP_UNROLL
    for (int j = 0; j < NX; ++j) acc[j] = 0.0;
    MPCQP_UNROLL4                                          // (four k at a time: the LDS reads of the next rows under the multiply-adds)
    for (int k = 0; k < kn; ++k) {
        const double l = sL[rr + NX * k];
        const double* Rk = sR + k;
        MPCQP_UNROLL
        for (int g = 0; g < NX; g += 4) {
            if (g < jn) {
                acc[g] += l * Rk[NX * g];
                acc[g + 1] += l * Rk[NX * (g + 1)];
                acc[g + 2] += l * Rk[NX * (g + 2)];
                acc[g + 3] += l * Rk[NX * (g + 3)];
            }
        }
    }
}

template <int NX>
MPCQP_HD void c2d_store(double* sM, int r, bool act, const double (&x)[NX]) {
    if (act) {
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j) sM[r + NX * j] = x[j];
    }
}

// P X = Q for the n lanes with `live` (rows of P and Q in p and q; n <= NX).  sPiv: 2 NX doubles.  Row k of X goes to
// sOut[k + NX j], j < NX; the rows from n on are zeroed.  False: singular to working precision, or a NaN among the pivots.
template <int NX, class W>
MPCQP_HD bool c2d_solve(W& w, double (&p)[NX], double (&q)[NX], int n, bool live, bool act, double* sPiv, double* sOut) {
    const int r = w.lane;
    int myk = -1;
    double pmax = 0.0, pmin = 1.7976931348623157e308;
    MPCQP_NOUNROLL
    for (int k = 0; k < n; ++k) {
        double ck = 0.0;
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j)
            if (j == k) ck = p[j];
        const bool cand = live && myk < 0;
        const double ak = fabs(ck);
        const double m = w.maxv(cand ? ak : -1.0);
        const int pl = (int)w.minv(cand && ak == m ? (double)r : 64.0);
        if (pl >= 64) return false;                         // (a column of NaNs)
        pmax = fmax(pmax, m);
        pmin = fmin(pmin, m);
        if (r == pl) {
            myk = k;
            MPCQP_UNROLL
            for (int j = 0; j < NX; ++j) {
                sPiv[j] = p[j];
                sPiv[NX + j] = q[j];
            }
        }
        w.sync();
        const double f = (live && r != pl) ? ck / sPiv[k] : 0.0;
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j) {
            if (j < n) {
                if (j == k) p[j] = r == pl ? p[j] : 0.0;
                else if (j > k) p[j] -= f * sPiv[j];
            }
            q[j] -= f * sPiv[NX + j];
        }
        w.sync();
    }
    if (!(pmin > 64.0 * 2.220446049250313e-16 * pmax)) return false;
    double dg = 1.0;
    MPCQP_UNROLL
    for (int j = 0; j < NX; ++j)
        if (j == myk) dg = p[j];
    if (live) {
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j) sOut[myk + NX * j] = q[j] / dg;
    } else if (act) {
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j) sOut[r + NX * j] = 0.0;
    }
    w.sync();
    return true;
}

template <int NX, class W>
MPCQP_HD int c2d_member(W& w, const C2dArgs& a, int b, double* sm) {
    // [13/13] Padé coefficients over b0 = 64764752532480000 (c0 = 1, c1 = 1/2)
    constexpr double B0 = 64764752532480000.0;
    constexpr double c1 = 0.5, c2 = 7771770303897600.0 / B0, c3 = 1187353796428800.0 / B0, c4 = 129060195264000.0 / B0,
                     c5 = 10559470521600.0 / B0, c6 = 670442572800.0 / B0, c7 = 33522128640.0 / B0, c8 = 1323241920.0 / B0,
                     c9 = 40840800.0 / B0, c10 = 960960.0 / B0, c11 = 16380.0 / B0, c12 = 182.0 / B0, c13 = 1.0 / B0;
    const int r = w.lane, nx = a.nx, nu = a.nu, ny = a.ny, nd = a.nd, nxd = a.nxd, nxh = a.nxh;
    const bool tust = c2d_tustin(a);
    const int N = c2d_order(a);
    const bool act = r < NX, live = r < N;
    const int rr = act ? r : 0;
    double *M0 = sm, *M1 = M0 + NX * NX, *M2 = M1 + NX * NX, *M3 = M2 + NX * NX, *M4 = M3 + NX * NX, *M5 = M4 + NX * NX,
           *M6 = M5 + NX * NX;
    const double* Ab = a.A + (size_t)b * nx * nx;
    const double* Bub = a.Bu + (size_t)b * nx * nu;
    const double* Cb = a.C + (size_t)b * ny * nx;
    const double* Bdb = nd > 0 ? a.Bd + (size_t)b * nx * nd : nullptr;
    const double* Ddb = nd > 0 ? a.Dd + (size_t)b * ny * nd : nullptr;
    const double* dopb = a.dop ? a.dop + (size_t)b * nxd : nullptr;
    const double Ts = a.Ts[b];
    bool bad = !(Ts > 0.0 && c2d_fin(Ts));
    double acc[NX], u[NX], v[NX];

    // ---- M Ts to LDS, its norm, the finiteness of every input
    double rs = 0.0;
    MPCQP_UNROLL
    for (int j = 0; j < NX; ++j) {
        double x = 0.0;
        if (r < nx && j < N) {
            x = j < nx ? Ab[r + nx * j] : j < nx + nu ? Bub[r + nx * (j - nx)] : Bdb[r + nx * (j - nx - nu)];
            bad = bad || !c2d_fin(x);
            x *= Ts;
        }
        if (act) M0[r + NX * j] = x;
        rs += fabs(x);
    }
    for (int i = r; i < ny; i += WAVE) {
        MPCQP_UNROLL4
        for (int j = 0; j < nx; ++j) bad = bad || !c2d_fin(Cb[i + ny * j]);
        MPCQP_UNROLL4
        for (int e = 0; e < nd; ++e) bad = bad || !c2d_fin(Ddb[i + ny * e]);
    }
    if (tust && r < nx)
        for (int e = 0; e < nd; ++e) bad = bad || !c2d_fin(Bdb[r + nx * e]);
    if (dopb)
        for (int i = r; i < nxd; i += WAVE) bad = bad || !c2d_fin(dopb[i]);
    if (w.any(bad)) return C2D_REFUSED;
    const double n1 = w.maxv(rs);
    if (!c2d_fin(n1)) return C2D_REFUSED;
    w.sync();

    // ---- the powers, the scaling
    c2d_mul<NX>(M0, M0, rr, N, N, acc);
    c2d_store<NX>(M1, r, act, acc);
    w.sync();
    c2d_mul<NX>(M1, M1, rr, N, N, acc);
    c2d_store<NX>(M2, r, act, acc);
    rs = 0.0;
    MPCQP_UNROLL
    for (int j = 0; j < NX; ++j) rs += fabs(acc[j]);
    const double n4 = w.maxv(live ? rs : 0.0);
    w.sync();
    c2d_mul<NX>(M2, M1, rr, N, N, acc);
    c2d_store<NX>(M3, r, act, acc);
    rs = 0.0;
    MPCQP_UNROLL
    for (int j = 0; j < NX; ++j) rs += fabs(acc[j]);
    const double n6 = w.maxv(live ? rs : 0.0);
    const double eta = fmin(n1, fmax(sqrt(sqrt(n4)), cbrt(sqrt(n6))));
    if (!c2d_fin(eta)) return C2D_REFUSED;
    int s = 0;
    for (double t = eta / C2D_THETA13; t > 1.0 && s <= C2D_SQ_MAX; t *= 0.5) ++s;
    if (s > C2D_SQ_MAX) return C2D_REFUSED;
    const double sc = ldexp(1.0, -s), sc2 = sc * sc, sc4 = sc2 * sc2, sc6 = sc4 * sc2;
    if (act) {                                              // (a lane's own entries: exact, powers of two)
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j) {
            const int o = r + NX * j;
            const double a2 = M1[o] * sc2, a4 = M2[o] * sc4, a6 = M3[o] * sc6;
            M0[o] *= sc;
            M1[o] = a2;
            M2[o] = a4;
            M3[o] = a6;
            M4[o] = c13 * a6 + c11 * a4 + c9 * a2;
        }
    }
    w.sync();

    // ---- U = M (M^6 (c13 M^6 + c11 M^4 + c9 M^2) + c7 M^6 + c5 M^4 + c3 M^2 + c1 I)
    c2d_mul<NX>(M3, M4, rr, N, N, acc);
    MPCQP_UNROLL
    for (int j = 0; j < NX; ++j) {
        const int o = rr + NX * j;
        acc[j] += c7 * M3[o] + c5 * M2[o] + c3 * M1[o] + (j == r ? c1 : 0.0);
    }
    w.sync();
    c2d_store<NX>(M4, r, act, acc);
    w.sync();
    c2d_mul<NX>(M0, M4, rr, N, N, u);
    w.sync();
    // ---- V = M^6 (c12 M^6 + c10 M^4 + c8 M^2) + c6 M^6 + c4 M^4 + c2 M^2 + I
    if (act) {
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j) {
            const int o = r + NX * j;
            M4[o] = c12 * M3[o] + c10 * M2[o] + c8 * M1[o];
        }
    }
    w.sync();
    c2d_mul<NX>(M3, M4, rr, N, N, v);
    MPCQP_UNROLL
    for (int j = 0; j < NX; ++j) {
        const int o = rr + NX * j;
        const double vv = v[j] + (c6 * M3[o] + c4 * M2[o] + c2 * M1[o] + (j == r ? 1.0 : 0.0)), uu = u[j];
        u[j] = vv - uu;
        v[j] = vv + uu;
    }
    w.sync();
    if (!c2d_solve<NX>(w, u, v, N, live, act, M4, M5)) return C2D_REFUSED;
    MPCQP_NOUNROLL
    for (int i = 0; i < s; ++i) {
        c2d_mul<NX>(M5, M5, rr, N, N, acc);
        w.sync();
        c2d_store<NX>(M5, r, act, acc);
        w.sync();
    }
    if (live) {
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j) bad = bad || !c2d_fin(M5[r + NX * j]);
    }

    // ---- the Tustin block of the measured disturbances
    if (tust) {
        const double ah = 0.5 * Ts;
        const bool lx = r < nx, ly = r < ny;
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j) {
            const double e = j == r ? 1.0 : 0.0, x = (lx && j < nx) ? ah * Ab[r + nx * j] : 0.0;
            u[j] = e - x;
            v[j] = e;
            if (act) M2[r + NX * j] = lx ? e + x : 0.0;
        }
        if (!c2d_solve<NX>(w, u, v, nx, lx, act, M4, M1)) return C2D_REFUSED;
        c2d_mul<NX>(M1, M2, rr, nx, nx, acc);              // At
        c2d_store<NX>(M3, r, act, acc);
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j) bad = bad || (lx && !c2d_fin(acc[j]));
        w.sync();
        if (act) {
            MPCQP_UNROLL
            for (int j = 0; j < NX; ++j) {
                M2[r + NX * j] = (lx && j < nd) ? Bdb[r + nx * j] * Ts : 0.0;
                M0[r + NX * j] = (ly && j < nx) ? Cb[r + ny * j] : 0.0;
            }
        }
        w.sync();
        c2d_mul<NX>(M1, M2, rr, nx, nd, acc);              // Bt
        c2d_store<NX>(M4, r, act, acc);
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j) bad = bad || (lx && !c2d_fin(acc[j]));
        c2d_mul<NX>(M0, M1, rr, nx, nx, acc);              // Ct
        c2d_store<NX>(M6, r, act, acc);
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j) bad = bad || (ly && !c2d_fin(acc[j]));
        w.sync();
        if (act) {
            MPCQP_UNROLL
            for (int j = 0; j < NX; ++j) M2[r + NX * j] = (lx && j < nd) ? Bdb[r + nx * j] : 0.0;
        }
        w.sync();
        c2d_mul<NX>(M6, M2, rr, nx, nd, acc);              // Dt
        MPCQP_UNROLL
        for (int j = 0; j < NX; ++j) {
            acc[j] = (ly && j < nd) ? Ddb[r + ny * j] + ah * acc[j] : 0.0;
            bad = bad || !c2d_fin(acc[j]);
        }
        c2d_store<NX>(M0, r, act, acc);
    }
    if (w.any(bad)) return C2D_REFUSED;
    w.sync();

    // ---- the augmented model, row i of every matrix by lane i (Cs_u and Cs_y hold 0 and 1 only: copies of columns; the +0.0
    // is what the product Bu Cs_u makes of a -0.0)
    const bool zohd = nd > 0 && !tust;
    double* Ah = a.Ahat + (size_t)b * nxh * nxh;
    double* Bh = a.Bhu + (size_t)b * nxh * nu;
    double* Ch = a.Chat + (size_t)b * ny * nxh;
    for (int i = r; i < nxh; i += WAVE) {
        const int si = i - nxd;
        for (int j = 0; j < nxh; ++j) {
            double x = 0.0;
            if (j < nxd) {
                if (i < nx && j < nx) x = M5[i + NX * j];
                else if (tust && i >= nx && i < nxd && j >= nx) x = M3[(i - nx) + NX * (j - nx)];
            } else {
                const int sj = j - nxd;
                if (i < nx) x = a.s_in[sj] >= 0 ? M5[i + NX * (nx + a.s_in[sj])] + 0.0 : 0.0;
                else if (si >= 0) x = (sj == si || (sj == si - 1 && a.s_prev[si])) ? 1.0 : 0.0;
            }
            Ah[i + nxh * j] = x;
        }
        for (int c = 0; c < nu; ++c) Bh[i + nxh * c] = i < nx ? M5[i + NX * (nx + c)] : 0.0;
        if (nd > 0) {
            double* Bdh = a.Bhd + (size_t)b * nxh * nd;
            for (int e = 0; e < nd; ++e) {
                double x = 0.0;
                if (zohd && i < nx) x = M5[i + NX * (nx + nu + e)];
                else if (tust && i >= nx && i < nxd) x = M4[(i - nx) + NX * e];
                Bdh[i + nxh * e] = x;
            }
        }
        if (dopb) a.dophat[(size_t)b * nxh + i] = i < nxd ? dopb[i] : 0.0;
    }
    for (int i = r; i < ny; i += WAVE) {
        MPCQP_UNROLL4
        for (int j = 0; j < nxh; ++j) {
            double x = 0.0;
            if (j < nx) x = Cb[i + ny * j];
            else if (j < nxd) x = M6[i + NX * (j - nx)];
            else x = a.s_out[j - nxd] == i ? 1.0 : 0.0;
            Ch[i + ny * j] = x;
        }
        if (nd > 0) {
            double* Ddh = a.Dhd + (size_t)b * ny * nd;
            for (int e = 0; e < nd; ++e) Ddh[i + ny * e] = tust ? M0[i + NX * e] : Ddb[i + ny * e];
        }
    }
    return C2D_OK;
}

template <int NX, class W>
MPCQP_HD void c2d_body(W& w, const C2dArgs& a, int b, double* sm) {
    const int st = c2d_member<NX>(w, a, b, sm);
    if (w.lane == 0) a.status[b] = st;
}

}  // namespace c2d
}  // namespace mpcqp
