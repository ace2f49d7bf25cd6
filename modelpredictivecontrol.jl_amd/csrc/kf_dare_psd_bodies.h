// kf_dare_psd_bodies.h -- the steady-state Riccati solve of kf_dare_bodies.h for a positive SEMIdefinite Q̂: process noise
// that enters through fewer channels than there are states (Q̂ = B_w B_w'), delay or shift-register states, a σQ with zeros
// -- what the reference takes as a matter of course (ControlSystemsBase.kalman, src/estimator/kalman.jl:205-222).
//
// The doubling iteration is that of kf_dare_body, update for update: A(k), G(k), H(k), the symmetrisations, DARE_TOL,
// DARE_MAX_ITER and the gain at the end; the convergence test has one more condition (below).  What changes is how
// S = (H⁻¹ + G)⁻¹ is formed, because
// H(k) -- Q̂ at k = 0 and the covariance after 2^k periods later, singular for good where a mode carries no noise -- has no
// inverse:
//     H = L L'                        unpivoted Cholesky factor of the semidefinite H(k) (Ops::chol_psd); a pivot <= 0
//                                     drops its column
//     S = L (I + L' G L)⁻¹ L'         I + L'GL is symmetric positive definite with pivots >= 1: Ops::gj and its test serve
// which is (H⁻¹ + G)⁻¹ wherever H⁻¹ exists (push-through identity) and its limit where it does not.  A pivot of H(k) below
// -DARE_PSD_NEG max(1, max diag H(k)) is not rounding: the estimator breaks down (DARE_BROKE_DOWN), as an indefinite Q̂
// must.  Per iteration: one factorisation, one inverse, ten products (two more than the definite body), five transposes.
//
// Convergence: H(k+1) - H(k) = A(k)' S A(k).  With a definite S a small step means a small A(k) -- the closed-loop
// transition matrix over 2^k periods has died out and H is the stabilising solution.  A singular S does not say that: a
// mode that no noise reaches leaves H alone whether it decays or not, and for a pole ON the unit circle (an output
// integrator with a zero in Q̂: no stabilising solution exists, SciPy and the reference raise) H converges in a few
// iterations to a P̂ whose estimator keeps that pole.  So an estimator has converged when H has stopped moving AND
// max|A(k+1)| <= DARE_PSD_STAB: a stable mode gets there (at the price of an iteration or two, which leave H as it is),
// the silent integrator keeps its 1 in A(k) and ends at the cap with DARE_NOT_CONVERGED.
//
// A SECOND PASS over the batch (launch_kf_dare_psd, kf_dare_launch.h): an estimator takes part if the definite body left
// it DARE_BROKE_DOWN, or if its Q̂ is numerically singular (smallest pivot <= DARE_PSD_SING max diag Q̂: the definite
// body can get through such a Q̂ on a rounding-sized positive pivot and then answers status 0 with a wrong P̂∞).  Every other
// estimator is frozen by selects from the start -- it never runs, and its K̂, P̂∞, status, iters and path are not written --
// and a wavefront none of whose groups holds a candidate moves on after one vote, so a batch of definite Q̂ pays one launch
// that reads Q̂ and the status words and factors Q̂ once.  A candidate gets path = 1 and the status and iteration count of
// this pass, whatever they are.  One that fails here after the definite body wrote a result gets zeros in K̂ and P̂∞: a
// non-zero status never comes with a gain of this solve.
//
// Padding, independence and memory are those of kf_dare_body: the padded block of H is the identity, so is that of L, of
// I + L'GL (G is zero there) and of S; every estimator makes its own reductions, finished ones are frozen by selects, the
// loop exits on W::any(running), and K̂, P̂∞ are written for DARE_OK only.
#pragma once
#include "kf_cov_bodies.h"
#include "kf_dare_launch.h"

namespace mpcqp {
namespace kf {

template <class W, int NX>
MPCQP_HD void kf_dare_psd_body(W& w, const DareArgs& a, int wave_id) {
    using O = mhe::Ops<W, NX>;
    using mhe::sfor;
    typename O::Row A, G, H, S, T, U, X;
    constexpr int RL = mhe::WaveGeom<W>::GL, GPW = mhe::WaveGeom<W>::GPW;
    O op{w};
    const int lane = w.lane, r = lane & (RL - 1), g = lane / RL;
    const int nx = a.nx, ny = a.ny, nym = a.nym;
    const int my = r < nym ? a.i_ym[r] : 0;            // the row of Ĉ this lane holds as row r of Ĉm
    const bool own = r < NX;                           // this lane owns a row of the padded operands (the others: anything)
    auto transpose = [&](const typename O::Row& M, typename O::Row& D) {      // D = M'
        typename O::Row I;
        sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; I[c] = r == c ? 1.0 : 0.0; D[c] = 0.0; });
        op.mmt_acc(I, M, D, 1.0);
    };
    auto symmetrise = [&](typename O::Row& M, typename O::Row& Tmp) {         // M = ½ (M + M')
        transpose(M, Tmp);
        sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; M[c] = 0.5 * (M[c] + Tmp[c]); });
    };
    for (int wg = wave_id; wg * GPW < a.B; wg += a.nwaves) {
        const int bq = wg * GPW + g;
        const bool live = bq < a.B;
        const int b = live ? bq : a.B - 1;
        const double* Ab = a.Ahat + (size_t)b * nx * nx;
        const double* Cb = a.C + (size_t)b * ny * nx;
        const double* Qb = a.Q + (size_t)b * nx * nx;
        const double* Rb = a.R + (size_t)b * nym * nym;
        // the estimators the first pass could not serve, or should not have served (a numerically singular Q̂ that got
        // through its pivot test on a rounding-sized positive pivot); the others are frozen from here on
        double qd = 0.0;                           // this lane's diagonal entry of Q̂, then the largest of the estimator
        sfor<NX>([&](auto ic) {
            constexpr int c = decltype(ic)::v;
            S[c] = (r < nx && c < nx) ? Qb[c * nx + r] : 0.0;
            qd = (r == c) ? S[c] : qd;
        });
        qd = w.rmax(own ? qd : 0.0);
        // (the padding carries max diag Q̂, so that its pivots are neither the smallest nor out of scale)
        sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; S[c] = (r == c && r >= nx) ? (qd > 0.0 ? qd : 1.0) : S[c]; });
        double qmin;
        op.chol_psd(S, U, r, qmin);
        const int st1 = a.status[b];               // what the first pass said
        const bool cand = live && (st1 == DARE_BROKE_DOWN || !(qmin > DARE_PSD_SING * qd));
        if (!w.any(cand)) continue;
        // ---- G(0) = Ĉm' R̂⁻¹ Ĉm, A(0) = Â', H(0) = Q̂
        sfor<NX>([&](auto ic) {
            constexpr int c = decltype(ic)::v;
            T[c] = (r < nym && c < nym) ? Rb[c * nym + r] : (r == c ? 1.0 : 0.0);          // R̂, identity in the padding
            S[c] = (r < nym && c < nx) ? Cb[my + ny * c] : 0.0;                            // Ĉm  (row = measured output)
            X[c] = (r < nx && c < nym) ? Cb[a.i_ym[c] + ny * r] : 0.0;                     // Ĉm' (row = state)
        });
        bool good = op.gj(T, r);                   // R̂⁻¹; false: a pivot of its LDL' is not in (0, inf)
        op.mm(T, S, U);                            // R̂⁻¹ Ĉm
        op.mm(X, U, G);                            // Ĉm' (R̂⁻¹ Ĉm)
        symmetrise(G, T);
        sfor<NX>([&](auto ic) {
            constexpr int c = decltype(ic)::v;
            const bool in_x = r < nx && c < nx;
            A[c] = in_x ? Ab[r * nx + c] : 0.0;                                            // Â' (row r = column r of Â)
            H[c] = in_x ? Qb[c * nx + r] : (r == c ? 1.0 : 0.0);                           // Q̂, identity in the padding
        });
        // ---- doubling iterations.  run, conv, good and it are the same on every lane of an estimator (they follow from
        // broadcasts and reductions over its lanes)
        bool run = good && cand, conv = false;
        int it = 0;
        for (int k = 0; k < DARE_MAX_ITER; ++k) {
            if (!w.any(run)) break;
            // S = L (I + L' G L)⁻¹ L' with H = L L'                                   L -> U
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; S[c] = H[c]; });
            double hmin;
            bool ok = op.chol_psd(S, U, r, hmin) >= -DARE_PSD_NEG;
            op.mm(G, U, T);                        // G L
            transpose(U, X);                       // L'
            op.mm(X, T, S);                        // L' G L
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; S[c] += r == c ? 1.0 : 0.0; });
            ok = op.gj(S, r) && ok;                // (I + L' G L)⁻¹
            op.mm(U, S, T);                        // L (I + L' G L)⁻¹
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; S[c] = 0.0; });
            op.mmt_acc(T, U, S, 1.0);              // ... L'
            symmetrise(S, T);
            // H(k+1) = H + A' S A                                                     -> U
            transpose(A, X);
            op.mm(S, A, T);
            op.mm(X, T, U);
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; U[c] += H[c]; });
            symmetrise(U, X);
            // W = I - G S -> T,   G - G S G -> S
            op.mm(G, S, T);
            op.mm(T, G, X);
            sfor<NX>([&](auto ic) {
                constexpr int c = decltype(ic)::v;
                S[c] = G[c] - X[c];
                T[c] = (r == c ? 1.0 : 0.0) - T[c];
            });
            // G(k+1) = G + A (G - G S G) A'                                           -> S
            op.mm(A, S, X);
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; S[c] = G[c]; });
            op.mmt_acc(X, A, S, 1.0);
            symmetrise(S, X);
            // A(k+1) = A W A                                                          -> T
            op.mm(A, T, X);
            op.mm(X, A, T);
            // this estimator's own test: finite, and how far H moved
            double fin = 1.0, dmax = 0.0, hmax = 0.0, amax = 0.0;
            sfor<NX>([&](auto ic) {
                constexpr int c = decltype(ic)::v;
                fin = (U[c] - U[c] == 0.0 && S[c] - S[c] == 0.0 && T[c] - T[c] == 0.0) ? fin : 0.0;
                dmax = fmax(dmax, fabs(U[c] - H[c]));
                hmax = fmax(hmax, fabs(U[c]));
                amax = fmax(amax, fabs(T[c]));
            });
            const bool step_ok = (w.rmin(own ? fin : 1.0) > 0.5) && ok;        // (every lane takes part in the reductions)
            dmax = w.rmax(own ? dmax : 0.0);
            hmax = w.rmax(own ? hmax : 0.0);
            amax = w.rmax(own ? amax : 0.0);
            const bool upd = run && step_ok;
            sfor<NX>([&](auto ic) {
                constexpr int c = decltype(ic)::v;
                A[c] = upd ? T[c] : A[c];
                G[c] = upd ? S[c] : G[c];
                H[c] = upd ? U[c] : H[c];
            });
            it += run ? 1 : 0;
            good = good && (step_ok || !run);
            // (with a singular S a mode can leave H alone without dying out -- a pole on the unit circle that no noise
            // reaches: H has then converged to a solution that does not stabilise, and A(k) says so)
            const bool cv = dmax <= DARE_TOL * fmax(1.0, hmax) && amax <= DARE_PSD_STAB;
            conv = conv || (upd && cv);
            run = upd && !cv;
        }
        // ---- K̂ = P̂∞ Ĉm' (Ĉm P̂∞ Ĉm' + R̂)⁻¹, as kf_cov_body's correction forms it
        sfor<NX>([&](auto ic) {
            constexpr int c = decltype(ic)::v;
            S[c] = (r < nym && c < nx) ? Cb[my + ny * c] : 0.0;
            T[c] = (r < nym && c < nym) ? Rb[c * nym + r] : (r == c ? 1.0 : 0.0);
            U[c] = 0.0;
        });
        op.mmt_acc(H, S, U, 1.0);                  // P̂ Ĉm'            (row = state, column = output)
        op.mm_add(S, U, T);                        // M̂ = R̂ + Ĉm (P̂ Ĉm')
        bool okg = op.gj(T, r);
        op.mm(U, T, X);                            // K̂
        double fin = 1.0;
        sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; fin = (X[c] - X[c] == 0.0) ? fin : 0.0; });
        okg = (w.rmin(own ? fin : 1.0) > 0.5) && okg;
        const int st = !(good && (okg || !conv)) ? DARE_BROKE_DOWN : conv ? DARE_OK : DARE_NOT_CONVERGED;
        if (cand && st == DARE_OK && r < nx) {
            double* Pb = a.P + (size_t)b * nx * nx;
            double* Kb = a.K + (size_t)b * nym * nx;
            sfor<NX>([&](auto ic) {
                constexpr int c = decltype(ic)::v;
                if (c < nx) Pb[c * nx + r] = H[c];
                if (c < nym) Kb[c * nx + r] = X[c];
            });
        }
        // a candidate that the first pass had served (a numerically singular Q̂ that got through its pivot test) and that
        // this pass refuses: what the first pass wrote is the result this pass exists to distrust -- zeros instead
        if (cand && st != DARE_OK && st1 == DARE_OK && r < nx) {
            double* Pb = a.P + (size_t)b * nx * nx;
            double* Kb = a.K + (size_t)b * nym * nx;
            sfor<NX>([&](auto ic) {
                constexpr int c = decltype(ic)::v;
                if (c < nx) Pb[c * nx + r] = 0.0;
                if (c < nym) Kb[c * nx + r] = 0.0;
            });
        }
        if (cand && r == 0) {
            a.status[b] = st;
            a.iters[b] = it;
            a.path[b] = 1;
        }
    }
}

}  // namespace kf
}  // namespace mpcqp
