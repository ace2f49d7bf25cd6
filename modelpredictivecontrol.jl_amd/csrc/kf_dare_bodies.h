// kf_dare_bodies.h -- steady-state gain of the SteadyKalmanFilter from Q̂ and R̂: the discrete algebraic Riccati equation of
// the predictor form
//     P = Â P Â' - Â P Ĉm' (Ĉm P Ĉm' + R̂)⁻¹ Ĉm P Â' + Q̂
// solved for every estimator of the batch by the structure-preserving doubling iteration, on the wave interface and the
// row-lane Ops of kf_cov_bodies.h (gfx950: one estimator per 16-lane DPP row, or one per wavefront with the NX^3 products
// on the matrix cores; CPU emulator: tests/emu/emu_kf_dare.cpp).  What the reference does once per estimator on the host
// (ControlSystemsBase.kalman in src/estimator/kalman.jl:205-222) and refuses to redo after setmodel! (kalman.jl:229-232).
//
//     A(0) = Â',  G(0) = Ĉm' R̂⁻¹ Ĉm,  H(0) = Q̂
//     S      = (H(k)⁻¹ + G(k))⁻¹                       two unpivoted inverses of symmetric positive definite matrices
//     W      = I - G(k) S
//     A(k+1) = A(k) W A(k)
//     G(k+1) = G(k) + A(k) (G(k) - G(k) S G(k)) A(k)'
//     H(k+1) = H(k) + A(k)' S A(k)
// until max|H(k+1) - H(k)| <= DARE_TOL max(1, max|H(k+1)|);  P̂∞ = H,  K̂ = P̂∞ Ĉm' (Ĉm P̂∞ Ĉm' + R̂)⁻¹ (the filter-form gain:
// kf_gain of kf_cov_bodies.h, which kf_cov_body's correction uses too).  Iteration k holds the covariance after 2^k periods of the
// recursion, which is why a dozen of them do what the fixed-point iteration needs hundreds for.  H(0)⁻¹ needs Q̂ positive
// definite: a semidefinite Q̂ breaks down here (status 2) and goes to the second pass, the same body in its square-root
// form (PSD = true, below; kf_dare_psd_body of kf_dare_psd_bodies.h names that instantiation).
//
// Symmetry: S, G(k+1) and H(k+1) are stored as ½ (M + M').  A transpose is the product I M' (Ops::mmt_acc with the identity:
// every term is a value times 0 or 1, so it is exact), which keeps the body on the existing Ops: eight products, four
// transposes and two inverses per iteration.
//
// Padding: rows / columns nx .. NX-1 carry the identity in H and zeros in A and G; S and W then carry the identity there,
// A and G stay zero and H stays the identity -- the padded block never reaches the estimator's own entries, and its ones
// do not move the test (it compares with max(1, .)).
//
// Independence: every estimator tests its own convergence with a reduction over its own lanes.  One that has converged,
// broken down or (in a partly filled group) does not exist is frozen by selects -- its A, G and H keep their bits while its
// neighbours iterate on -- and the wavefront leaves the loop when none of its estimators is running (W::any, the one
// wave-wide operation), so an estimator's result does not depend on who shares its wavefront.  K̂, P̂∞ are written for
// DARE_OK only: a failed estimator keeps what the arrays held.
//
// Memory: Â, Q̂, R̂ and the measured rows of Ĉ are read once before the loop, Ĉm and R̂ a second time for the gain (holding
// them across the loop would cost two more rows of registers for two reads per solve); K̂, P̂∞, status and the iteration
// count are written once.
//
// THE SQUARE-ROOT FORM (PSD = true) serves a positive SEMIdefinite Q̂: process noise that enters through fewer channels than
// there are states (Q̂ = B_w B_w'), delay or shift-register states, a σQ with zeros -- what the reference takes as a matter
// of course.  The iteration is the one above, update for update: A(k), G(k), H(k), the symmetrisations, DARE_TOL,
// DARE_MAX_ITER and the gain at the end.  What changes is how S = (H⁻¹ + G)⁻¹ is formed, because H(k) -- Q̂ at k = 0 and
// the covariance after 2^k periods later, singular for good where a mode carries no noise -- has no inverse:
//     H = L L'                        unpivoted Cholesky factor of the semidefinite H(k) (Ops::chol_psd); a pivot <= 0
//                                     drops its column
//     S = L (I + L' G L)⁻¹ L'         I + L'GL is symmetric positive definite with pivots >= 1: Ops::gj and its test serve
// which is (H⁻¹ + G)⁻¹ wherever H⁻¹ exists (push-through identity) and its limit where it does not.  A pivot of H(k) below
// -DARE_PSD_NEG max(1, max diag H(k)) is not rounding: the estimator breaks down (DARE_BROKE_DOWN), as an indefinite Q̂
// must.  Per iteration: one factorisation, one inverse, ten products (two more than the definite form), five transposes.
// The padded block of H is the identity, so is that of L, of I + L'GL (G is zero there) and of S.
//
// Its convergence test has one more condition.  H(k+1) - H(k) = A(k)' S A(k): with a definite S a small step means a small
// A(k) -- the closed-loop transition matrix over 2^k periods has died out and H is the stabilising solution.  A singular S
// does not say that: a mode that no noise reaches leaves H alone whether it decays or not, and for a pole ON the unit
// circle (an output integrator with a zero in Q̂: no stabilising solution exists, SciPy and the reference raise) H
// converges in a few iterations to a P̂ whose estimator keeps that pole.  So an estimator has converged when H has stopped
// moving AND max|A(k+1)| <= DARE_PSD_STAB: a stable mode gets there (at the price of an iteration or two, which leave H
// as it is), the silent integrator keeps its 1 in A(k) and ends at the cap with DARE_NOT_CONVERGED.
//
// It runs as A SECOND PASS over the batch (launch_kf_dare_psd, kf_dare_launch.h): an estimator takes part (`cand`) if the
// definite form left it DARE_BROKE_DOWN, or if its Q̂ is numerically singular (smallest pivot <= DARE_PSD_SING max diag Q̂:
// the definite form can get through such a Q̂ on a rounding-sized positive pivot and then answers status 0 with a wrong
// P̂∞).  Every other estimator is frozen by selects from the start -- it never runs, and its K̂, P̂∞, status, iters and path
// are not written -- and a wavefront none of whose groups holds a candidate moves on after one vote, so a batch of
// definite Q̂ pays one launch that reads Q̂ and the status words and factors Q̂ once.  A candidate gets path = 1 and the
// status and iteration count of this pass, whatever they are.  One that fails here after the definite form wrote a result
// gets zeros in K̂ and P̂∞: a non-zero status never comes with a gain of this solve.
#pragma once
#include "kf_cov_bodies.h"
#include "kf_dare_launch.h"

namespace mpcqp {
namespace kf {

// PSD: the square-root form (second pass); false: the definite form
template <class W, int NX, bool PSD = false>
MPCQP_HD void kf_dare_body(W& w, const DareArgs& a, int wave_id) {
    using O = mhe::Ops<W, NX>;
    using mhe::sfor;
    typename O::Row A, G, H, S, T, U, X;
    constexpr int RL = mhe::WaveGeom<W>::GL, GPW = mhe::WaveGeom<W>::GPW;
    O op{w};
    const int lane = w.lane, r = lane & (RL - 1), g = lane / RL;
    const int nx = a.nx, ny = a.ny, nym = a.nym;
    const int my = r < nym ? a.i_ym[r] : 0;            // the row of Ĉ this lane holds as row r of Ĉm
    const bool own = r < NX;                           // this lane owns a row of the padded operands (the others: anything)
    for (int wg = wave_id; wg * GPW < a.B; wg += a.nwaves) {
        const int bq = wg * GPW + g;
        const bool live = bq < a.B;
        const int b = live ? bq : a.B - 1;
        const double* Ab = a.Ahat + (size_t)b * nx * nx;
        const double* Cb = a.C + (size_t)b * ny * nx;
        const double* Qb = a.Q + (size_t)b * nx * nx;
        const double* Rb = a.R + (size_t)b * nym * nym;
        // the estimators this pass serves and writes: the first pass every one that exists ...
        bool cand = live;
        int st1 = DARE_BROKE_DOWN;                 // what the first pass said (second pass only)
        if constexpr (PSD) {
            // ... the second those the first could not serve, or should not have served (a numerically singular Q̂ that got
            // through its pivot test on a rounding-sized positive pivot); the others are frozen from here on
            double qd = 0.0;                       // this lane's diagonal entry of Q̂, then the largest of the estimator
            O::ld_sq(Qb, nx, r, 0.0, S);
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; qd = (r == c) ? S[c] : qd; });
            qd = w.rmax(own ? qd : 0.0);
            // (the padding carries max diag Q̂, so that its pivots are neither the smallest nor out of scale)
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; S[c] = (r == c && r >= nx) ? (qd > 0.0 ? qd : 1.0) : S[c]; });
            double qmin;
            op.chol_psd(S, U, r, qmin);
            st1 = a.status[b];
            cand = live && (st1 == DARE_BROKE_DOWN || !(qmin > DARE_PSD_SING * qd));
            if (!w.any(cand)) continue;
        }
        // ---- G(0) = Ĉm' R̂⁻¹ Ĉm, A(0) = Â', H(0) = Q̂
        O::ld_sq(Rb, nym, r, 1.0, T);              // R̂, identity in the padding
        ld_cm(Cb, my, ny, nym, nx, r, S);          // Ĉm  (row = measured output)
        ld_cmt(Cb, a.i_ym, ny, nym, nx, r, X);     // Ĉm' (row = state)
        bool good = op.gj(T, r);                   // R̂⁻¹; false: a pivot of its LDL' is not in (0, inf)
        op.mm(T, S, U);                            // R̂⁻¹ Ĉm
        op.mm(X, U, G);                            // Ĉm' (R̂⁻¹ Ĉm)
        op.symmetrise(G, T, r);
        O::ld_sq_t(Ab, nx, r, A);                  // Â' (row r = column r of Â)
        O::ld_sq(Qb, nx, r, 1.0, H);               // Q̂, identity in the padding
        // ---- doubling iterations.  run, conv, good and it are the same on every lane of an estimator (they follow from
        // broadcasts and reductions over its lanes).  (The definite body starts from `good` alone: a member of a partly
        // filled group that does not exist iterates on the copy it loaded, and nothing of it is stored.)
        bool run = PSD ? good && cand : good, conv = false;
        int it = 0;
        for (int k = 0; k < DARE_MAX_ITER; ++k) {
            if (!w.any(run)) break;
            bool ok;
            if constexpr (PSD) {
                // S = L (I + L' G L)⁻¹ L' with H = L L'                               L -> U
                sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; S[c] = H[c]; });
                double hmin;
                ok = op.chol_psd(S, U, r, hmin) >= -DARE_PSD_NEG;
                op.mm(G, U, T);                    // G L
                op.transpose(U, X, r);             // L'
                op.mm(X, T, S);                    // L' G L
                sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; S[c] += r == c ? 1.0 : 0.0; });
                ok = op.gj(S, r) && ok;            // (I + L' G L)⁻¹
                op.mm(U, S, T);                    // L (I + L' G L)⁻¹
                sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; S[c] = 0.0; });
                op.mmt_acc(T, U, S, 1.0);          // ... L'
            } else {
                sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; S[c] = H[c]; });
                ok = op.gj(S, r);                  // H⁻¹
                sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; S[c] += G[c]; });
                ok = op.gj(S, r) && ok;            // S = (H⁻¹ + G)⁻¹
            }
            op.symmetrise(S, T, r);
            // H(k+1) = H + A' S A                                                     -> U
            op.transpose(A, X, r);
            op.mm(S, A, T);
            op.mm(X, T, U);
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; U[c] += H[c]; });
            op.symmetrise(U, X, r);
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
            op.symmetrise(S, X, r);
            // A(k+1) = A W A                                                          -> T
            op.mm(A, T, X);
            op.mm(X, A, T);
            // this estimator's own test: finite, and how far H moved (every lane takes part in the reductions).  One pass
            // over the columns for the flag and the maxima, then Ops::vote_finite: with Ops::all_finite and its pass of
            // its own the NX = 16 kernels spill more than they did
            double fin = 1.0, dmax = 0.0, hmax = 0.0, amax = 0.0;
            sfor<NX>([&](auto ic) {
                constexpr int c = decltype(ic)::v;
                fin = (U[c] - U[c] == 0.0 && S[c] - S[c] == 0.0 && T[c] - T[c] == 0.0) ? fin : 0.0;
                dmax = fmax(dmax, fabs(U[c] - H[c]));
                hmax = fmax(hmax, fabs(U[c]));
                if constexpr (PSD) amax = fmax(amax, fabs(T[c]));
            });
            const bool step_ok = op.vote_finite(r, fin) && ok;
            dmax = w.rmax(own ? dmax : 0.0);
            hmax = w.rmax(own ? hmax : 0.0);
            if constexpr (PSD) amax = w.rmax(own ? amax : 0.0);
            const bool upd = run && step_ok;
            sfor<NX>([&](auto ic) {
                constexpr int c = decltype(ic)::v;
                A[c] = upd ? T[c] : A[c];
                G[c] = upd ? S[c] : G[c];
                H[c] = upd ? U[c] : H[c];
            });
            it += run ? 1 : 0;
            good = good && (step_ok || !run);
            // (square-root form: with a singular S a mode can leave H alone without dying out -- a pole on the unit circle
            // that no noise reaches: H has then converged to a solution that does not stabilise, and A(k) says so)
            const bool cv = dmax <= DARE_TOL * fmax(1.0, hmax) && (!PSD || amax <= DARE_PSD_STAB);
            conv = conv || (upd && cv);
            run = upd && !cv;
        }
        // ---- K̂ = P̂∞ Ĉm' (Ĉm P̂∞ Ĉm' + R̂)⁻¹
        ld_cm(Cb, my, ny, nym, nx, r, S);
        O::ld_sq(Rb, nym, r, 1.0, T);
        bool okg = kf_gain(op, r, H, S, T, U, X);
        okg = op.all_finite(r, X) && okg;
        const int st = !(good && (okg || !conv)) ? DARE_BROKE_DOWN : conv ? DARE_OK : DARE_NOT_CONVERGED;
        double* Pb = a.P + (size_t)b * nx * nx;
        double* Kb = a.K + (size_t)b * nym * nx;
        if (cand && st == DARE_OK && r < nx) {
            sfor<NX>([&](auto ic) {
                constexpr int c = decltype(ic)::v;
                if (c < nx) Pb[c * nx + r] = H[c];
                if (c < nym) Kb[c * nx + r] = X[c];
            });
        }
        // a candidate that the first pass had served (a numerically singular Q̂ that got through its pivot test) and that
        // the second refuses: what the first pass wrote is the result the second exists to distrust -- zeros instead
        if (PSD && cand && st != DARE_OK && st1 == DARE_OK && r < nx) {
            sfor<NX>([&](auto ic) {
                constexpr int c = decltype(ic)::v;
                if (c < nx) Pb[c * nx + r] = 0.0;
                if (c < nym) Kb[c * nx + r] = 0.0;
            });
        }
        if (cand && r == 0) {
            a.status[b] = st;
            a.iters[b] = it;
            if constexpr (PSD) a.path[b] = 1;
        }
    }
}

}  // namespace kf
}  // namespace mpcqp
