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
// until max|H(k+1) - H(k)| <= DARE_TOL max(1, max|H(k+1)|);  P̂∞ = H,  K̂ = P̂∞ Ĉm' (Ĉm P̂∞ Ĉm' + R̂)⁻¹ (the filter-form gain,
// in the order of operations of kf_cov_body's correction).  Iteration k holds the covariance after 2^k periods of the
// recursion, which is why a dozen of them do what the fixed-point iteration needs hundreds for.  H(0)⁻¹ needs Q̂ positive
// definite: a semidefinite Q̂ breaks down here (status 2) and goes to the second pass (kf_dare_psd_bodies.h).
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
#pragma once
#include "kf_cov_bodies.h"
#include "kf_dare_launch.h"

namespace mpcqp {
namespace kf {

template <class W, int NX>
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
        bool run = good, conv = false;
        int it = 0;
        for (int k = 0; k < DARE_MAX_ITER; ++k) {
            if (!w.any(run)) break;
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; S[c] = H[c]; });
            bool ok = op.gj(S, r);                 // H⁻¹
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; S[c] += G[c]; });
            ok = op.gj(S, r) && ok;                // S = (H⁻¹ + G)⁻¹
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
            double fin = 1.0, dmax = 0.0, hmax = 0.0;
            sfor<NX>([&](auto ic) {
                constexpr int c = decltype(ic)::v;
                fin = (U[c] - U[c] == 0.0 && S[c] - S[c] == 0.0 && T[c] - T[c] == 0.0) ? fin : 0.0;
                dmax = fmax(dmax, fabs(U[c] - H[c]));
                hmax = fmax(hmax, fabs(U[c]));
            });
            const bool step_ok = (w.rmin(own ? fin : 1.0) > 0.5) && ok;        // (every lane takes part in the reductions)
            dmax = w.rmax(own ? dmax : 0.0);
            hmax = w.rmax(own ? hmax : 0.0);
            const bool upd = run && step_ok;
            sfor<NX>([&](auto ic) {
                constexpr int c = decltype(ic)::v;
                A[c] = upd ? T[c] : A[c];
                G[c] = upd ? S[c] : G[c];
                H[c] = upd ? U[c] : H[c];
            });
            it += run ? 1 : 0;
            good = good && (step_ok || !run);
            const bool cv = dmax <= DARE_TOL * fmax(1.0, hmax);
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
        if (live && st == DARE_OK && r < nx) {
            double* Pb = a.P + (size_t)b * nx * nx;
            double* Kb = a.K + (size_t)b * nym * nx;
            sfor<NX>([&](auto ic) {
                constexpr int c = decltype(ic)::v;
                if (c < nx) Pb[c * nx + r] = H[c];
                if (c < nym) Kb[c * nx + r] = X[c];
            });
        }
        if (live && r == 0) {
            a.status[b] = st;
            a.iters[b] = it;
        }
    }
}

}  // namespace kf
}  // namespace mpcqp
