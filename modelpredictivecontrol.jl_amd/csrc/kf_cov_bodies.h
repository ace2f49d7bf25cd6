// kf_cov_bodies.h -- covariance and gain recursion of the time-varying KalmanFilter of the LinMPC loop, written against
// a wave interface W like mhe_bodies.h (gfx950: MheDevWave, one estimator per 16-lane DPP row; the wide interface, one
// estimator per wavefront with the NX^3 products on the matrix cores; CPU emulator: tests/emu/emu_kf_cov.cpp).
//
// What the reference does per period (one estimator, direct = true):
//   correct_estimate_kf!  src/estimator/kalman.jl:1235-1264  -> mode bit 0 (COV_CORRECT)
//       P̂Ĉm' = P̂ Ĉm';  M̂ = Ĉm (P̂Ĉm') + R̂;  K̂ = (P̂Ĉm') M̂⁻¹;  P̂ <- (I - K̂ Ĉm) P̂
//   predict_estimate_kf!  src/estimator/kalman.jl:1275-1290  -> mode bit 1 (COV_PREDICT)
//       P̂ <- Â (P̂ Â') + Q̂
// in that order of operations.  The recursion depends on WHICH measurements are missing and on nothing else in the data,
// so it runs as a kernel of its own ahead of the step on the same stream and hands K̂(k) to every step kernel through the
// gain buffer they already read.
//
// Missed corrections (kalman.jl:478-484, "NaN values in the Kalman filter measurements ym: skipping correction step"): an
// estimator whose row of CovArgs::y0m holds a NaN -- or every estimator of a COV_NO_YM launch -- keeps P̂ and K̂ bit for bit
// and gets COV_MISSED.  The prediction of that period runs, from P̂(k|k-1).  Every lane reads the nym entries of its own
// estimator's row (the same addresses within a DPP row here, within the wavefront in the wide family: no cross-lane
// operation, no register held beyond the flag); the products of the correction are computed all
// the same and discarded by the selects that already serve the drop policy, so the other estimators of the wavefront see
// the same instruction stream whoever misses.
//
// Symmetry: the corrected covariance is stored as ½ (P̂ + P̂') (what oracle/mhe.py keeps; the reference takes
// Hermitian(P̂, :L)), the predicted one as computed -- Â P̂ Â' + Q̂ of a symmetric P̂ is symmetric up to rounding, and the
// next correction symmetrises again.
//
// Dropped updates (the correct_cov! policy of mhe_bodies.h cov_body, where the reference's cholesky! would throw): a
// correction whose M̂ is not positive definite or not finite, or whose new P̂ / K̂ is not finite, is dropped for THAT
// estimator -- P̂ and K̂ keep their values, its status becomes COV_DROPPED.  The prediction of a period whose correction
// was dropped is skipped as well (there is no P̂(k|k) to predict from: P̂ stays P̂(k|k-1) until a correction succeeds, which
// puts the status back to COV_OK); so is a prediction that is not finite.  The neighbours in the wavefront are unaffected.
//
// Nothing is inverted but M̂ (Ops::gj), and P̂ never leaves the registers between the two halves of mode 3: the arithmetic
// of mode 3 is that of mode 1 followed by mode 2, so a fused period equals the separate calls bit for bit.
#pragma once
#include "kf_cov_launch.h"
#include "mhe_bodies.h"

namespace mpcqp {
namespace kf {

// Ĉm: the measured rows of Ĉ [ny x nx], lane r holds the row of measured output r (row my = i_ym[r] of Ĉ) ...
template <int NX>
MPCQP_HD void ld_cm(const double* Cb, int my, int ny, int nym, int nx, int r, double (&M)[NX]) {
    mhe::sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; M[c] = (r < nym && c < nx) ? Cb[my + ny * c] : 0.0; });
}
// ... and Ĉm': lane r holds the row of state r, column c is measured output c
template <int NX>
MPCQP_HD void ld_cmt(const double* Cb, const int* i_ym, int ny, int nym, int nx, int r, double (&M)[NX]) {
    mhe::sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; M[c] = (r < nx && c < nym) ? Cb[i_ym[c] + ny * r] : 0.0; });
}

// K̂ = P̂ Ĉm' (Ĉm P̂ Ĉm' + R̂)⁻¹ in the order of operations of correct_estimate_kf!.  M: in R̂ (the identity in the padding), out
// M̂⁻¹;  PC: out P̂ Ĉm' (row = state, column = output).  false: a pivot of the LDL' of M̂ is not in (0, inf).
template <class W, int NX>
MPCQP_HD bool kf_gain(const mhe::Ops<W, NX>& op, int r, const double (&P)[NX], const double (&Cm)[NX], double (&M)[NX],
                      double (&PC)[NX], double (&K)[NX]) {
    mhe::sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; PC[c] = 0.0; });
    op.mmt_acc(P, Cm, PC, 1.0);            // P̂ Ĉm'
    op.mm_add(Cm, PC, M);                  // M̂ = R̂ + Ĉm (P̂ Ĉm')
    const bool good = op.gj(M, r);         // M̂⁻¹
    op.mm(PC, M, K);                       // K̂ = (P̂ Ĉm') M̂⁻¹
    return good;
}

template <class W, int NX>
MPCQP_HD void kf_cov_body(W& w, const CovArgs& a, int mode, int wave_id) {
    using O = mhe::Ops<W, NX>;
    using mhe::sfor;
    typename O::Row P, S, G, M, X;
    constexpr int RL = mhe::WaveGeom<W>::GL, GPW = mhe::WaveGeom<W>::GPW;
    O op{w};
    const int lane = w.lane, r = lane & (RL - 1), g = lane / RL;
    const int nx = a.nx, ny = a.ny, nym = a.nym;
    const int my = r < nym ? a.i_ym[r] : 0;            // the row of Ĉ this lane holds as row r of Ĉm
    for (int wg = wave_id; wg * GPW < a.B; wg += a.nwaves) {
        const int bq = wg * GPW + g;
        const bool live = bq < a.B;
        const int b = live ? bq : a.B - 1;
        const double* Ab = a.Ahat + (size_t)b * nx * nx;
        const double* Cb = a.C + (size_t)b * ny * nx;
        const double* Qb = a.Q + (size_t)b * nx * nx;
        const double* Rb = a.R + (size_t)b * nym * nym;
        double* Pb = a.P + (size_t)b * nx * nx;
        double* Kb = a.K + (size_t)b * nym * nx;
        O::ld_sq(Pb, nx, r, 0.0, P);
        bool dropped = false, changed = false;
        if (mode & COV_CORRECT) {
            // any(isnan, y0m) of this estimator (Inf is a measurement)
            bool missed = false;
            if (a.y0m) {
                const double* yb = a.y0m + (size_t)b * nym;
                for (int i = 0; i < nym; ++i) missed = missed || yb[i] != yb[i];
            }
            ld_cm(Cb, my, ny, nym, nx, r, S);      // Ĉm (row = measured output)
            O::ld_sq(Rb, nym, r, 1.0, M);          // R̂, identity in the padding
            bool good = kf_gain(op, r, P, S, M, G, X);
            op.mm(X, S, G);                        // K̂ Ĉm
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; G[c] = (r == c ? 1.0 : 0.0) - G[c]; });
            op.mm(G, P, M);                        // (I - K̂ Ĉm) P̂
            op.symmetrise(M, G, r);
            good = op.all_finite(r, M, X) && good;           // (every lane takes part in the vote: not behind `good &&`)
            const bool apply = good && !missed;
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; P[c] = apply ? M[c] : P[c]; });
            if (live && apply && r < nx)
                sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; if (c < nym) Kb[c * nx + r] = X[c]; });
            if (live && r == 0) a.status[b] = missed ? COV_MISSED : good ? COV_OK : COV_DROPPED;
            dropped = !good && !missed;
            changed = apply;
        } else if (mode & COV_NO_YM) {
            if (live && r == 0) a.status[b] = COV_MISSED;
        } else if (mode & COV_PREDICT) {
            dropped = a.status[b] == COV_DROPPED;
        }
        if (mode & COV_PREDICT) {
            O::ld_sq(Ab, nx, r, 0.0, S);
            O::ld_sq(Qb, nx, r, 0.0, M);
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; G[c] = 0.0; });
            op.mmt_acc(P, S, G, 1.0);              // P̂ Â'
            op.mm_add(S, G, M);                    // Q̂ + Â (P̂ Â')
            const bool finite = op.all_finite(r, M);
            const bool keep = finite && !dropped;
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; P[c] = keep ? M[c] : P[c]; });
            if (live && r == 0 && !finite && !dropped) a.status[b] = COV_DROPPED;
            changed = changed || keep;
        }
        if (live && changed && r < nx)
            sfor<NX>([&](auto ic) { constexpr int c = decltype(ic)::v; if (c < nx) Pb[c * nx + r] = P[c]; });
    }
}

}  // namespace kf
}  // namespace mpcqp
