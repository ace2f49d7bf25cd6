// kf_dare_lds_bodies.h -- steady-state gain of the SteadyKalmanFilter from Q̂ and R̂ for 32 < max(nx̂, nym) <= 64: the
// doubling iteration of kf_dare_bodies.h (definite form; its header states the equations, the padding and the test)
// with another residency.  There a lane holds a row of each of seven operands in registers, which ends at 32 columns.
// Here ONE ESTIMATOR BELONGS TO A WORKGROUP of T wavefronts, its operands live in LDS as padded N x N matrices (row-major,
// leading dimension dare_lds_ld(N)), and a product runs as 16 x 16 output tiles of v_mfma_f64_16x16x4 whose results stay
// in the accumulators of the wavefront that owns the tile until they are written over an operand that is no longer needed
// (gfx950: kf_dare_lds_kernels.hip; CPU emulator, T = 1: tests/emu/emu_kf_dare_lds.cpp).
//
// LDS: four operand buffers -- bA, bG, bH hold A(k), G(k), H(k) between iterations, bX is the work buffer -- and a few
// vectors (kf_dare_lds_launch.h: dare_lds_doubles).  What does not fit is held in accumulator layout in registers: H(k)
// while its buffer carries S A(k), G(k) while its buffer carries G - G S G and then A (G - G S G).  One iteration:
//     bX = H;  bX = bX⁻¹ + G;  bX = bX⁻¹;  bX = ½ (bX + bX')                                   S
//     acc = bX bA;            h = bH;       bH = acc                                            S A
//     acc = h + bA' bH;                     bH = acc;  bH = ½ (bH + bH');  test against h       H(k+1)
//     acc = bG bX;                          bX = acc                                            T = G S
//     acc = bX bG;            g = bG;       bG = g - acc                                        G - G S G
//     acc = bA bG;                          bG = acc                                            A (G - G S G)
//     acc = g + bG bA';                     bG = acc;  bG = ½ (bG + bG')                        G(k+1)
//     acc = bA bX;                          bX = bA - acc                                       A W = A - A T
//     acc = bX bA;                          bA = acc                                            A(k+1)
// eight products, two inverses, three symmetrisations, 2 N + 25 workgroup barriers.
//
// Team: output tile ti (row-major over the N/16 x N/16 tiles) belongs to wavefront ti mod T; element idx of an
// elementwise pass (inverse, copies, symmetrisation) to thread idx mod 64 T.  Who computes an entry changes with T, what
// is computed for it does not: the k order inside a tile is 0, 4, ..., N-4 for every T, every elementwise operation is
// written once, and the reductions are maxima.  So the result is bit-identical for every T; T = 1 has no cross-wave
// hazard and is the yardstick of the others.  Every write of an LDS buffer is separated from its readers by a workgroup
// barrier (W::sync) -- `put` takes one before it stores where the product just finished read the destination.
//
// Inverse: unpivoted Gauss-Jordan in place, the step of Ops::gj (mhe_bodies.h: the pivot row is not divided, every row is
// scaled by its own reciprocal pivot at the end) with its pivot test.  A thread keeps its N² / 64 T entries in registers
// over the N steps; the pivot row and column of step k are copies in LDS scratch that step k-1 wrote while it updated
// them, so a step costs two LDS reads per entry and one barrier.
//
// Exit: the workgroup holds one estimator, so convergence and break-down are workgroup-uniform values (they come from LDS
// words every thread reads, or from reductions) and the loops are left by plain branches.  An estimator's result does not
// depend on B, on the grid or on its neighbours.
//
// Semidefinite Q̂ is not served here (there is no square-root form at this size): the first inverse of the first
// iteration IS the unpivoted factorisation of Q̂ = H(0), and an estimator whose smallest pivot there is <= DARE_PSD_SING
// max diag Q̂ -- the rule by which the second pass of the row-lane kernels picks its candidates -- ends with
// DARE_BROKE_DOWN.  K̂ and P̂∞ are written for DARE_OK only.
#pragma once
#include "kf_dare_launch.h"
#include "kf_dare_lds_launch.h"
#include "mhe_bodies.h"

namespace mpcqp {
namespace kf {

// W: lane (0 .. 63 within the wavefront) and sync() (workgroup barrier).  wv: this wavefront's index in the team.
template <class W, int N, int T>
struct DareLds {
    static_assert(N % 16 == 0 && N <= DARE_LDS_NMAX, "padded order: whole 16 x 16 tiles");
    static constexpr int LD = dare_lds_ld(N), NTL = N / 16, NTILES = NTL * NTL, TPW = (NTILES + T - 1) / T, NTHR = WAVE * T;
    static constexpr int NE = N * N / NTHR;           // entries of a thread in an elementwise pass
    static_assert(NE * NTHR == N * N, "an elementwise pass deals whole rounds of entries to the threads");
    using Acc = double[TPW][4];
    W& w;
    const int wv, tid, li, lk;
    double *bA, *bG, *bH, *bX, *sc, *piv, *red;

    MPCQP_HD DareLds(W& w_, int wv_, double* lds)
        : w(w_), wv(T == 1 ? 0 : wv_), tid((T == 1 ? 0 : wv_) * WAVE + w_.lane), li(w_.lane & 15), lk(w_.lane >> 4) {
        bA = lds; bG = bA + N * LD; bH = bG + N * LD; bX = bH + N * LD;
        sc = bX + N * LD; piv = sc + 4 * N; red = piv + N;
    }

    // f(r, c) for the entries of this thread of an elementwise pass: consecutive lanes take consecutive columns
    template <class F>
    MPCQP_HD void for_elems(F&& f) const {
#pragma unroll 4
        for (int idx = tid; idx < N * N; idx += NTHR) f(idx / N, idx % N);
    }
    // slot t of this wavefront holds a tile (a wave-uniform test, and none where T divides the tile count)
    MPCQP_HD static bool owns(int t, int ti) { return T * t + T <= NTILES || ti < NTILES; }
    // f(t, q, row, col) for the accumulator entries of this lane: tile ti = wv + T t, D[row = (lane >> 4) + 4 q][col = lane & 15]
    template <class F>
    MPCQP_HD void for_acc(F&& f) const {
        mhe::sfor<TPW>([&](auto it) {
            constexpr int t = decltype(it)::v;
            const int ti = wv + T * t;
            if (owns(t, ti)) {
                const int r0 = 16 * (ti / NTL) + lk, c0 = 16 * (ti % NTL) + li;
                mhe::sfor<4>([&](auto iq) { constexpr int q = decltype(iq)::v; f(it, iq, r0 + 4 * q, c0); });
            }
        });
    }
    MPCQP_HD void zero(Acc& acc) const {
        mhe::sfor<TPW>([&](auto it) { mhe::sfor<4>([&](auto iq) { acc[decltype(it)::v][decltype(iq)::v] = 0.0; }); });
    }
    MPCQP_HD void ld_acc(const double* M, Acc& acc) const {
        for_acc([&](auto it, auto iq, int r, int c) { acc[decltype(it)::v][decltype(iq)::v] = M[r * LD + c]; });
    }
    // M = acc.  FENCE: the destination was read by other threads since the last barrier (the product that made acc)
    template <bool FENCE>
    MPCQP_HD void put(double* M, const Acc& acc) const {
        if constexpr (FENCE) w.sync();
        for_acc([&](auto it, auto iq, int r, int c) { M[r * LD + c] = acc[decltype(it)::v][decltype(iq)::v]; });
        w.sync();
    }
    // acc += op(X) op(Y) on this wavefront's tiles; TA / TB: the operand is the transpose of what the buffer holds.
    // A[i = lane & 15][k = lane >> 4], B[k][j = lane & 15] per step of four k, as in Ops::mm_staged
    template <bool TA, bool TB>
    MPCQP_HD void mma(const double* X, const double* Y, Acc& acc) const {
        mhe::sfor<TPW>([&](auto it) {
            constexpr int t = decltype(it)::v;
            const int ti = wv + T * t;
            if (owns(t, ti)) {
                const int i0 = 16 * (ti / NTL), j0 = 16 * (ti % NTL);
#if defined(__HIP_DEVICE_COMPILE__)
                typedef double v4d_ __attribute__((ext_vector_type(4)));
                v4d_ c = {acc[t][0], acc[t][1], acc[t][2], acc[t][3]};
                const double* xa = TA ? X + lk * LD + i0 + li : X + (i0 + li) * LD + lk;
                const double* yb = TB ? Y + (j0 + li) * LD + lk : Y + lk * LD + j0 + li;
#pragma unroll 4
                for (int k0 = 0; k0 < N; k0 += 4)
                    c = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[TA ? k0 * LD : k0], yb[TB ? k0 : k0 * LD], c, 0, 0, 0);
                acc[t][0] = c[0]; acc[t][1] = c[1]; acc[t][2] = c[2]; acc[t][3] = c[3];
#else
                mhe::sfor<4>([&](auto iq) {
                    constexpr int q = decltype(iq)::v;
                    const int r = i0 + lk + 4 * q, cc = j0 + li;
                    double s = acc[t][q];
                    for (int k = 0; k < N; ++k) s = fma(TA ? X[k * LD + r] : X[r * LD + k], TB ? Y[cc * LD + k] : Y[k * LD + cc], s);
                    acc[t][q] = s;
                });
#endif
            }
        });
    }
    // M = ½ (M + M') in place: the thread of entry (r, c), c > r, writes both
    MPCQP_HD void symmetrise(double* M) const {
        for_elems([&](int r, int c) {
            if (c > r) {
                const double m = 0.5 * (M[r * LD + c] + M[c * LD + r]);
                M[r * LD + c] = m;
                M[c * LD + r] = m;
            }
        });
        w.sync();
    }
    // max over the workgroup of three values at once
    MPCQP_HD void wg_max3(double& x, double& y, double& z) const {
        red[tid] = x; red[NTHR + tid] = y; red[2 * NTHR + tid] = z;
        w.sync();
        for (int i = 0; i < NTHR; ++i) { x = fmax(x, red[i]); y = fmax(y, red[NTHR + i]); z = fmax(z, red[2 * NTHR + i]); }
        w.sync();
    }
    // In-place inverse of the symmetric positive definite M (visible to every thread: a barrier lies behind its last
    // write), then M = post(M, r, c) in the same pass.  false -- for the whole workgroup, M then holds nothing of use --:
    // a pivot is not in (0, inf).  pmin: the smallest of the first n pivots (those of the estimator's own block).
    template <class F>
    MPCQP_HD bool gj(double* M, int n, double& pmin, F&& post) const {
        // The NE entries of this thread stay in registers over the N steps; LDS carries the pivot rows and columns only.
        // A step first loads all it needs and then computes and stores: the compiler cannot tell the scratch it reads from
        // the scratch it writes, and a load behind a store would wait for it, entry after entry.
        double m[NE], pr[NE], pc[NE];
        int rr[NE], cc[NE];
        mhe::sfor<NE>([&](auto ie) {
            constexpr int e = decltype(ie)::v;
            const int idx = tid + e * NTHR;
            rr[e] = idx / N; cc[e] = idx % N;
            m[e] = M[rr[e] * LD + cc[e]];
        });
        mhe::sfor<NE>([&](auto ie) {
            constexpr int e = decltype(ie)::v;
            if (rr[e] == 0) sc[cc[e]] = m[e];
            if (cc[e] == 0) sc[N + rr[e]] = m[e];
        });
        w.sync();
        pmin = 1e300;
        for (int k = 0; k < N; ++k) {
            const double *prow = sc + (k & 1) * 2 * N, *pcol = prow + N;
            double *nrow = sc + ((k + 1) & 1) * 2 * N, *ncol = nrow + N;
            const double dk = prow[k];
            if (!((dk > 1e-280) && (dk < 1e280))) { w.sync(); return false; }
            if (k < n) pmin = fmin(pmin, dk);
            const double pinv = mhe::recip(dk);
            if (tid == 0) piv[k] = pinv;
            mhe::sfor<NE>([&](auto ie) { constexpr int e = decltype(ie)::v; pr[e] = prow[cc[e]]; pc[e] = pcol[rr[e]]; });
            mhe::sfor<NE>([&](auto ie) {
                constexpr int e = decltype(ie)::v;
                const int r = rr[e], c = cc[e];
                const double g = (r == k) ? 0.0 : -pc[e] * pinv;            // other rows: a[c] - a[k] a_k[c] / dk
                const double v = (c == k) ? ((r == k) ? 1.0 : g) : fma(pr[e], g, m[e]);
                m[e] = v;
                if (r == k + 1) nrow[c] = v;
                if (c == k + 1) ncol[r] = v;
            });
            w.sync();
        }
        mhe::sfor<NE>([&](auto ie) { constexpr int e = decltype(ie)::v; pr[e] = piv[rr[e]]; });
        mhe::sfor<NE>([&](auto ie) {
            constexpr int e = decltype(ie)::v;
            M[rr[e] * LD + cc[e]] = post(m[e] * pr[e], rr[e], cc[e]);
        });
        w.sync();
        return true;
    }
    MPCQP_HD bool gj(double* M, int n, double& pmin) const { return gj(M, n, pmin, [](double v, int, int) { return v; }); }

    // the n x n matrix p of the ABI (column-major) padded with `pad` on the diagonal; consecutive lanes read consecutive words
    MPCQP_HD void ld_sq(double* M, const double* p, int n, double pad) const {
        for_elems([&](int c, int r) { M[r * LD + c] = (r < n && c < n) ? p[c * n + r] : (r == c ? pad : 0.0); });
    }
    // Ĉm: row m = measured output m (row i_ym[m] of Ĉ), zeros in the padding
    MPCQP_HD void ld_cm(double* M, const DareArgs& a, const double* Cb) const {
        for_elems([&](int c, int m) { M[m * LD + c] = (m < a.nym && c < a.nx) ? Cb[a.i_ym[m] + a.ny * c] : 0.0; });
    }

    MPCQP_HD void solve(const DareArgs& a, int b) const {
        const int nx = a.nx, nym = a.nym;
        const double* Ab = a.Ahat + (size_t)b * nx * nx;
        const double* Cb = a.C + (size_t)b * a.ny * nx;
        const double* Qb = a.Q + (size_t)b * nx * nx;
        const double* Rb = a.R + (size_t)b * nym * nym;
        Acc acc, keep;
        double pmin;
        int st = DARE_BROKE_DOWN, it = 0;
        // ---- G(0) = Ĉm' R̂⁻¹ Ĉm
        ld_sq(bX, Rb, nym, 1.0);
        ld_cm(bH, a, Cb);
        w.sync();
        bool good = gj(bX, nym, pmin);                 // R̂⁻¹
        if (good) {
            zero(acc); mma<false, false>(bX, bH, acc); put<true>(bX, acc);          // R̂⁻¹ Ĉm
            zero(acc); mma<true, false>(bH, bX, acc); put<false>(bG, acc);          // Ĉm' (R̂⁻¹ Ĉm)
            symmetrise(bG);
            // ---- A(0) = Â', H(0) = Q̂ (identity in the padding), max diag Q̂
            for_elems([&](int r, int c) { bA[r * LD + c] = (r < nx && c < nx) ? Ab[r * nx + c] : 0.0; });
            ld_sq(bH, Qb, nx, 1.0);
            double qd = 0.0, u0 = 0.0, u1 = 0.0;
            for (int i = tid; i < nx; i += NTHR) qd = fmax(qd, Qb[i * nx + i]);
            wg_max3(qd, u0, u1);                       // (its barriers also stand between the loads and their readers)
            st = DARE_NOT_CONVERGED;
            for (int k = 0; k < DARE_MAX_ITER; ++k) {
                it = k + 1;
                // S = (H⁻¹ + G)⁻¹                                                           -> bX
                for_elems([&](int r, int c) { bX[r * LD + c] = bH[r * LD + c]; });
                w.sync();
                bool ok = gj(bX, nx, pmin, [&](double v, int r, int c) { return v + bG[r * LD + c]; });
                // (k = 0: these were the pivots of Q̂ -- a numerically singular one is not for this form)
                if (ok && k == 0 && !(pmin > DARE_PSD_SING * qd)) ok = false;
                ok = ok && gj(bX, nx, pmin);
                if (!ok) { st = DARE_BROKE_DOWN; break; }
                symmetrise(bX);
                // H(k+1) = H + A' S A                                                       -> bH, H(k) in `keep`
                zero(acc); mma<false, false>(bX, bA, acc);
                ld_acc(bH, keep);
                put<false>(bH, acc);                   // (bH: read by this lane alone, at the entries it writes)
                ld_acc_from(keep, acc); mma<true, false>(bA, bH, acc); put<true>(bH, acc);
                symmetrise(bH);
                double bad = 0.0, dmax = 0.0, hmax = 0.0;
                for_acc([&](auto it_, auto iq, int r, int c) {
                    const double h = bH[r * LD + c];
                    bad = (h - h == 0.0) ? bad : 1.0;
                    dmax = fmax(dmax, fabs(h - keep[decltype(it_)::v][decltype(iq)::v]));
                    hmax = fmax(hmax, fabs(h));
                });
                // T = G S -> bX,   G - G S G -> bG, G(k) in `keep`
                zero(acc); mma<false, false>(bG, bX, acc); put<true>(bX, acc);
                zero(acc); mma<false, false>(bX, bG, acc);
                ld_acc(bG, keep);
                for_acc([&](auto it_, auto iq, int, int) {
                    constexpr int t = decltype(it_)::v, q = decltype(iq)::v;
                    acc[t][q] = keep[t][q] - acc[t][q];
                });
                put<true>(bG, acc);
                // G(k+1) = G + A (G - G S G) A'                                             -> bG
                zero(acc); mma<false, false>(bA, bG, acc); put<true>(bG, acc);
                ld_acc_from(keep, acc); mma<false, true>(bG, bA, acc);
                for_acc([&](auto it_, auto iq, int, int) {
                    const double g = acc[decltype(it_)::v][decltype(iq)::v];
                    bad = (g - g == 0.0) ? bad : 1.0;
                });
                put<true>(bG, acc);
                symmetrise(bG);
                // A(k+1) = A W A = (A - A T) A                                              -> bA
                zero(acc); mma<false, false>(bA, bX, acc);
                for_acc([&](auto it_, auto iq, int r, int c) {
                    constexpr int t = decltype(it_)::v, q = decltype(iq)::v;
                    acc[t][q] = bA[r * LD + c] - acc[t][q];
                });
                put<true>(bX, acc);
                zero(acc); mma<false, false>(bX, bA, acc);
                for_acc([&](auto it_, auto iq, int, int) {
                    const double v = acc[decltype(it_)::v][decltype(iq)::v];
                    bad = (v - v == 0.0) ? bad : 1.0;
                });
                put<true>(bA, acc);
                // this estimator's test: finite, and how far H moved
                wg_max3(bad, dmax, hmax);
                if (bad > 0.5) { st = DARE_BROKE_DOWN; break; }
                if (dmax <= DARE_TOL * fmax(1.0, hmax)) { st = DARE_OK; break; }
            }
        }
        if (st == DARE_OK) {
            // ---- K̂ = P̂∞ Ĉm' (Ĉm P̂∞ Ĉm' + R̂)⁻¹ in the order of kf_gain (kf_cov_bodies.h); P̂∞ = bH
            ld_cm(bA, a, Cb);
            ld_sq(bX, Rb, nym, 1.0);
            w.sync();
            zero(acc); mma<false, true>(bH, bA, acc); put<false>(bG, acc);          // P̂ Ĉm'
            ld_acc(bX, acc); mma<false, false>(bA, bG, acc); put<false>(bX, acc);   // M̂ = R̂ + Ĉm (P̂ Ĉm')
            const bool okg = gj(bX, nym, pmin);                                     // M̂⁻¹
            double bad = 0.0, u0 = 0.0, u1 = 0.0;
            if (okg) {
                zero(acc); mma<false, false>(bG, bX, acc);                          // K̂ = (P̂ Ĉm') M̂⁻¹
                for_acc([&](auto it_, auto iq, int, int) {
                    const double v = acc[decltype(it_)::v][decltype(iq)::v];
                    bad = (v - v == 0.0) ? bad : 1.0;
                });
            }
            wg_max3(bad, u0, u1);
            if (okg && !(bad > 0.5)) {
                double* Pb = a.P + (size_t)b * nx * nx;
                double* Kb = a.K + (size_t)b * nym * nx;
                for_acc([&](auto it_, auto iq, int r, int c) {
                    if (r < nx && c < nym) Kb[c * nx + r] = acc[decltype(it_)::v][decltype(iq)::v];
                });
                for_elems([&](int c, int r) { if (r < nx && c < nx) Pb[c * nx + r] = bH[r * LD + c]; });
            } else {
                st = DARE_BROKE_DOWN;
            }
        }
        if (tid == 0) {
            a.status[b] = st;
            a.iters[b] = it;
        }
        w.sync();                                      // the next estimator's loads write what this one may still read
    }
    MPCQP_HD void ld_acc_from(const Acc& src, Acc& acc) const {
        mhe::sfor<TPW>([&](auto it) { mhe::sfor<4>([&](auto iq) { acc[decltype(it)::v][decltype(iq)::v] = src[decltype(it)::v][decltype(iq)::v]; }); });
    }
};

// one workgroup: the estimators wg, wg + a.nwaves, ... (a.nwaves: workgroups of the persistent grid)
template <class W, int N, int T>
MPCQP_HD void kf_dare_lds_body(W& w, const DareArgs& a, int wg, int wv, double* lds) {
    const DareLds<W, N, T> op(w, wv, lds);
    for (int b = wg; b < a.B; b += a.nwaves) op.solve(a, b);
}

}  // namespace kf
}  // namespace mpcqp
