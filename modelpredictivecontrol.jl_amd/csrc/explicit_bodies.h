// explicit_bodies.h -- the ExplicitMPC of the batch (src/controller/explicitmpc.jl): the unconstrained LinMPC with H~ factored
// once per model and Z~ = -H~^-1 q~ applied every period (explicitmpc.jl:216).  Written against the wave interface of
// mpcqp_bodies.h (lane, sync, bcast, any: DevWave on gfx950, EmuWave in tests/emu/emu_explicit.cpp).
//
//   explicit_factor_body  once per model: Cholesky of H~ (Model::Hpk) in LDS, one row per lane, then H~^-1 = L^-T L^-1, the
//                         sums of the input weights per move.  A pivot that is not in (0, inf), or an inverse that is not
//                         finite, fails THAT controller: status EX_FAILED, zero tables (where the reference's cholesky throws).
//   explicit_step_body    one period, one wavefront per controller: F = B + K x0 + V lastu0 (+ G d0 + J D^0), q~ =
//                         2[(M E)'(F - R^y) + (L Pu)'(Tu lastu0 - R^u)] (initpred!, execute.jl:247-277) with diagonal, block
//                         and dense weights, then Z~ = -H~^-1 q~ as a product with the stored inverse (a.Hinv: its packed lower
//                         triangle, staged in LDS), u0 and the optional Y^0 = E Z~ + F.  No factorisation, no interior-point
//                         code.
//   explicit_law_body     with inputs held over the horizon the period is affine in [x0; lastu0; ry; d0]: one lane per row of
//                         Z~ (or of u0) of the WHOLE batch, 64 consecutive rows per wavefront, the table read in 16-byte
//                         pairs (explicit_launch.h: law_index).  Pure bandwidth.
// A controller whose factorisation failed gets status 2, Z~ = 0 and u0 = lastu0 from both per-period bodies; its
// neighbours never see it (no cross-controller operation anywhere).
#pragma once
#include <math.h>

#include "explicit_launch.h"

namespace mpcqp {
namespace ex {

template <class W>
MPCQP_HD void explicit_factor_body(W& w, const FactorArgs& a, int b, double* sm) {
    const int n = a.n, i = w.lane;
    double* A = sm;                    // [n][n] row-major: lane i owns row i
    double* X = sm + (size_t)n * n;    // L^-1, row-major; lane c computes column c
    const double* Hp_ = a.Hpk + (size_t)b * a.npk;
    if (i < n)
        for (int j = 0; j <= i; ++j) A[i * n + j] = Hp_[pk(i, j)];
    w.sync();
    bool ok = true;
    for (int k = 0; k < n; ++k) {
        const double dk = A[k * n + k];                   // (every lane reads the same word)
        if (!(dk > 0.0 && dk - dk == 0.0)) { ok = false; break; }      // wave-uniform
        const double r = sqrt(dk), ri = 1.0 / r;
        w.sync();
        double lik = 0.0;
        if (i > k && i < n) { lik = A[i * n + k] * ri; A[i * n + k] = lik; }
        if (i == k) A[k * n + k] = r;
        w.sync();
        if (i > k && i < n)
            for (int j = k + 1; j <= i; ++j) A[i * n + j] -= lik * A[j * n + k];
        w.sync();
    }
    bool fin = true;
    if (ok) {
        // column c of X = L^-1 by forward substitution (L[r][k]: one word for the whole wavefront)
        if (i < n) {
            const int c = i;
            for (int r = 0; r < c; ++r) X[r * n + c] = 0.0;
            X[c * n + c] = 1.0 / A[c * n + c];
            for (int r = c + 1; r < n; ++r) {
                double s = 0.0;
                for (int k = c; k < r; ++k) s += A[r * n + k] * X[k * n + c];
                X[r * n + c] = -s / A[r * n + r];
            }
        }
        w.sync();
        // row i of the lower triangle of H~^-1 = X'X
        if (i < n) {
            double* Hi = a.Hinv + (size_t)b * tri(n) + tri(i);
            for (int j = 0; j <= i; ++j) {
                double s = 0.0;
                for (int k = i; k < n; ++k) s += X[k * n + i] * X[k * n + j];
                fin = fin && (s - s == 0.0);
                Hi[j] = s;
            }
        }
    }
    ok = ok && !w.any(!fin);
    if (i < n) {
        double* Hi = a.Hinv + (size_t)b * tri(n) + tri(i);
        if (!ok)
            for (int j = 0; j <= i; ++j) Hi[j] = 0.0;
        // sum of the diagonal input weights from the first step of this lane's move on
        const int j = i / a.nu, c = i - j * a.nu;
        const double* Ld = a.Ldiag + (size_t)b * a.Hp * a.nu + c;
        double ls = 0.0;
        for (int t = a.jl[j]; t < a.Hp; ++t) ls += Ld[t * a.nu];
        a.Lsum[(size_t)b * n + i] = ls;
    }
    if (i == 0) a.status[b] = ok ? EX_OK : EX_FAILED;
}

template <class W>
MPCQP_HD void explicit_step_body(W& w, const StepArgs& a, int b, double* sm) {
    const Dims& d = a.d;
    const Model& m = a.m;
    const int nx = d.nxh, nu = d.nu, ny = d.ny, nd = d.nd, nY = d.nY, nU = d.nU, Hp = d.Hp, n = d.nDU;
    const int lane = w.lane;
    double* F = sm;                    // [nY]
    double* T = F + nY;                // [max(nY, 64)] M (F - R^y)
    double* zs = T;                    // [64] exchange buffer, once q~ has T
    double* S = T + (nY > WAVE ? nY : WAVE); // [Hp][ny][nu] step-response table
    double* Hs = S + (size_t)Hp * ny * nu;   // [tri(n)] packed lower triangle of H~^-1
    const double* x0 = a.xhat0 + (size_t)b * nx;
    const double* lu = a.lastu0 + (size_t)b * nu;
    const double* K = m.Ktab + (size_t)b * nx * nY;
    const double* Sg = m.Stab + (size_t)b * Hp * ny * nu;
    const bool rconst = d.flags & 1u;
    const double* Ry = a.Ry + (size_t)b * (rconst ? ny : nY);
    const double* Ru = a.Ru ? a.Ru + (size_t)b * nU : nullptr;
    const bool good = a.fstatus[b] == EX_OK;
    const bool diagM = !m.Mfull && !m.Mblk;
    // global -> LDS in batches of eight loads per lane (the loads of a batch are in flight together; a slot behind the end re-reads the last word)
    auto stage = [&](double* dst, const double* src, int len) {
        for (int r0 = lane; r0 < len; r0 += 8 * WAVE) {
            double v[8];
            MPCQP_UNROLL
            for (int u = 0; u < 8; ++u) { const int r = r0 + u * WAVE; v[u] = src[r < len ? r : len - 1]; }
            MPCQP_UNROLL
            for (int u = 0; u < 8; ++u) { const int r = r0 + u * WAVE; if (r < len) dst[r] = v[u]; }
        }
    };
    stage(Hs, a.Hinv + (size_t)b * tri(n), tri(n));
    stage(S, Sg, Hp * ny * nu);
    // F = B + K x0 + V lastu0 (+ G d0 + J D^0)                execute.jl:249-255; V block t = Sigma_t.  B = 0 without f^op - x^op
    for (int r = lane; r < nY; r += WAVE) {
        const int t = r / ny, a_ = r - t * ny;
        double acc = m.dop ? m.Bvec[(size_t)b * nY + r] : 0.0;
        const double md = diagM ? m.Mdiag[(size_t)b * nY + r] : 0.0;
        const double ryr = rconst ? Ry[a_] : Ry[r];
        int k = 0;
        for (; k + 8 <= nx; k += 8) {
            double kv[8];
            MPCQP_UNROLL
            for (int u = 0; u < 8; ++u) kv[u] = K[(size_t)(k + u) * nY + r];
            MPCQP_UNROLL
            for (int u = 0; u < 8; ++u) acc += kv[u] * x0[k + u];
        }
        for (; k < nx; ++k) acc += K[(size_t)k * nY + r] * x0[k];
        for (int c = 0; c < nu; ++c) acc += Sg[(t * ny + a_) * nu + c] * lu[c];
        if (nd > 0) {
            const double* Gd = m.Gdtab + (size_t)b * Hp * ny * nd;
            const double* dd0 = a.d0 + (size_t)b * nd;
            const double* Dh = a.Dhat0 + (size_t)b * d.nD;
            const double* Dd = m.Dd + (size_t)b * ny * nd;      // (ny,nd) column-major
            for (int e = 0; e < nd; ++e) {
                acc += Gd[(t * ny + a_) * nd + e] * dd0[e];     // G block t = C A^t Bd
                acc += Dd[a_ + ny * e] * Dh[t * nd + e];        // J diagonal block = Dd
                for (int j = 0; j < t; ++j) acc += Gd[((t - j - 1) * ny + a_) * nd + e] * Dh[j * nd + e];   // J[t, j] = G block t-j-1
            }
        }
        F[r] = acc;
        if (diagM) T[r] = md * (acc - ryr);         // T = M (F - R^y), diagonal M_Hp: the lane's own entry
        if (a.F_keep) a.F_keep[(size_t)b * nY + r] = acc;
    }
    w.sync();
    // T = M (F - R^y): dense or block-diagonal M_Hp, in the precedence of the step kernels
    auto cy = [&](int r) { return F[r] - (rconst ? Ry[r % ny] : Ry[r]); };
    if (m.Mfull) {
        const double* Mf = m.Mfull + (size_t)b * nY * nY;
        for (int r = lane; r < nY; r += WAVE) {
            double acc = 0.0;
            for (int r2 = 0; r2 < nY; ++r2) acc += Mf[r + (size_t)nY * r2] * cy(r2);
            T[r] = acc;
        }
        w.sync();
    } else if (m.Mblk) {
        const double* Mb = m.Mblk + (size_t)b * Hp * ny * ny;
        for (int r = lane; r < nY; r += WAVE) {
            const int t = r / ny, a_ = r - t * ny;
            double acc = 0.0;
            for (int a2 = 0; a2 < ny; ++a2) acc += Mb[((size_t)t * ny + a2) * ny + a_] * cy(t * ny + a2);
            T[r] = acc;
        }
        w.sync();
    }
    // q~[k] = 2 [E'T + Pu'L Cu][k], k = (move j, channel c): E block (t, j) = Sigma_{t - j_j} for t >= j_j
    const int j = lane < n ? lane / nu : 0, c = lane < n ? lane - j * nu : 0;
    const int t0 = m.jl[j];
    double q = 0.0;
    if (lane < n) {
        const double* Sc = S + c;
        const double* Tt = T + (size_t)t0 * ny;
        const int len = (Hp - t0) * ny;
        double q0 = 0.0, q1 = 0.0;
        int r = 0;
        MPCQP_UNROLL4
        for (; r + 1 < len; r += 2) { q0 += Sc[r * nu] * Tt[r]; q1 += Sc[(r + 1) * nu] * Tt[r + 1]; }
        if (r < len) q0 += Sc[r * nu] * Tt[r];
        q = q0 + q1;
    }
    if (m.Ldense) {        // dense L_Hp: the rows of L Cu, Cu = Tu lastu0 - R^u, 64 at a time through zs; each lane adds its own
        const double* Lf = m.Ldense + (size_t)b * nU * nU;
        for (int r0 = 0; r0 < nU; r0 += WAVE) {
            const int r = r0 + lane;
            double acc = 0.0;
            if (r < nU)
                for (int r2 = 0; r2 < nU; ++r2) acc += Lf[r + (size_t)nU * r2] * (lu[r2 % nu] - (Ru ? Ru[r2] : 0.0));
            w.sync();
            zs[lane] = acc;
            w.sync();
            if (lane < n)
                for (int k = 0; k < WAVE && r0 + k < nU; ++k)
                    if ((r0 + k) % nu == c && (r0 + k) / nu >= t0) q += zs[k];
        }
    } else if (lane < n) {
        if (!Ru) {         // R^u = 0: sum_t L[t, c] lastu0[c], the sum kept by k_explicit_factor
            q += a.Lsum[(size_t)b * n + lane] * lu[c];
        } else {
            const double* Ld = m.Ldiag + (size_t)b * nU + c;
            const double luc = lu[c];
            double acc = 0.0;
            for (int t = t0; t < Hp; ++t) acc += Ld[t * nu] * (luc - Ru[t * nu + c]);
            q += acc;
        }
    }
    q *= 2.0;
    if (a.q_keep && lane < n) a.q_keep[(size_t)b * n + lane] = q;
    // Z~ = -H~^-1 q~
    // row `lane` of the symmetric matrix out of its packed lower triangle: (i, k) at tri(max) + min
    const int i = lane < n ? lane : 0, ti = tri(i);
    double z0 = 0.0, z1 = 0.0;
    int k = 0;
    MPCQP_UNROLL4
    for (; k + 1 < n; k += 2) {
        z0 += Hs[k <= i ? ti + k : tri(k) + i] * w.bcast(q, k);
        z1 += Hs[k + 1 <= i ? ti + k + 1 : tri(k + 1) + i] * w.bcast(q, k + 1);
    }
    if (k < n) z0 += Hs[k <= i ? ti + k : tri(k) + i] * w.bcast(q, k);
    double z = -(z0 + z1);
    if (!good || lane >= n) z = 0.0;
    if (lane < n) a.Z[(size_t)b * n + lane] = z;
    if (lane < nu) a.u0[(size_t)b * nu + lane] = z + lu[lane];       // getinput!, execute.jl:536-546
    if (lane == 0) a.status[b] = good ? EX_OK : EX_FAILED;
    if (a.Yhat0) {          // predict!, transcription.jl:1136-1145: Y^0 = E Z~ + F
        w.sync();
        zs[lane] = z;
        w.sync();
        for (int r = lane; r < nY; r += WAVE) {
            const int t = r / ny, a_ = r - t * ny;
            double acc = F[r];
            for (int jj = 0; jj < d.Hc && m.jl[jj] <= t; ++jj) {
                const double* Sb = S + ((size_t)(t - m.jl[jj]) * ny + a_) * nu;
                for (int cc = 0; cc < nu; ++cc) acc += Sb[cc] * zs[jj * nu + cc];
            }
            a.Yhat0[(size_t)b * nY + r] = acc;
        }
    }
}

// input k of the law of controller b: [1; x0; lastu0; ry; d0] (k is wave-uniform)
MPCQP_HD inline double law_input(const LawArgs& a, size_t b, int k) {
    if (k == 0) return 1.0;
    k -= 1;
    if (k < a.nx) return a.xhat0[b * a.nx + k];
    k -= a.nx;
    if (k < a.nu) return a.lastu0[b * a.nu + k];
    k -= a.nu;
    if (k < a.ny) return a.ry[b * a.ny + k];
    k -= a.ny;
    if (k < a.nd) return a.d0[b * a.nd + k];
    return 0.0;            // the padding column of an odd table
}

template <class W>
MPCQP_HD void explicit_law_body(W& w, const LawArgs& a, int wave_id) {
    const size_t total = (size_t)a.B * a.rows;
    const size_t groups = (total + WAVE - 1) / WAVE;
    for (size_t g = wave_id; g < groups; g += a.nwaves) {
        const size_t R = g * WAVE + w.lane;
        const bool live = R < total;
        const size_t b = (live ? R : total - 1) / a.rows;
        const int i = (int)((live ? R : total - 1) - b * a.rows);
        const double* tp = a.table + (g * a.kp) * (2 * WAVE) + (size_t)w.lane * 2;
        double z0 = 0.0, z1 = 0.0;
        for (int p = 0; p < a.kp; ++p) {
#if defined(__HIP_DEVICE_COMPILE__)
            const double2 tv = *reinterpret_cast<const double2*>(tp + (size_t)p * 2 * WAVE);
            const double t0 = tv.x, t1 = tv.y;
#else
            const double t0 = tp[(size_t)p * 2 * WAVE], t1 = tp[(size_t)p * 2 * WAVE + 1];
#endif
            z0 += t0 * law_input(a, b, 2 * p);
            z1 += t1 * law_input(a, b, 2 * p + 1);
        }
        const double z = z0 + z1;
        if (live) {
            if (a.Z) a.Z[R] = z;
            if (i < a.nu) a.u0[b * a.nu + i] = z + a.lastu0[b * a.nu + i];
            if (i == 0) a.status[b] = a.fstatus[b];
        }
    }
}

// one thread per (controller, input word): the unit input of column k (k >= 1; column 0 is the all-zero input).  A disturbance
// column sets d0 and the whole preview, D^ = repeat(d0) -- the reference's default call moveinput!(mpc, ry, d)
MPCQP_HD inline void explicit_law_unit_at(const LawBuildArgs& a, size_t b, int t) {
    int k = a.k - 1;
    if (k < 0) return;
    if (k < a.nx) { if (t == 0) a.xhat0[b * a.nx + k] = 1.0; return; }
    k -= a.nx;
    if (k < a.nu) { if (t == 0) a.lastu0[b * a.nu + k] = 1.0; return; }
    k -= a.nu;
    if (k < a.ny) { if (t == 0) a.ry[b * a.ny + k] = 1.0; return; }
    k -= a.ny;
    if (k < a.nd) {
        if (t == 0) a.d0[b * a.nd + k] = 1.0;
        if (t < a.Hp) a.Dhat0[(b * a.Hp + t) * a.nd + k] = 1.0;
    }
}
// one thread per row R = b * n + i of the batch: column k of both tables
MPCQP_HD inline void explicit_law_pack_at(const LawBuildArgs& a, size_t R) {
    const double v = a.k == 0 ? a.Z0[R] : a.Zk[R] - a.Z0[R];
    a.table_z[law_index(R, a.k, a.kp)] = v;
    const size_t b = R / a.n, i = R - b * a.n;
    if (i < (size_t)a.nu) a.table_u[law_index(b * a.nu + i, a.k, a.kp)] = v;
}

}  // namespace ex
}  // namespace mpcqp
