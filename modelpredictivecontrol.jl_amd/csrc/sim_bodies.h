// sim_bodies.h -- the plant of the closed-loop simulation (include/mpcqp.h: mpcqp_sim; src/plot_sim.jl:253-319), written
// against the wave interface of the other bodies (lane, sync): k_sim_plant on the device, tests/emu/emu_sim.cpp on the CPU.
// sim_launch.h says what a launch does.  Every sum runs over its columns in ascending order, in the lane that owns the row,
// and reads nothing of another controller: a member's result does not depend on the batch around it.
#pragma once
#include "mpcqp_types.h"
#include "sim_launch.h"

namespace mpcqp {
namespace sim {

// v + step + σ w, each term only when its array is given (a σ of 0 with a NaN draw still gives NaN: the draw is read)
MPCQP_HD double disturbed(double v, const double* step, const double* sig, const double* w, size_t k, size_t kw) {
    if (step) v += step[k];
    if (sig) v += sig[k] * w[kw];
    return v;
}

template <class W>
MPCQP_HD void sim_plant_body(W& w, const PlantArgs& a, int wave, double* sm) {
    const int G = a.G, g = w.lane / G, r = w.lane % G, base = g * G;
    const size_t b = (size_t)wave * (size_t)(WAVE / G) + (size_t)g;
    const bool on = b < (size_t)a.B;
    const int nxp = a.nxp, nu = a.nu, ny = a.ny, nd = a.nd, N = a.N;
    double *xs = sm, *us = sm + WAVE, *ds = sm + 2 * WAVE, *ys = sm + 3 * WAVE;

    if (a.i_est >= 0) {          // X̂(k|k) and Ŷ = Ĉ x̂0 + D̂d d0
        const size_t i = (size_t)a.i_est;
        if (on) {
            const double* xh = a.xhat + b * a.nxh;
            if (a.Xhat)
                for (int k = r; k < a.nxh; k += G) a.Xhat[(b * N + i) * a.nxh + k] = xh[k];
            if (a.Yhat && r < ny) {
                double y = 0.0;
                for (int j = 0; j < a.nxh; ++j) y += a.Chat[(b * a.nxh + j) * ny + r] * xh[j];
                if (a.Dhd)
                    for (int j = 0; j < nd; ++j) y += a.Dhd[(b * nd + j) * ny + r] * a.d0[b * nd + j];
                if (a.yhs) y += a.yhs[b * ny + r];
                a.Yhat[(b * N + i) * ny + r] = y;
            }
        }
        return;
    }

    if (a.i_tail >= 0) {
        const size_t i = (size_t)a.i_tail;
        if (on) {
            if (r < nu) {
                const double u = a.u0[b * nu + r];
                const double ud = disturbed(u, a.u_step, a.su, a.wu, b * nu + r, (b * N + i) * nu + r);
                a.lastu0[b * nu + r] = u;
                if (a.U) a.U[(b * N + i) * nu + r] = u;
                if (a.Ud) a.Ud[(b * N + i) * nu + r] = ud;
                us[base + r] = ud;
            }
            if (r < nd) ds[base + r] = a.d0[b * nd + r];
            if (r < nxp) xs[base + r] = a.x[b * nxp + r];
            if (r == 0 && a.status) a.status[b * N + i] = a.st ? a.st[b] : 0;
        }
        w.sync();
        double xn = 0.0;
        if (on && r < nxp) {
            for (int j = 0; j < nxp; ++j) xn += a.A[(b * nxp + j) * nxp + r] * xs[base + j];
            for (int j = 0; j < nu; ++j) xn += a.Bu[(b * nu + j) * nxp + r] * us[base + j];
            if (a.Bd)
                for (int j = 0; j < nd; ++j) xn += a.Bd[(b * nd + j) * nxp + r] * ds[base + j];
            if (a.fx) xn += a.fx[b * nxp + r];
            xn = disturbed(xn, nullptr, a.sx, a.wx, b * nxp + r, (b * N + i) * nxp + r);
        }
        w.sync();                // every lane has read the old state
        if (on && r < nxp) a.x[b * nxp + r] = xn;
    }

    if (a.i_head >= 0) {
        const size_t i = (size_t)a.i_head;
        if (on) {
            if (r < nd) {
                const double dv = disturbed(a.d[b * nd + r], a.d_step, a.sd, a.wd, b * nd + r, (b * N + i) * nd + r);
                a.d0[b * nd + r] = dv;
                ds[base + r] = dv;
                if (a.D) a.D[(b * N + i) * nd + r] = dv;
                if (a.Dhat0)
                    for (int t = 0; t < a.Hp; ++t) a.Dhat0[(b * a.Hp + t) * nd + r] = dv;
            }
            if (r < nxp) {       // (the lane's own store of the tail, or the caller's state)
                const double xv = a.x[b * nxp + r];
                xs[base + r] = xv;
                if (a.X) a.X[(b * N + i) * nxp + r] = xv;
            }
            if (r < ny && a.ry_cur) a.ry_cur[b * ny + r] = a.ry_per_period ? a.ry[(b * N + i) * ny + r] : a.ry[b * ny + r];
        }
        w.sync();
        if (on && r < ny) {
            double y = 0.0;
            for (int j = 0; j < nxp; ++j) y += a.C[(b * nxp + j) * ny + r] * xs[base + j];
            if (a.Dd)
                for (int j = 0; j < nd; ++j) y += a.Dd[(b * nd + j) * ny + r] * ds[base + j];
            y = disturbed(y, a.y_step, a.sy, a.wy, b * ny + r, (b * N + i) * ny + r);
            if (a.Y) a.Y[(b * N + i) * ny + r] = y;
            ys[base + r] = y;
        }
        w.sync();
        if (on && r < a.nym) a.y0m[b * a.nym + r] = ys[base + a.i_ym[r]];
    }
}

}  // namespace sim
}  // namespace mpcqp

// ---- the fused loop of an explicit-law handle (sim_launch.h: FusedArgs) -------------------------------------------------------
#include <utility>

#include "explicit_launch.h"

namespace mpcqp {
namespace sim {

// One table of a controller in LDS: R rows, its columns padded with zeros to a multiple of four; element (r, j) at
// off_t + (j * 4 + g) * R + r.  `off` is the lane's own offset (a lane beyond the last row reads the last row: what it computes
// is never used), `stride` = 4 R.
struct FusedTab {
    int off, stride;
};
MPCQP_HD int fused_pad4(int n) { return (n + 3) & ~3; }

// acc + sum_{j < n} T[r][j] v_j, v spread over the lanes of the row (zero beyond its length): four columns per block, the
// broadcast is the DPP modifier of the multiply-add (fmabc4); ascending j
template <int J0, class W>
MPCQP_HD void fused_mv_block(W& w, const double* sm, const FusedTab& t, double v, double& acc) {
    const double* q = sm + t.off + J0 * t.stride;
    w.template fmabc4<J0, J0 + 1, J0 + 2, J0 + 3>(acc, v, v, v, v, q[0], q[t.stride], q[2 * t.stride], q[3 * t.stride]);
}
template <class W>
MPCQP_HD double fused_mv(W& w, const double* sm, const FusedTab& t, double v, int n, double acc) {
    if (n > 0) fused_mv_block<0>(w, sm, t, v, acc);      // (n is wave-uniform)
    if (n > 4) fused_mv_block<4>(w, sm, t, v, acc);
    if (n > 8) fused_mv_block<8>(w, sm, t, v, acc);
    if (n > 12) fused_mv_block<12>(w, sm, t, v, acc);
    return acc;
}
template <int J, class W>
MPCQP_HD double fused_pick_step(W& w, double v, int sel, double cur) {
    const double b = w.template rowbc<J>(v);
    return sel == J ? b : cur;
}
template <class W, int... J>
MPCQP_HD double fused_pick(W& w, double v, int sel, std::integer_sequence<int, J...>) {       // v of lane `sel` of the row
    double cur = 0.0;
    ((cur = fused_pick_step<J>(w, v, sel, cur)), ...);
    return cur;
}

template <class W>
MPCQP_HD void sim_explicit_body(W& w, const FusedArgs& a, int wave, double* sm) {
    const PlantArgs& p = a.p;
    const int g = w.lane / FUSED_RL, r = w.lane % FUSED_RL;
    const size_t b = (size_t)wave * 4 + (size_t)g;
    const bool on = b < (size_t)p.B;
    const size_t bb = on ? b : (size_t)p.B - 1;          // a lane of an empty row computes on the last member and stores nothing
    const int nxh = p.nxh, nxp = p.nxp, nu = p.nu, ny = p.ny, nd = p.nd, nym = p.nym, N = p.N;
    const int iym = r < nym ? p.i_ym[r] : -1;
    // -- tables, once: column-major sources, row r in lane r -----------------------------------------------------------------
    int next = 0;
    auto tab = [&](int R, int ncols) {
        FusedTab t{next + g * R + (r < R ? r : R - 1), 4 * R};
        next += 4 * R * fused_pad4(ncols);
        return t;
    };
    // src[(bb * ncols + j) * ld + row], or the law's column k0 + j of row `row` when ld < 0
    auto fill = [&](const FusedTab& t, int ncols, const double* src, int ld, int row, int k0 = 0) {
        if (r * 4 < t.stride)
            for (int j = 0; j < fused_pad4(ncols); ++j)
                sm[t.off + j * t.stride] = (j < ncols && src) ? (ld < 0 ? src[ex::law_index(bb * nu + row, k0 + j, a.kp)] : src[(bb * ncols + j) * ld + row]) : 0.0;
    };
    const FusedTab Cm = tab(nym, nxh), Cmd = tab(nym, nd), K = tab(nxh, nym), Ch = tab(ny, nxh), Chd = tab(ny, nd), Ah = tab(nxh, nxh),
                   Bh = tab(nxh, nu), Bdh = tab(nxh, nd), A = tab(nxp, nxp), Bu = tab(nxp, nu), Bd = tab(nxp, nd), C = tab(ny, nxp),
                   Dd = tab(ny, nd), L0 = tab(nu, 1), Lx = tab(nu, nxh), Lu = tab(nu, nu), Lr = tab(nu, ny), Ld = tab(nu, nd);
    fill(Cm, nxh, p.Chat, ny, iym); fill(Cmd, nd, p.Dhd, ny, iym); fill(K, nym, a.Khat, nxh, r);
    fill(Ch, nxh, p.Chat, ny, r); fill(Chd, nd, p.Dhd, ny, r);
    fill(Ah, nxh, a.Ahat, nxh, r); fill(Bh, nu, a.Bhu, nxh, r); fill(Bdh, nd, a.Bhd, nxh, r);
    fill(A, nxp, p.A, nxp, r); fill(Bu, nu, p.Bu, nxp, r); fill(Bd, nd, p.Bd, nxp, r);
    fill(C, nxp, p.C, ny, r); fill(Dd, nd, p.Dd, ny, r);
    fill(L0, 1, a.law, -1, r, 0); fill(Lx, nxh, a.law, -1, r, 1); fill(Lu, nu, a.law, -1, r, 1 + nxh);
    fill(Lr, ny, a.law, -1, r, 1 + nxh + nu); fill(Ld, nd, a.law, -1, r, 1 + nxh + nu + ny);
    // -- the lane's entries of the vectors -----------------------------------------------------------------------------------
    double x = r < nxp ? p.x[bb * nxp + r] : 0.0, xh = r < nxh ? p.xhat[bb * nxh + r] : 0.0, lu = r < nu ? p.lastu0[bb * nu + r] : 0.0;
    const double ry = r < ny ? p.ry[bb * ny + r] : 0.0, dbase = r < nd ? p.d[bb * nd + r] : 0.0;
    const double fx = (r < nxp && p.fx) ? p.fx[bb * nxp + r] : 0.0, dop = (r < nxh && a.dop) ? a.dop[bb * nxh + r] : 0.0;
    const int fst = a.fstatus[bb];
    const auto seq = std::make_integer_sequence<int, FUSED_RL>{};
    // correction of x̂ with the measurement ym of this period: skipped for a member with a NaN in ym
    auto correct = [&](double ym, double d0) {
        double v = ym;
        v = -fused_mv(w, sm, Cm, xh, nxh, -v);
        v = -fused_mv(w, sm, Cmd, d0, nd, -v);
        if (r >= nym) v = 0.0;
        const double miss = w.rsum((r < nym && ym != ym) ? 1.0 : 0.0);
        const double xc = fused_mv(w, sm, K, v, nym, xh);
        if (miss == 0.0 && r < nxh) xh = xc;
    };
    for (int i = 0; i < N; ++i) {
        // the tables stay in LDS: without this the compiler hoists every table load out of the loop, 356 VGPRs and one
        // wavefront per SIMD
        asm volatile("" ::: "memory");
        const size_t bi = bb * N + (size_t)i;
        const double d0 = r < nd ? disturbed(dbase, p.d_step, p.sd, p.wd, bb * nd + r, bi * nd + r) : 0.0;
        double y = fused_mv(w, sm, C, x, nxp, 0.0);
        y = fused_mv(w, sm, Dd, d0, nd, y);
        if (r < ny) y = disturbed(y, p.y_step, p.sy, p.wy, bb * ny + r, bi * ny + r);
        const double ym = fused_pick(w, y, iym, seq);
        if (on) {
            if (p.D && r < nd) p.D[bi * nd + r] = d0;
            if (p.X && r < nxp) p.X[bi * nxp + r] = x;
            if (p.Y && r < ny) p.Y[bi * ny + r] = y;
        }
        if (a.direct) correct(ym, d0);
        double yh = fused_mv(w, sm, Ch, xh, nxh, 0.0);
        yh = fused_mv(w, sm, Chd, d0, nd, yh);
        if (on) {
            if (p.Xhat && r < nxh) p.Xhat[bi * nxh + r] = xh;
            if (p.Yhat && r < ny) p.Yhat[bi * ny + r] = yh;
        }
        // the law: Z̃[0:nu] = g0 + Gx x̂0 + Gu lastu0 + Gr ry + Gd d0 (zero tables for a member whose factorisation failed)
        double z = sm[L0.off];
        z = fused_mv(w, sm, Lx, xh, nxh, z);
        z = fused_mv(w, sm, Lu, lu, nu, z);
        z = fused_mv(w, sm, Lr, ry, ny, z);
        z = fused_mv(w, sm, Ld, d0, nd, z);
        const double u0 = r < nu ? z + lu : 0.0;
        const double ud = r < nu ? disturbed(u0, p.u_step, p.su, p.wu, bb * nu + r, bi * nu + r) : 0.0;
        if (on) {
            if (p.U && r < nu) p.U[bi * nu + r] = u0;
            if (p.Ud && r < nu) p.Ud[bi * nu + r] = ud;
            if (p.status && r == 0) p.status[bi] = fst;
        }
        double xn = fused_mv(w, sm, A, x, nxp, 0.0);
        xn = fused_mv(w, sm, Bu, ud, nu, xn);
        xn = fused_mv(w, sm, Bd, d0, nd, xn);
        if (r < nxp) x = disturbed(xn + fx, nullptr, p.sx, p.wx, bb * nxp + r, bi * nxp + r);
        if (!a.direct) correct(ym, d0);
        double xp = fused_mv(w, sm, Ah, xh, nxh, 0.0);
        xp = fused_mv(w, sm, Bh, u0, nu, xp);
        xp = fused_mv(w, sm, Bdh, d0, nd, xp);
        if (r < nxh) xh = xp + dop;
        lu = u0;
    }
    if (on) {
        if (r < nxp) p.x[b * nxp + r] = x;
        if (r < nxh) const_cast<double*>(p.xhat)[b * nxh + r] = xh;
        if (r < nu) p.lastu0[b * nu + r] = lu;
    }
}

}  // namespace sim
}  // namespace mpcqp
