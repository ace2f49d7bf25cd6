// im_bodies.h -- the InternalModel estimator (src/estimator/internal_model.jl) for every member of a batch, written against
// the part of the wave interface every wave has (lane, sync): k_im_* on the device (im_kernels.hip), tests/emu/emu_im.cpp on
// the CPU.  im_launch.h says how the lanes and the LDS are laid out.  Every sum runs over its columns in ascending order, in
// the lane that owns the row, and reads nothing of another member: a member's result does not depend on the batch around it.
//
// The stochastic prediction is NOT formed from the tables Ks, Ps of init_stochpred (construct.jl:1254-1267): block t of
// Ŷs = Ks x̂s + Ps ŷs equals Cs As^(t-1) (Âs x̂s + B̂s ŷs), so the correction computes z = Âs x̂s + B̂s ŷs once -- next period's
// x̂s, kept for the update -- and then Hp times  Ŷs_t = Cs z, z <- As z  with As and Cs in LDS.
#pragma once
#include <math.h>

#include "im_launch.h"
#include "mpcqp_types.h"

namespace mpcqp {
namespace im {

struct Group {
    int r, N;                   // lane inside the group, leading dimension of the LDS matrices
    size_t b, bb;               // member, and the member whose data the lanes read (the last one for an empty group)
    bool on;
    double *M, *R, *v;          // the two LDS matrices of the group and its slice of vector slot 0 (slot k at v + k * WAVE)
};
template <class W>
MPCQP_HD Group group_of(const W& w, const ImArgs& a, int wave, double* mat, double* vec) {
    const int G = a.G, g = w.lane / G, N = mat_dim(G);
    Group q;
    q.r = w.lane % G; q.N = N;
    q.b = (size_t)wave * (size_t)(WAVE / G) + (size_t)g;
    q.on = q.b < (size_t)a.B;
    q.bb = q.on ? q.b : (size_t)a.B - 1;
    q.M = mat + (size_t)g * 2 * N * N; q.R = q.M + N * N;      // (the update has no matrices: never dereferenced there)
    q.v = vec + g * G;
    return q;
}

// Gaussian elimination with partial pivoting of the n x n matrix M (element (i, j) at M[i + N j]) applied to nrhs right-hand
// sides at once, then back-substitution: R[c + N i] is entry i of right-hand side c and of its solution.  Lane i owns row i
// of M during the elimination, lane c right-hand side c throughout.  n and nrhs are the same in every group, so every lane
// of the wavefront passes the same barriers; what differs between the groups is data.  Returns true (in every lane of the
// group) when a pivot was zero, not finite or not above reltol * max|M|: the solution is then not to be used.
template <class W>
MPCQP_HD bool ge_solve(W& w, double* M, double* R, int N, int n, int nrhs, int r, double reltol) {
    double big = 0.0;
    if (reltol > 0.0)
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) big = fmax(big, fabs(M[i + N * j]));
    const double tol = reltol * big;
    bool bad = false;
    for (int k = 0; k < n; ++k) {
        int p = k;
        double best = fabs(M[k + N * k]);
        for (int i = k + 1; i < n; ++i) {
            const double av = fabs(M[i + N * k]);
            if (av > best) { best = av; p = i; }
        }
        if (!(best > tol) || !(best < INFINITY)) bad = true;
        w.sync();               // every lane has read column k (and, one step back, the multipliers of column k - 1)
        if (p != k) {
            if (r < n) { const double t = M[k + N * r]; M[k + N * r] = M[p + N * r]; M[p + N * r] = t; }
            if (r < nrhs) { const double t = R[r + N * k]; R[r + N * k] = R[r + N * p]; R[r + N * p] = t; }
        }
        w.sync();
        if (r > k && r < n) {
            const double l = M[r + N * k] / M[k + N * k];
            M[r + N * k] = l;
            for (int j = k + 1; j < n; ++j) M[r + N * j] -= l * M[k + N * j];
        }
        w.sync();
        if (r < nrhs) {
            const double rk = R[r + N * k];
            for (int i = k + 1; i < n; ++i) R[r + N * i] -= M[i + N * k] * rk;
        }
    }
    if (r < nrhs)
        for (int i = n - 1; i >= 0; --i) {
            double s = R[r + N * i];
            for (int j = i + 1; j < n; ++j) s -= M[i + N * j] * R[r + N * j];
            R[r + N * i] = s / M[i + N * i];
        }
    w.sync();
    return bad;
}

// `flag` of any lane r < n of the group, in every lane of the group (slot: a vector slot nobody else is using)
template <class W>
MPCQP_HD bool group_any(W& w, double* slot, int r, int n, bool flag) {
    slot[r] = flag ? 1.0 : 0.0;
    w.sync();
    bool any = false;
    for (int i = 0; i < n; ++i) any = any || slot[i] != 0.0;
    w.sync();
    return any;
}

// index j with i_ym[j] == r, or -1: the measured channel that output r is
MPCQP_HD int measured_index(const ImArgs& a, int r) {
    int jr = -1;
    for (int j = 0; j < a.nym; ++j)
        if (a.i_ym[j] == r) jr = j;
    return jr;
}

// ŷs of measured channel r (r < nym): y0m - (Ĉm x̂d + D̂dm d0), 0 for a measurement that is not finite; vx, vd: x̂d and d0 in LDS
MPCQP_HD double stoch_output(const ImArgs& a, size_t bb, int r, const double* vx, const double* vd) {
    const int q = a.i_ym[r];
    double acc = 0.0;
    for (int k = 0; k < a.nx; ++k) acc += a.C[(bb * a.nx + k) * a.ny + q] * vx[k];
    for (int e = 0; e < a.nd; ++e) acc += a.Dd[(bb * a.nd + e) * a.ny + q] * vd[e];
    const double y = a.y0m[bb * a.nym + r];
    return fabs(y) < INFINITY ? y - acc : 0.0;
}

// Âs x̂s + B̂s ŷs of row r (r < nxs); vxs: x̂s, vym: the measured entries of ŷs, both in LDS
MPCQP_HD double stoch_next(const ImArgs& a, size_t bb, int r, const double* vxs, const double* vym) {
    const int nxs = a.nxs;
    double z = 0.0;
    for (int k = 0; k < nxs; ++k) z += a.Ahs[(bb * nxs + k) * nxs + r] * vxs[k];
    for (int j = 0; j < a.nym; ++j) z += a.Bhs[(bb * a.nym + j) * nxs + r] * vym[j];
    return z;
}

// init_internalmodel: B̂s = Bs Ds⁻¹ (elimination on Ds' with the rows of Bs as right-hand sides), Âs = As - B̂s Cs; the
// stochastic state, outputs and prediction start at zero, B_eff = B.  A zero or non-finite pivot: status 2, Âs = B̂s = 0.
template <class W>
MPCQP_HD void im_setup_body(W& w, const ImArgs& a, int wave, double* sm) {
    const Group q = group_of(w, a, wave, sm, sm + IM_MAT_DOUBLES);
    const int r = q.r, N = q.N, nxs = a.nxs, nym = a.nym, nY = a.Hp * a.ny;
    const size_t bb = q.bb;
    const double *As = a.As + bb * nxs * nxs, *Bs = a.Bs + bb * nxs * nym, *Cs = a.Cs + bb * nym * nxs, *Ds = a.Ds + bb * nym * nym;
    if (r < nym)
        for (int i = 0; i < nym; ++i) q.M[i + N * r] = Ds[r + nym * i];
    if (r < nxs)
        for (int i = 0; i < nym; ++i) q.R[r + N * i] = Bs[r + nxs * i];
    w.sync();
    bool bad = ge_solve(w, q.M, q.R, N, nym, nxs, r, 0.0);
    bool mine = false;
    if (r < nxs)
        for (int i = 0; i < nym; ++i) mine = mine || !(fabs(q.R[r + N * i]) < INFINITY);
    bad = group_any(w, q.v, r, nxs, mine) || bad;
    if (!q.on) return;
    const size_t b = q.b;
    if (r < nxs) {
        for (int j = 0; j < nym; ++j) a.Bhs[(b * nym + j) * nxs + r] = bad ? 0.0 : q.R[r + N * j];
        for (int k = 0; k < nxs; ++k) {
            double acc = As[r + nxs * k];
            for (int j = 0; j < nym; ++j) acc -= q.R[r + N * j] * Cs[j + nym * k];
            a.Ahs[(b * nxs + k) * nxs + r] = bad ? 0.0 : acc;
        }
        a.xs[b * nxs + r] = 0.0;
        a.z[b * nxs + r] = 0.0;
    }
    if (r < a.ny) a.ys[b * a.ny + r] = 0.0;
    for (int i = r; i < nY; i += a.G) {
        a.Yhs[b * nY + i] = 0.0;
        a.Beff[b * nY + i] = a.Bvec[b * nY + i];
    }
    if (r == 0) a.status[b] = bad ? 2 : 0;
}

// correct_estimate! and predictstoch!: ŷs, z = Âs x̂s + B̂s ŷs, then the Hp blocks of Ŷs and of B_eff = B + Ŷs
template <class W>
MPCQP_HD void im_correct_body(W& w, const ImArgs& a, int wave, double* sm) {
    const Group q = group_of(w, a, wave, sm, sm + IM_MAT_DOUBLES);
    const int r = q.r, N = q.N, nx = a.nx, ny = a.ny, nd = a.nd, nxs = a.nxs, nym = a.nym, nY = a.Hp * ny;
    const size_t bb = q.bb;
    double *vx = q.v, *vd = q.v + WAVE, *vxs = q.v + 2 * WAVE, *vym = q.v + 3 * WAVE, *vz = q.v + 4 * WAVE;      // (vz: two slots)
    const bool off = a.status[bb] != 0;
    if (r < nxs)
        for (int k = 0; k < nxs; ++k) q.M[r + N * k] = a.As[(bb * nxs + k) * nxs + r];
    if (r < nym)
        for (int k = 0; k < nxs; ++k) q.R[r + N * k] = a.Cs[(bb * nxs + k) * nym + r];
    if (r < nx) vx[r] = a.xhat0[bb * nx + r];
    if (r < nd) vd[r] = a.d0[bb * nd + r];
    if (r < nxs) vxs[r] = a.xs[bb * nxs + r];
    const int jr = r < ny ? measured_index(a, r) : -1;
    w.sync();
    if (r < nym) vym[r] = off ? 0.0 : stoch_output(a, bb, r, vx, vd);
    w.sync();
    if (r < nxs) {
        const double z = stoch_next(a, bb, r, vxs, vym);
        vz[r] = z;
        if (q.on) a.z[q.b * nxs + r] = z;
    }
    if (q.on && r < ny) a.ys[q.b * ny + r] = jr >= 0 ? vym[jr] : 0.0;
    w.sync();
    for (int t = 0; t < a.Hp; ++t) {
        const double* zc = vz + (t & 1) * WAVE;
        if (r < ny) {
            double y = 0.0;
            if (jr >= 0)
                for (int k = 0; k < nxs; ++k) y += q.R[jr + N * k] * zc[k];
            if (q.on) {
                const size_t i = q.b * nY + (size_t)t * ny + r;
                a.Yhs[i] = y;
                a.Beff[i] = a.Bvec[i] + y;
            }
        }
        if (r < nxs) {
            double zn = 0.0;
            for (int k = 0; k < nxs; ++k) zn += q.M[r + N * k] * zc[k];
            vz[((t + 1) & 1) * WAVE + r] = zn;
        }
        w.sync();
    }
}

// update_estimate!: x̂d <- Â x̂d + B̂u u0 + B̂d d0 + (f̂op - x̂op), x̂s <- the z of the last correction
template <class W>
MPCQP_HD void im_update_body(W& w, const ImArgs& a, int wave, double* sm) {
    const Group q = group_of(w, a, wave, sm, sm);       // (sm: the IM_VEC vector slots only)
    const int r = q.r, nx = a.nx, nu = a.nu, nd = a.nd, nxs = a.nxs;
    const size_t bb = q.bb;
    double *vx = q.v, *vd = q.v + WAVE, *vu = q.v + 2 * WAVE;
    if (r < nx) vx[r] = a.xhat0[bb * nx + r];
    if (r < nd) vd[r] = a.d0[bb * nd + r];
    if (r < nu) vu[r] = a.u0[bb * nu + r];
    w.sync();
    if (!q.on) return;
    const size_t b = q.b;
    if (r < nx) {
        double xn = 0.0;
        for (int k = 0; k < nx; ++k) xn += a.Ahat[(b * nx + k) * nx + r] * vx[k];
        for (int k = 0; k < nu; ++k) xn += a.Bu[(b * nu + k) * nx + r] * vu[k];
        for (int k = 0; k < nd; ++k) xn += a.Bd[(b * nd + k) * nx + r] * vd[k];
        if (a.dop) xn += a.dop[b * nx + r];
        a.xhat0[b * nx + r] = xn;
    }
    if (r < nxs) a.xs[b * nxs + r] = a.z[b * nxs + r];
}

// init_estimate!: x̂d = (I - Â)⁻¹ (B̂u u0 + B̂d d0 + f̂op - x̂op), ŷs from it, x̂s = (I - Âs)⁻¹ B̂s ŷs.  A member one of whose
// systems is singular (a pivot not above 64 eps max|entry|) or whose solution is not finite: status 1, nothing written.
template <class W>
MPCQP_HD void im_init_body(W& w, const ImArgs& a, int wave, double* sm) {
    const Group q = group_of(w, a, wave, sm, sm + IM_MAT_DOUBLES);
    const int r = q.r, N = q.N, nx = a.nx, nu = a.nu, ny = a.ny, nd = a.nd, nxs = a.nxs, nym = a.nym;
    const size_t bb = q.bb;
    double *vx = q.v, *vd = q.v + WAVE, *vxs = q.v + 2 * WAVE, *vym = q.v + 3 * WAVE, *vf = q.v + 4 * WAVE;
    const double reltol = 64.0 * 2.220446049250313e-16;
    const bool off = a.status[bb] != 0;
    const int jr = r < ny ? measured_index(a, r) : -1;
    if (r < nd) vd[r] = a.d0[bb * nd + r];
    if (r < nx) {
        for (int j = 0; j < nx; ++j) q.M[r + N * j] = (j == r ? 1.0 : 0.0) - a.Ahat[(bb * nx + j) * nx + r];
        double rhs = a.dop ? a.dop[bb * nx + r] : 0.0;
        for (int k = 0; k < nu; ++k) rhs += a.Bu[(bb * nu + k) * nx + r] * a.u0[bb * nu + k];
        for (int k = 0; k < nd; ++k) rhs += a.Bd[(bb * nd + k) * nx + r] * a.d0[bb * nd + k];
        q.R[N * r] = rhs;
    }
    w.sync();
    bool bad = ge_solve(w, q.M, q.R, N, nx, 1, r, reltol);
    const double xd = r < nx ? q.R[N * r] : 0.0;
    if (r < nx) vx[r] = xd;
    w.sync();
    if (r < nym) vym[r] = off ? 0.0 : stoch_output(a, bb, r, vx, vd);
    w.sync();                   // (also: every lane has read its solution out of R)
    if (r < nxs) {
        for (int j = 0; j < nxs; ++j) q.M[r + N * j] = (j == r ? 1.0 : 0.0) - a.Ahs[(bb * nxs + j) * nxs + r];
        double rhs = 0.0;
        for (int j = 0; j < nym; ++j) rhs += a.Bhs[(bb * nym + j) * nxs + r] * vym[j];
        q.R[N * r] = rhs;
    }
    w.sync();
    bad = ge_solve(w, q.M, q.R, N, nxs, 1, r, reltol) || bad;
    const double xs = r < nxs ? q.R[N * r] : 0.0;
    if (r < nxs) vxs[r] = xs;
    bad = group_any(w, vf, r, a.G, !(fabs(xd) < INFINITY) || !(fabs(xs) < INFINITY)) || bad;
    if (!q.on) return;
    const size_t b = q.b;
    if (!bad) {
        if (r < nx) a.xhat0[b * nx + r] = xd;
        if (r < nxs) {
            a.xs[b * nxs + r] = xs;
            a.z[b * nxs + r] = stoch_next(a, bb, r, vxs, vym);
        }
        if (r < ny) a.ys[b * ny + r] = jr >= 0 ? vym[jr] : 0.0;
    }
    if (r == 0) a.init_status[b] = bad ? 1 : 0;
}

// B_eff = B + Ŷs of element i of the batch: after setmodel wrote a new B, with the Ŷs of the last correction
MPCQP_HD void im_beff_body(const ImArgs& a, size_t i) { a.Beff[i] = a.Bvec[i] + a.Yhs[i]; }

}  // namespace im
}  // namespace mpcqp
