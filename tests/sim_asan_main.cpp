// TEST INFRASTRUCTURE ONLY: stand-alone program (own main) of tests/test_sim.py::test_host_code_under_sanitizers -- the
// simulation entry points of csrc/mpcqp_host.hip, compiled with -fsanitize=address,undefined, on the emulator objects.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/mpcqp.h"
#define CHECK(x) do { int rc_ = (x); if (rc_ != 0) { std::printf("%s -> %d\n", #x, rc_); return 1; } } while (0)
typedef std::vector<double> vec;
int main() {
    const int B = 5, nx = 3, nu = 2, ny = 2, nd = 1, Hp = 6, Hc = 2, n = nu * Hc, nxp = 4, N = 4;
    unsigned s = 4711;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (1u << 24) - 0.5; };
    auto fill = [&](vec& v, double scale) { for (auto& x : v) x = scale * rnd(); };
    vec A(B * nx * nx), Bu(B * nx * nu), C(B * ny * nx), Bd(B * nx * nd), Dd(B * ny * nd);
    for (auto* v : {&A, &Bu, &C, &Bd, &Dd}) fill(*v, 0.8);
    vec pA(B * nxp * nxp), pBu(B * nxp * nu), pC(B * ny * nxp), pBd(B * nxp * nd), pDd(B * ny * nd), fx(B * nxp);
    for (auto* v : {&pA, &pBu, &pC, &pBd, &pDd, &fx}) fill(*v, 0.6);
    vec K(B * nx * ny);
    fill(K, 0.4);
    const int32_t iym[2] = {1, 0};
    vec M(B * ny * Hp, 1.0), Nw(B * n, 0.1), L(B * nu * Hp, 0.05);
    vec ry(B * ny), ryN(B * N * ny), d(B * nd), us(B * nu), ys(B * ny), ds(B * nd), su(B * nu), sy(B * ny), sd(B * nd), sx(B * nxp);
    vec wu(B * N * nu), wy(B * N * ny), wd(B * N * nd), wx(B * N * nxp);
    for (auto* v : {&ry, &ryN, &d, &us, &ys, &ds, &wu, &wy, &wd, &wx}) fill(*v, 1.0);
    for (auto* v : {&su, &sy, &sd, &sx}) for (auto& x : *v) x = 0.1 + 0.1 * std::fabs(rnd());

    // kind 0: explicit law, 1: explicit step, 2: mpcqp_step (unconstrained); each in both forms of the estimator
    for (int kind = 0; kind < 3; ++kind)
        for (int direct = 1; direct >= 0; --direct) {
            mpcqp_dims dm{};
            dm.batch = B; dm.nxhat = nx; dm.nu = nu; dm.ny = ny; dm.nd = nd; dm.Hp = Hp; dm.Hc = Hc; dm.neps = 0;
            mpcqp_handle h = nullptr;
            CHECK(mpcqp_create(&dm, &h));
            vec x0(B * nxp), xh(B * nx), lu(B * nu), Z(B * n, 0.0);
            for (auto* v : {&x0, &xh, &lu}) fill(*v, 0.5);
            vec Y(B * N * ny), X(B * N * nxp), D(B * N * nd), Xh(B * N * nx), Yh(B * N * ny), U(B * N * nu), Ud(B * N * nu);
            std::vector<int32_t> st(B * N, -1);
            mpcqp_sim_io io{};
            io.N = N; io.ry = ry.data(); io.d = d.data(); io.x0 = x0.data(); io.xhat0 = xh.data(); io.lastu0 = lu.data();
            io.Ztilde = Z.data();
            if (mpcqp_sim(h, &io) != MPCQP_ERR_ORDER) return 2;                 // nothing attached
            CHECK(mpcqp_set_model(h, A.data(), Bu.data(), C.data(), Bd.data(), Dd.data(), nullptr));
            CHECK(mpcqp_set_weights(h, M.data(), Nw.data(), L.data(), nullptr));
            if (kind < 2) CHECK(mpcqp_explicit_prepare(h, kind == 0 ? MPCQP_EXPLICIT_LAW : 0));
            if (mpcqp_sim_set_plant(h, 65, pA.data(), pBu.data(), pC.data(), nullptr, nullptr, nullptr) != MPCQP_ERR_UNSUPPORTED) return 3;
            if (mpcqp_sim_set_plant(h, 0, pA.data(), pBu.data(), pC.data(), nullptr, nullptr, nullptr) != MPCQP_ERR_ARG) return 3;
            CHECK(mpcqp_sim_set_plant(h, nxp, pA.data(), pBu.data(), pC.data(), nullptr, nullptr, nullptr));
            CHECK(mpcqp_sim_set_plant(h, nxp, pA.data(), pBu.data(), pC.data(), pBd.data(), pDd.data(), fx.data()));      // repeated
            if (mpcqp_sim(h, &io) != MPCQP_ERR_ORDER) return 4;                 // no estimator
            CHECK(mpcqp_kf_set(h, K.data(), iym, 2));
            CHECK(mpcqp_kf_set_direct(h, direct));
            io.N = 0;
            if (mpcqp_sim(h, &io) != MPCQP_ERR_ARG) return 5;
            io.N = N;
            io.sigma_x = sx.data();
            if (mpcqp_sim(h, &io) != MPCQP_ERR_NULL) return 6;                  // σ without draws
            io.u_step = us.data(); io.y_step = ys.data(); io.d_step = ds.data();
            io.sigma_u = su.data(); io.sigma_y = sy.data(); io.sigma_d = sd.data();
            io.w_u = wu.data(); io.w_y = wy.data(); io.w_d = wd.data(); io.w_x = wx.data();
            io.Y = Y.data(); io.X = X.data(); io.D = D.data(); io.Xhat = Xh.data(); io.Yhat = Yh.data(); io.U = U.data(); io.Ud = Ud.data();
            io.status = st.data();
            io.ry = ryN.data(); io.flags = MPCQP_SIM_FLAG_RY_PER_PERIOD | MPCQP_SIM_FLAG_NO_FUSE;
            const vec x00 = x0, xh0 = xh, lu0 = lu;
            CHECK(mpcqp_sim(h, &io));
            if (mpcqp_sim_path(h) != (kind == 0 ? MPCQP_SIM_PATH_FUSED : MPCQP_SIM_PATH_PERIOD)) return 7;
            for (int32_t v : st) if (v != 0) return 8;
            for (auto* v : {&Y, &X, &D, &Xh, &Yh, &U, &Ud, &x0, &xh, &lu}) for (double e : *v) if (!std::isfinite(e)) return 9;
            // two runs of N / 2 from the same start: the same bits (draws and set points sliced per member)
            const int H = N / 2;
            vec x1 = x00, xh1 = xh0, lu1 = lu0, Z1(B * n, 0.0);
            mpcqp_handle g = nullptr;
            CHECK(mpcqp_create(&dm, &g));
            CHECK(mpcqp_set_model(g, A.data(), Bu.data(), C.data(), Bd.data(), Dd.data(), nullptr));
            CHECK(mpcqp_set_weights(g, M.data(), Nw.data(), L.data(), nullptr));
            if (kind < 2) CHECK(mpcqp_explicit_prepare(g, kind == 0 ? MPCQP_EXPLICIT_LAW : 0));
            CHECK(mpcqp_sim_set_plant(g, nxp, pA.data(), pBu.data(), pC.data(), pBd.data(), pDd.data(), fx.data()));
            CHECK(mpcqp_kf_set(g, K.data(), iym, 2));
            CHECK(mpcqp_kf_set_direct(g, direct));
            for (int half = 0; half < 2; ++half) {
                auto cut = [&](const vec& w, int m) {
                    vec o((size_t)B * H * m);
                    for (int b = 0; b < B; ++b)
                        std::memcpy(&o[(size_t)b * H * m], &w[((size_t)b * N + (size_t)half * H) * m], sizeof(double) * H * m);
                    return o;
                };
                vec cu = cut(wu, nu), cy = cut(wy, ny), cd = cut(wd, nd), cx = cut(wx, nxp), cr = cut(ryN, ny);
                vec U2((size_t)B * H * nu), Xh2((size_t)B * H * nx);
                mpcqp_sim_io j = io;
                j.N = H; j.w_u = cu.data(); j.w_y = cy.data(); j.w_d = cd.data(); j.w_x = cx.data(); j.ry = cr.data();
                j.x0 = x1.data(); j.xhat0 = xh1.data(); j.lastu0 = lu1.data(); j.Ztilde = kind == 0 ? nullptr : Z1.data();
                j.Y = j.X = j.D = j.Yhat = j.Ud = nullptr; j.status = nullptr;      // records that are not asked for
                j.U = U2.data(); j.Xhat = Xh2.data();
                CHECK(mpcqp_sim(g, &j));
                for (int b = 0; b < B; ++b)
                    for (int i = 0; i < H; ++i) {
                        for (int c = 0; c < nu; ++c) if (U2[((size_t)b * H + i) * nu + c] != U[((size_t)b * N + half * H + i) * nu + c]) return 10;
                        for (int c = 0; c < nx; ++c) if (Xh2[((size_t)b * H + i) * nx + c] != Xh[((size_t)b * N + half * H + i) * nx + c]) return 11;
                    }
            }
            if (x1 != x0 || xh1 != xh || lu1 != lu) return 12;
            if (kind != 0 && Z1 != Z) return 13;
            if (kind == 0) {
                // the single-launch path (ry held, no flag): within 1e-9 of the per-period records of the same draws, and two
                // runs of N / 2 equal one of N bit for bit
                vec xa = x00, xha = xh0, lua = lu0, xb = x00, xhb = xh0, lub = lu0, Up(B * N * nu), Uf(B * N * nu), Xf(B * N * nx);
                mpcqp_sim_io f = io;
                f.flags = MPCQP_SIM_FLAG_NO_FUSE; f.ry = ry.data(); f.Ztilde = nullptr;
                f.x0 = xa.data(); f.xhat0 = xha.data(); f.lastu0 = lua.data(); f.U = Up.data();
                CHECK(mpcqp_sim(h, &f));
                xa = x00; xha = xh0; lua = lu0;
                f.flags = 0; f.U = Uf.data(); f.Xhat = Xf.data();
                CHECK(mpcqp_sim(h, &f));
                for (size_t k = 0; k < Uf.size(); ++k) if (!(std::fabs(Uf[k] - Up[k]) <= 1e-9 * (1.0 + std::fabs(Up[k])))) return 14;
                for (int half = 0; half < 2; ++half) {
                    auto cut = [&](const vec& w, int m) {
                        vec o((size_t)B * H * m);
                        for (int b = 0; b < B; ++b)
                            std::memcpy(&o[(size_t)b * H * m], &w[((size_t)b * N + (size_t)half * H) * m], sizeof(double) * H * m);
                        return o;
                    };
                    vec cu = cut(wu, nu), cy = cut(wy, ny), cd = cut(wd, nd), cx = cut(wx, nxp), U2((size_t)B * H * nu);
                    mpcqp_sim_io j = f;
                    j.N = H; j.w_u = cu.data(); j.w_y = cy.data(); j.w_d = cd.data(); j.w_x = cx.data();
                    j.x0 = xb.data(); j.xhat0 = xhb.data(); j.lastu0 = lub.data();
                    j.Y = j.X = j.D = j.Yhat = j.Ud = j.Xhat = nullptr; j.status = nullptr; j.U = U2.data();
                    CHECK(mpcqp_sim(g, &j));
                    for (int b = 0; b < B; ++b)
                        for (int k = 0; k < H * nu; ++k) if (U2[(size_t)b * H * nu + k] != Uf[((size_t)b * N + half * H) * nu + k]) return 15;
                }
                if (xb != xa || xhb != xha || lub != lua) return 16;
            }
            CHECK(mpcqp_destroy(g));
            CHECK(mpcqp_destroy(h));
        }
    std::printf("sim sanitizer run: ok\n");
    return 0;
}
