// TEST INFRASTRUCTURE ONLY: stand-alone program (own main) of tests/test_mhe_loop.py::test_host_code_under_sanitizers -- a
// MovingHorizonEstimator behind a controller (mpcqp_mhe_attach, mpcqp_loop_device, mpcqp_sim with a moving window, detaching a
// borrowed estimator) and mpcqp_est_initstate of csrc/mpcqp_host.hip, compiled with -fsanitize=address,undefined, on the
// emulator objects (whose device memory is the host's: host arrays serve as device pointers).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../include/mpcqp_mhe.h"
#define CHECK(x) do { int rc_ = (x); if (rc_ != 0) { std::printf("%s -> %d\n", #x, rc_); return 1; } } while (0)
typedef std::vector<double> vec;
int main() {
    const int B = 5, nx = 3, nu = 2, ny = 2, nd = 1, Hp = 6, Hc = 2, n = nu * Hc, nxp = 4, N = 5, He = 2, nym = 1;
    unsigned s = 1234;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (1u << 24) - 0.5; };
    auto fill = [&](vec& v, double scale) { for (auto& x : v) x = scale * rnd(); };
    vec A(B * nx * nx), Bu(B * nx * nu), C(B * ny * nx), Bd(B * nx * nd), Dd(B * ny * nd);
    for (auto* v : {&A, &Bu, &C, &Bd, &Dd}) fill(*v, 0.8);
    const int32_t iym[1] = {1};
    // the estimator's model: the measured rows of Ĉ and D̂d (column-major per member)
    vec Cm(B * nym * nx), Ddm(B * nym * nd);
    for (int b = 0; b < B; ++b) {
        for (int j = 0; j < nx; ++j) Cm[(size_t)b * nx + j] = C[(size_t)b * ny * nx + iym[0] + ny * j];
        for (int j = 0; j < nd; ++j) Ddm[(size_t)b * nd + j] = Dd[(size_t)b * ny * nd + iym[0] + ny * j];
    }
    vec Q(B * nx * nx, 0.0), R(B * nym * nym, 0.2), P0(B * nx * nx, 0.0);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < nx; ++i) Q[(size_t)b * nx * nx + i * (nx + 1)] = 0.05, P0[(size_t)b * nx * nx + i * (nx + 1)] = 0.5;
    vec pA(B * nxp * nxp), pBu(B * nxp * nu), pC(B * ny * nxp), pBd(B * nxp * nd), pDd(B * ny * nd);
    for (auto* v : {&pA, &pBu, &pC, &pBd, &pDd}) fill(*v, 0.6);
    vec M(B * ny * Hp, 1.0), Nw(B * n, 0.1), L(B * nu * Hp, 0.05);
    vec ry(B * ny), d(B * nd), sy(B * ny, 0.1), wy(B * N * ny);
    for (auto* v : {&ry, &d, &wy}) fill(*v, 1.0);

    for (int direct = 1; direct >= 0; --direct) {
        mpcqp_dims dm{};
        dm.batch = B; dm.nxhat = nx; dm.nu = nu; dm.ny = ny; dm.nd = nd; dm.Hp = Hp; dm.Hc = Hc; dm.neps = 0;
        dm.flags = MPCQP_FLAG_RY_CONSTANT;
        mpcqp_handle h = nullptr;
        CHECK(mpcqp_create(&dm, &h));
        CHECK(mpcqp_set_model(h, A.data(), Bu.data(), C.data(), Bd.data(), Dd.data(), nullptr));
        CHECK(mpcqp_set_weights(h, M.data(), Nw.data(), L.data(), nullptr));
        CHECK(mpcqp_sim_set_plant(h, nxp, pA.data(), pBu.data(), pC.data(), pBd.data(), pDd.data(), nullptr));
        auto estimator = [&](int batch, int nym_, mpcqp_mhe* e) {
            mpcqp_mhe_dims ed{};
            ed.batch = batch; ed.nxhat = nx; ed.nu = nu; ed.nym = nym_; ed.nd = nd; ed.He = He; ed.direct = direct;
            return mpcqp_mhe_create(&ed, e);
        };
        mpcqp_mhe e = nullptr, wrongB = nullptr;
        CHECK(estimator(B, nym, &e));
        CHECK(estimator(B - 1, nym, &wrongB));
        CHECK(mpcqp_mhe_set_model(e, A.data(), Bu.data(), Cm.data(), Bd.data(), Ddm.data(), nullptr, Q.data(), R.data()));
        CHECK(mpcqp_mhe_init(e, nullptr, P0.data(), nullptr, nullptr));
        mpcqp_mhe_dims back{};
        CHECK(mpcqp_mhe_get_dims(e, &back));
        if (back.batch != B || back.He != He || back.direct != direct || back.nym != nym) return 2;

        vec x0(B * nxp), xh(B * nx), lu(B * nu), Z(B * n, 0.0), u0(B * nu), y0m(B * nym), Dh(B * nd * Hp);
        for (auto* v : {&x0, &xh, &lu, &y0m}) fill(*v, 0.5);
        for (int b = 0; b < B; ++b) for (int t = 0; t < Hp; ++t) Dh[(size_t)(b * Hp + t) * nd] = d[b];
        std::vector<int32_t> st(B, -1), it(B, -1), est((size_t)N * B, -1), ist(B, -1);
        mpcqp_sim_io io{};
        io.N = N; io.ry = ry.data(); io.d = d.data(); io.x0 = x0.data(); io.xhat0 = xh.data(); io.lastu0 = lu.data(); io.Ztilde = Z.data();
        io.sigma_y = sy.data(); io.w_y = wy.data();
        // nothing attached
        if (mpcqp_sim(h, &io) != MPCQP_ERR_ORDER) return 3;
        if (mpcqp_loop_device(h, xh.data(), y0m.data(), lu.data(), ry.data(), nullptr, d.data(), Dh.data(), Z.data(), u0.data(), st.data(),
                              it.data(), nullptr, nullptr) != MPCQP_ERR_ORDER) return 4;
        if (mpcqp_est_initstate(h, xh.data(), lu.data(), y0m.data(), d.data(), ist.data()) != MPCQP_ERR_ORDER) return 5;
        if (mpcqp_sim_est_status(h, est.data(), 1) != MPCQP_ERR_ORDER) return 6;
        // refusals of the attachment
        if (mpcqp_mhe_attach(h, wrongB, iym, nym) != MPCQP_ERR_DIMS) return 7;
        const int32_t two[2] = {0, 1}, outside[1] = {2};
        if (mpcqp_mhe_attach(h, e, two, 2) != MPCQP_ERR_DIMS) return 8;
        if (mpcqp_mhe_attach(h, e, outside, 1) != MPCQP_ERR_ARG) return 9;
        if (mpcqp_mhe_attach(h, e, nullptr, 1) != MPCQP_ERR_NULL) return 10;
        CHECK(mpcqp_mhe_attach(h, e, iym, nym));
        if (mpcqp_sim_path(h) != MPCQP_SIM_PATH_PERIOD) return 11;

        // the loop: three periods, the window grows and then moves (He = 2)
        const vec xh_before = xh;
        for (int k = 0; k < 3; ++k) {
            CHECK(mpcqp_loop_device(h, xh.data(), y0m.data(), lu.data(), ry.data(), nullptr, d.data(), Dh.data(), Z.data(), u0.data(),
                                    st.data(), it.data(), nullptr, nullptr));
            lu = u0;
            for (int32_t v : st) if (v != 0) return 12;
        }
        if (mpcqp_mhe_nk(e) != He) return 13;
        if (direct && xh == xh_before) return 14;          // the caller's x̂0 received the estimate the step used
        vec xe(B * nx);
        CHECK(mpcqp_mhe_get(e, MPCQP_MHE_XHAT0, xe.data()));
        for (double v : xe) if (!std::isfinite(v)) return 15;

        // a simulation with a moving window, every record asked for
        vec Y(B * N * ny), X(B * N * nxp), D(B * N * nd), Xh(B * N * nx), Yh(B * N * ny), U(B * N * nu), Ud(B * N * nu);
        std::vector<int32_t> cst(B * N, -1);
        io.Y = Y.data(); io.X = X.data(); io.D = D.data(); io.Xhat = Xh.data(); io.Yhat = Yh.data(); io.U = U.data(); io.Ud = Ud.data();
        io.status = cst.data();
        CHECK(mpcqp_sim(h, &io));
        CHECK(mpcqp_sim_est_status(h, est.data(), N));
        if (mpcqp_sim_est_status(h, est.data(), N + 1) != MPCQP_ERR_ARG) return 16;
        for (int32_t v : est) if (v != 0) return 17;
        for (int32_t v : cst) if (v != 0) return 18;
        for (auto* v : {&Y, &X, &D, &Xh, &Yh, &U, &Ud, &x0, &xh, &lu}) for (double w : *v) if (!std::isfinite(w)) return 19;
        CHECK(mpcqp_mhe_get(e, MPCQP_MHE_XHAT0, xe.data()));
        if (xe != xh) return 20;                            // io->xhat0 received the last estimate

        // initstate: solved members, one member without full column rank (its Ĉ and its row of Â zeroed in column 0 ...)
        vec xi(B * nx, 7.0);
        CHECK(mpcqp_est_initstate(h, xi.data(), lu.data(), y0m.data(), d.data(), ist.data()));
        for (int b = 0; b < B; ++b) {
            if (ist[b] != 0) return 21;
            for (int i = 0; i < nx; ++i) if (xi[(size_t)b * nx + i] == 7.0 || !std::isfinite(xi[(size_t)b * nx + i])) return 22;
        }
        vec A2 = A, C2 = C;
        for (int i = 0; i < nx; ++i) A2[(size_t)2 * nx * nx + i] = i == 0 ? 1.0 : 0.0;        // member 2: column 0 of I - Â is zero
        for (int i = 0; i < ny; ++i) C2[(size_t)2 * ny * nx + i] = 0.0;                       // ... and column 0 of Ĉ
        CHECK(mpcqp_set_model(h, A2.data(), Bu.data(), C2.data(), Bd.data(), Dd.data(), nullptr));
        vec xj(B * nx, 7.0);
        CHECK(mpcqp_est_initstate(h, xj.data(), lu.data(), y0m.data(), d.data(), ist.data()));
        for (int b = 0; b < B; ++b) {
            if (ist[b] != (b == 2 ? 1 : 0)) return 23;
            for (int i = 0; i < nx; ++i)
                if (b == 2 ? xj[(size_t)b * nx + i] != 7.0 : xj[(size_t)b * nx + i] != xi[(size_t)b * nx + i]) return 24;
        }

        // detach while the estimator is borrowed, then destroy it: the controller no longer touches it
        CHECK(mpcqp_mhe_attach(h, nullptr, nullptr, 0));
        CHECK(mpcqp_mhe_destroy(e));
        if (mpcqp_sim(h, &io) != MPCQP_ERR_ORDER) return 25;
        // a Kalman gain after an attachment: a Kalman handle again
        mpcqp_mhe e2 = nullptr;
        CHECK(estimator(B, nym, &e2));
        CHECK(mpcqp_mhe_set_model(e2, A.data(), Bu.data(), Cm.data(), Bd.data(), Ddm.data(), nullptr, Q.data(), R.data()));
        CHECK(mpcqp_mhe_init(e2, nullptr, P0.data(), nullptr, nullptr));
        CHECK(mpcqp_mhe_attach(h, e2, iym, nym));
        vec K(B * nx * nym, 0.1);
        CHECK(mpcqp_kf_set(h, K.data(), iym, nym));
        CHECK(mpcqp_mhe_destroy(e2));
        CHECK(mpcqp_sim(h, &io));                           // runs on the gain; e2 is gone
        if (mpcqp_sim_est_status(h, est.data(), 1) != MPCQP_ERR_ORDER) return 26;
        CHECK(mpcqp_mhe_destroy(wrongB));
        CHECK(mpcqp_destroy(h));
    }
    std::printf("mhe loop sanitizer run: ok\n");
    return 0;
}
