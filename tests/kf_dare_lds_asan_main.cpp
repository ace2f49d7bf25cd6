// TEST INFRASTRUCTURE ONLY (tests/test_kf_dare_lds.py): a stand-alone program around csrc/mpcqp_host.hip compiled for the host
// with -fsanitize=address,undefined and linked with the CPU emulator objects and the launcher of tests/emu/emu_kf_dare_lds.cpp.
// It builds a SteadyKalmanFilter from Q̂ and R̂ at nx̂ = 33 -- the first size of the LDS-resident solve (csrc/kf_dare_lds_bodies.h;
// padded order 48) --, checks the solved P̂∞ against the Riccati equation itself, swaps the model, solves again (host-synchronous
// and on a stream), reads everything back, walks through what stays refused beyond 32 and destroys the handle.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/mpcqp.h"
#include "../include/mpcqp_mhe.h"

#define CHECK(call)                                                                 \
    do {                                                                            \
        const int rc_ = (call);                                                     \
        if (rc_ != MPCQP_OK) { printf("%s -> %d (%s)\n", #call, rc_, mpcqp_strerror(rc_)); return 1; } \
    } while (0)
#define EXPECT(call, code)                                                          \
    do {                                                                            \
        const int rc_ = (call);                                                     \
        if (rc_ != (code)) { printf("%s -> %d, expected %d\n", #call, rc_, (int)(code)); return 1; } \
    } while (0)

// largest entry of  Â P Â' - Â P Ĉm' (Ĉm P Ĉm' + R̂)⁻¹ Ĉm P Â' + Q̂ - P  for one member with ONE measured output (row iy of Ĉ)
static double riccati_residual(const double* A, const double* C, const double* Q, double R, const double* P, int nx, int ny, int iy) {
    std::vector<double> AP(nx * nx, 0.0), APA(nx * nx, 0.0), APc(nx, 0.0), Pc(nx, 0.0);
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j)
            for (int k = 0; k < nx; ++k) AP[i + nx * j] += A[i + nx * k] * P[k + nx * j];
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j)
            for (int k = 0; k < nx; ++k) APA[i + nx * j] += AP[i + nx * k] * A[j + nx * k];
    double m = R;
    for (int i = 0; i < nx; ++i)
        for (int k = 0; k < nx; ++k) Pc[i] += P[i + nx * k] * C[iy + ny * k];
    for (int i = 0; i < nx; ++i) m += C[iy + ny * i] * Pc[i];
    for (int i = 0; i < nx; ++i)
        for (int k = 0; k < nx; ++k) APc[i] += A[i + nx * k] * Pc[k];
    double worst = 0.0;
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j)
            worst = std::fmax(worst, std::fabs(APA[i + nx * j] - APc[i] * APc[j] / m + Q[i + nx * j] - P[i + nx * j]));
    return worst;
}

int main() {
    const int B = 3, nx = 33, nu = 2, ny = 2, nym = 1;
    mpcqp_dims dims{};
    dims.batch = B; dims.nxhat = nx; dims.nu = nu; dims.ny = ny; dims.nd = 0; dims.Hp = 3; dims.Hc = 1; dims.neps = 1;
    mpcqp_handle h = nullptr;
    CHECK(mpcqp_create(&dims, &h));
    std::vector<double> A(B * nx * nx, 0.0), Bu(B * nx * nu, 0.0), C(B * ny * nx, 0.0);
    std::vector<double> Q(B * nx * nx, 0.0), R(B * nym * nym, 0.0), P0(B * nx * nx, 0.0);
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < nx; ++i) {
            A[b * nx * nx + i + nx * i] = 0.9 - 0.05 * b;
            if (i + 1 < nx) A[b * nx * nx + i + nx * (i + 1)] = 0.1;
            Q[b * nx * nx + i + nx * i] = 0.02 + 0.01 * i;
            P0[b * nx * nx + i + nx * i] = 1.0;
            for (int c = 0; c < nu; ++c) Bu[b * nx * nu + i + nx * c] = 0.1 * (i + c + 1);
            for (int a = 0; a < ny; ++a) C[b * ny * nx + a + ny * i] = std::sin(1.0 + a + 2.0 * i + b);
        }
        R[b] = 0.04;
    }
    const int32_t i_ym[nym] = {1};
    std::vector<int32_t> st(B, -1), it(B, -1), path(B, -1);
    EXPECT(mpcqp_kf_set_steady(h, Q.data(), R.data(), i_ym, nym), MPCQP_ERR_ORDER);        // no model yet
    CHECK(mpcqp_set_model(h, A.data(), Bu.data(), C.data(), nullptr, nullptr, nullptr));
    CHECK(mpcqp_kf_set_steady(h, Q.data(), R.data(), i_ym, nym));
    if (mpcqp_kf_lanes_per_estimator(h) != 64) { printf("lanes per estimator: %d\n", mpcqp_kf_lanes_per_estimator(h)); return 1; }
    std::vector<double> P(B * nx * nx), K(B * nx * nym), K0(B * nx * nym), x(B * nx, 0.5), y(B * nym, 1.0), u(B * nu, -0.2);
    double res = 0.0, gain = 0.0, moved = 0.0;
    for (int pass = 0; pass < 3; ++pass) {
        if (pass == 1) {                                       // a model swap: the old gain stays until the caller re-solves
            for (double& v : A) v *= 0.9;
            CHECK(mpcqp_set_model(h, A.data(), Bu.data(), C.data(), nullptr, nullptr, nullptr));
            CHECK(mpcqp_get(h, MPCQP_GET_KF_GAIN, K.data()));
            for (size_t i = 0; i < K.size(); ++i)
                if (K[i] != K0[i]) { printf("the gain moved before the re-solve\n"); return 1; }
            CHECK(mpcqp_kf_solve_steady(h));
        }
        if (pass == 2) CHECK(mpcqp_kf_solve_steady_device(h, nullptr));
        CHECK(mpcqp_kf_status(h, st.data()));
        CHECK(mpcqp_kf_steady_iters(h, it.data()));
        CHECK(mpcqp_kf_steady_path(h, path.data()));
        CHECK(mpcqp_get(h, MPCQP_GET_KF_COV, P.data()));
        CHECK(mpcqp_get(h, MPCQP_GET_KF_GAIN, K.data()));
        for (int b = 0; b < B; ++b) {
            if (st[b] != 0 || path[b] != 0 || it[b] < 1 || it[b] > 40) { printf("status[%d] = %d, path %d, after %d iterations\n", b, st[b], path[b], it[b]); return 1; }
            res = std::fmax(res, riccati_residual(&A[b * nx * nx], &C[b * ny * nx], &Q[b * nx * nx], R[b], &P[b * nx * nx], nx, ny, i_ym[0]));
            for (int i = 0; i < nx * nym; ++i) gain = std::fmax(gain, std::fabs(K[b * nx * nym + i]));
        }
        if (pass == 0) K0 = K;
        if (pass == 1)
            for (size_t i = 0; i < K.size(); ++i) moved = std::fmax(moved, std::fabs(K[i] - K0[i]));
        CHECK(mpcqp_kf_correct(h, x.data(), y.data(), nullptr));
        CHECK(mpcqp_kf_predict(h, x.data(), u.data(), nullptr));
    }
    if (!(res <= 1e-11) || !(gain > 1e-3) || !(moved > 1e-6) || !std::isfinite(x[0])) {
        printf("residual %g gain %g moved %g x %g\n", res, gain, moved, x[0]);
        return 1;
    }
    // what stays refused beyond 32: the time-varying KalmanFilter and initstate; the handle keeps its solved gain
    K0 = K;
    EXPECT(mpcqp_kf_set_covariances(h, Q.data(), R.data(), P0.data(), i_ym, nym), MPCQP_ERR_UNSUPPORTED);
    EXPECT(mpcqp_est_initstate(h, x.data(), u.data(), y.data(), nullptr, st.data()), MPCQP_ERR_UNSUPPORTED);
    CHECK(mpcqp_kf_steady_iters(h, it.data()));                // (still in steady mode)
    CHECK(mpcqp_get(h, MPCQP_GET_KF_GAIN, K.data()));
    for (size_t i = 0; i < K.size(); ++i)
        if (K[i] != K0[i]) { printf("a refused call moved the gain\n"); return 1; }
    Q[0] = -1.0;                                               // member 0: not positive definite -> status 2, zero gain
    CHECK(mpcqp_kf_set_steady(h, Q.data(), R.data(), i_ym, nym));
    CHECK(mpcqp_kf_status(h, st.data()));
    CHECK(mpcqp_get(h, MPCQP_GET_KF_GAIN, K.data()));
    if (st[0] != 2 || st[1] != 0 || K[0] != 0.0 || K[nx * nym] == 0.0) { printf("status %d %d, K %g %g\n", st[0], st[1], K[0], K[nx * nym]); return 1; }
    CHECK(mpcqp_kf_set(h, K.data(), i_ym, nym));               // leaves the mode
    EXPECT(mpcqp_kf_solve_steady(h), MPCQP_ERR_ORDER);
    CHECK(mpcqp_destroy(h));
    printf("kf dare lds asan ok (Riccati residual %.1e, max |K| %.3f)\n", res, gain);
    return 0;
}
