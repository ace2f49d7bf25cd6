// TEST INFRASTRUCTURE ONLY (tests/test_kf_cov.py): a stand-alone program around csrc/mpcqp_host.hip compiled for the host with
// -fsanitize=address,undefined and linked with the CPU emulator objects.  It sets the covariances of a time-varying
// KalmanFilter, runs three periods (correction + prediction, host pointers), replaces Q̂ / R̂ and P̂, reads everything back and
// destroys the handle: the allocations, uploads and read-backs of the new entry points under the sanitizers.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/mpcqp.h"

#define CHECK(call)                                                                 \
    do {                                                                            \
        const int rc_ = (call);                                                     \
        if (rc_ != MPCQP_OK) { printf("%s -> %d (%s)\n", #call, rc_, mpcqp_strerror(rc_)); return 1; } \
    } while (0)

int main() {
    const int B = 5, nx = 6, nu = 2, ny = 3, nym = 2;          // B = 5: a tail group of one estimator
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
        for (int a = 0; a < nym; ++a) R[b * nym * nym + a + nym * a] = 0.04;
    }
    const int32_t i_ym[nym] = {2, 0};
    CHECK(mpcqp_set_model(h, A.data(), Bu.data(), C.data(), nullptr, nullptr, nullptr));
    CHECK(mpcqp_kf_set_covariances(h, Q.data(), R.data(), P0.data(), i_ym, nym));
    if (mpcqp_kf_lanes_per_estimator(h) != 16) { printf("lanes per estimator: %d\n", mpcqp_kf_lanes_per_estimator(h)); return 1; }
    std::vector<double> x(B * nx, 0.5), y(B * nym, 1.0), u(B * nu, -0.2), P(B * nx * nx), K(B * nx * nym);
    std::vector<int32_t> st(B, -1);
    for (int k = 0; k < 3; ++k) {
        CHECK(mpcqp_kf_correct(h, x.data(), y.data(), nullptr));
        CHECK(mpcqp_kf_predict(h, x.data(), u.data(), nullptr));
        if (k == 0) CHECK(mpcqp_kf_set_covariances(h, Q.data(), R.data(), nullptr, i_ym, nym));       // Q̂, R̂ alone: P̂ stays
    }
    CHECK(mpcqp_get(h, MPCQP_GET_KF_COV, P.data()));
    CHECK(mpcqp_get(h, MPCQP_GET_KF_GAIN, K.data()));
    CHECK(mpcqp_kf_status(h, st.data()));
    double asym = 0.0, gain = 0.0;
    for (int b = 0; b < B; ++b) {
        if (st[b] != 0) { printf("status[%d] = %d\n", b, st[b]); return 1; }
        for (int i = 0; i < nx; ++i)
            for (int j = 0; j < nx; ++j) {
                const double p = P[b * nx * nx + i + nx * j];
                if (!std::isfinite(p)) { printf("P not finite\n"); return 1; }
                asym = std::fmax(asym, std::fabs(p - P[b * nx * nx + j + nx * i]));
            }
        for (int i = 0; i < nx * nym; ++i) gain = std::fmax(gain, std::fabs(K[b * nx * nym + i]));
    }
    if (!(asym <= 1e-12) || !(gain > 1e-3) || !std::isfinite(x[0])) { printf("asym %g gain %g x %g\n", asym, gain, x[0]); return 1; }
    CHECK(mpcqp_kf_set_state_covariance(h, P0.data()));
    P0[1] = 0.5;                                               // not symmetric any more
    if (mpcqp_kf_set_state_covariance(h, P0.data()) != MPCQP_ERR_ARG) { printf("asymmetric P accepted\n"); return 1; }
    CHECK(mpcqp_destroy(h));
    printf("kf asan ok (asym %.1e, max |K| %.3f)\n", asym, gain);
    return 0;
}
