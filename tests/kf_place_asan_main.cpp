// TEST INFRASTRUCTURE ONLY (tests/test_kf_place.py): a stand-alone program around csrc/mpcqp_host.hip compiled for the host with
// -fsanitize=address,undefined and linked with the CPU emulator objects.  It builds a Luenberger observer from its poles, checks
// the placed poles through the characteristic polynomial of Â (I - K̂ Ĉm), swaps the model, places again (host-synchronous and
// on a stream), reads everything back, walks through the refusals and destroys the handle: the allocations, uploads, launches
// and read-backs of the new entry points under the sanitizers.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../include/mpcqp.h"

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

// largest |det(p_j I - Â (I - K̂ Ĉm))| over the poles of one member with ONE measured output (row iy of Ĉ), relative to the
// product of the column norms of the matrix: zero at a placed pole
static double pole_residual(const double* A, const double* C, const double* K, const double* p, int nx, int ny, int iy) {
    std::vector<double> M(nx * nx), T(nx * nx);
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j) {
            double s = 0.0;
            for (int k = 0; k < nx; ++k) s += A[i + nx * k] * ((k == j ? 1.0 : 0.0) - K[k] * C[iy + ny * j]);
            M[i + nx * j] = s;
        }
    double worst = 0.0;
    for (int e = 0; e < nx; ++e) {
        for (int i = 0; i < nx * nx; ++i) T[i] = -M[i];
        for (int i = 0; i < nx; ++i) T[i + nx * i] += p[e];
        double det = 1.0, scale = 1.0;
        for (int j = 0; j < nx; ++j) {
            double s = 0.0;
            for (int i = 0; i < nx; ++i) s += T[i + nx * j] * T[i + nx * j];
            scale *= std::sqrt(s);
        }
        for (int k = 0; k < nx; ++k) {              // elimination with partial pivoting
            int piv = k;
            for (int i = k + 1; i < nx; ++i)
                if (std::fabs(T[i + nx * k]) > std::fabs(T[piv + nx * k])) piv = i;
            if (piv != k) {
                for (int j = 0; j < nx; ++j) std::swap(T[k + nx * j], T[piv + nx * j]);
                det = -det;
            }
            det *= T[k + nx * k];
            if (T[k + nx * k] == 0.0) break;
            for (int i = k + 1; i < nx; ++i) {
                const double f = T[i + nx * k] / T[k + nx * k];
                for (int j = k; j < nx; ++j) T[i + nx * j] -= f * T[k + nx * j];
            }
        }
        worst = std::fmax(worst, std::fabs(det) / scale);
    }
    return worst;
}

int main() {
    const int B = 5, nx = 6, nu = 2, ny = 3, nym = 1;
    mpcqp_dims dims{};
    dims.batch = B; dims.nxhat = nx; dims.nu = nu; dims.ny = ny; dims.nd = 0; dims.Hp = 3; dims.Hc = 1; dims.neps = 1;
    mpcqp_handle h = nullptr;
    CHECK(mpcqp_create(&dims, &h));
    std::vector<double> A(B * nx * nx, 0.0), Bu(B * nx * nu, 0.0), C(B * ny * nx, 0.0), poles(B * nx, 0.0);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < nx; ++i) {
            A[b * nx * nx + i + nx * i] = 0.9 - 0.05 * b - 0.07 * i;
            if (i + 1 < nx) A[b * nx * nx + i + nx * (i + 1)] = 0.1;
            if (i > 0) A[b * nx * nx + i + nx * (i - 1)] = 0.05;
            poles[b * nx + i] = 0.1 + 0.1 * i + 0.01 * b;
            for (int c = 0; c < nu; ++c) Bu[b * nx * nu + i + nx * c] = 0.1 * (i + c + 1);
            for (int a = 0; a < ny; ++a) C[b * ny * nx + a + ny * i] = std::sin(1.0 + a + 2.0 * i + b);
        }
    const int32_t iym[1] = {1}, twice[2] = {1, 1};
    std::vector<double> K(B * nx * nym), K2(B * nx * nym), P(B * nx * nx);
    std::vector<int32_t> st(B), sw(B);

    // refusals in front of the mode
    EXPECT(mpcqp_kf_set_poles(h, poles.data(), iym, nym), MPCQP_ERR_ORDER);         // no model yet
    CHECK(mpcqp_set_model(h, A.data(), Bu.data(), C.data(), nullptr, nullptr, nullptr));
    EXPECT(mpcqp_kf_set_poles(h, nullptr, iym, nym), MPCQP_ERR_NULL);
    EXPECT(mpcqp_kf_set_poles(h, poles.data(), twice, 2), MPCQP_ERR_ARG);
    EXPECT(mpcqp_kf_set_poles(h, poles.data(), iym, ny + 1), MPCQP_ERR_DIMS);
    poles[3] = 1.0;
    EXPECT(mpcqp_kf_set_poles(h, poles.data(), iym, nym), MPCQP_ERR_ARG);
    poles[3] = std::nan("");
    EXPECT(mpcqp_kf_set_poles(h, poles.data(), iym, nym), MPCQP_ERR_ARG);
    poles[3] = 0.4;
    EXPECT(mpcqp_kf_place(h), MPCQP_ERR_ORDER);
    EXPECT(mpcqp_kf_place_device(h, nullptr), MPCQP_ERR_ORDER);
    EXPECT(mpcqp_kf_place_sweeps(h, sw.data()), MPCQP_ERR_ORDER);
    EXPECT(mpcqp_kf_set_place_cap(h, 3), MPCQP_ERR_ORDER);

    // set: placed, read back
    CHECK(mpcqp_kf_set_poles(h, poles.data(), iym, nym));
    CHECK(mpcqp_kf_status(h, st.data()));
    CHECK(mpcqp_kf_place_sweeps(h, sw.data()));
    CHECK(mpcqp_get(h, MPCQP_GET_KF_GAIN, K.data()));
    EXPECT(mpcqp_get(h, MPCQP_GET_KF_COV, P.data()), MPCQP_ERR_ORDER);
    EXPECT(mpcqp_kf_lanes_per_estimator(h), 64);
    EXPECT(mpcqp_kf_steady_iters(h, sw.data()), MPCQP_ERR_ORDER);
    for (int b = 0; b < B; ++b) {
        if (st[b] != 0) { printf("member %d: status %d\n", b, st[b]); return 1; }
        const double res = pole_residual(&A[b * nx * nx], &C[b * ny * nx], &K[b * nx], &poles[b * nx], nx, ny, iym[0]);
        if (!(res <= 1e-10)) { printf("member %d: pole residual %g\n", b, res); return 1; }
    }
    // one output: the gain is unique, whatever the cap
    EXPECT(mpcqp_kf_set_place_cap(h, 101), MPCQP_ERR_ARG);
    EXPECT(mpcqp_kf_set_place_cap(h, -1), MPCQP_ERR_ARG);
    CHECK(mpcqp_kf_set_place_cap(h, 0));
    CHECK(mpcqp_kf_place(h));
    CHECK(mpcqp_kf_place_sweeps(h, sw.data()));
    for (int b = 0; b < B; ++b)
        if (sw[b] != 0) { printf("member %d: %d sweeps at cap 0\n", b, sw[b]); return 1; }
    CHECK(mpcqp_kf_set_place_cap(h, 30));

    // a model swap: the old gain stays until the placement runs again, host-synchronous and on a stream
    for (double& v : A) v *= 0.9;
    CHECK(mpcqp_set_model(h, A.data(), Bu.data(), C.data(), nullptr, nullptr, nullptr));
    CHECK(mpcqp_get(h, MPCQP_GET_KF_GAIN, K2.data()));
    for (size_t i = 0; i < K.size(); ++i)
        if (std::fabs(K2[i] - K[i]) > 1e-9 * (1.0 + std::fabs(K[i]))) { printf("the gain moved with set_model alone\n"); return 1; }
    CHECK(mpcqp_kf_place(h));
    CHECK(mpcqp_get(h, MPCQP_GET_KF_GAIN, K.data()));
    CHECK(mpcqp_kf_place_device(h, nullptr));
    CHECK(mpcqp_get(h, MPCQP_GET_KF_GAIN, K2.data()));
    CHECK(mpcqp_kf_status(h, st.data()));
    for (int b = 0; b < B; ++b) {
        if (st[b] != 0) { printf("member %d: status %d after the swap\n", b, st[b]); return 1; }
        const double res = pole_residual(&A[b * nx * nx], &C[b * ny * nx], &K[b * nx], &poles[b * nx], nx, ny, iym[0]);
        if (!(res <= 1e-10)) { printf("member %d: pole residual %g after the swap\n", b, res); return 1; }
    }
    for (size_t i = 0; i < K.size(); ++i)
        if (K2[i] != K[i]) { printf("_device differs from the host call\n"); return 1; }

    // the estimator steps of a steady gain
    std::vector<double> x(B * nx, 0.0), y(B * nym, 1.0), u(B * nu, 0.5);
    CHECK(mpcqp_kf_correct(h, x.data(), y.data(), nullptr));
    CHECK(mpcqp_kf_predict(h, x.data(), u.data(), nullptr));
    CHECK(mpcqp_kf_update(h, x.data(), u.data(), y.data(), nullptr));

    // a member that breaks down keeps its gain: a NaN in its Â
    const double keep = A[2 * nx * nx + 1];
    A[2 * nx * nx + 1] = std::nan("");
    CHECK(mpcqp_set_model(h, A.data(), Bu.data(), C.data(), nullptr, nullptr, nullptr));
    CHECK(mpcqp_kf_place(h));
    CHECK(mpcqp_kf_status(h, st.data()));
    CHECK(mpcqp_get(h, MPCQP_GET_KF_GAIN, K2.data()));
    for (int b = 0; b < B; ++b)
        if (st[b] != (b == 2 ? 2 : 0)) { printf("member %d: status %d with a NaN in member 2\n", b, st[b]); return 1; }
    for (size_t i = 0; i < K.size(); ++i)
        if (K2[i] != K[i]) { printf("a gain changed around a broken member\n"); return 1; }
    A[2 * nx * nx + 1] = keep;
    CHECK(mpcqp_set_model(h, A.data(), Bu.data(), C.data(), nullptr, nullptr, nullptr));

    // leaving the mode
    CHECK(mpcqp_kf_set(h, K.data(), iym, nym));
    EXPECT(mpcqp_kf_place(h), MPCQP_ERR_ORDER);
    EXPECT(mpcqp_kf_place_sweeps(h, sw.data()), MPCQP_ERR_ORDER);
    EXPECT(mpcqp_kf_status(h, st.data()), MPCQP_ERR_ORDER);
    EXPECT(mpcqp_kf_lanes_per_estimator(h), 0);
    CHECK(mpcqp_kf_set_poles(h, poles.data(), iym, nym));
    CHECK(mpcqp_destroy(h));
    printf("kf place asan ok\n");
    return 0;
}
