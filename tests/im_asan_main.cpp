// TEST INFRASTRUCTURE ONLY (tests/test_im_asan.py): a stand-alone program around csrc/mpcqp_host.hip compiled for the host with
// -fsanitize=address,undefined and linked with the CPU emulator objects.  It attaches an InternalModel with a general
// stochastic model (nxs != nym, i_ym not a prefix), runs three periods of correct / update (host pointers), initstate,
// set_model (the refresh of B + Ŷs), the read-backs and the refusals, switches to the default model (smaller arrays, the
// buffers are reused) and destroys the handle: the allocations, uploads and read-backs of the new entry points under the
// sanitizers.
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
        if (rc_ != (code)) { printf("%s -> %d, expected %d\n", #call, rc_, (code)); return 1; } \
    } while (0)

int main() {
    const int B = 5, nx = 6, nu = 2, ny = 3, nym = 2, nxs = 4, Hp = 4;         // B = 5: a tail group of one member
    mpcqp_dims dims{};
    dims.batch = B; dims.nxhat = nx; dims.nu = nu; dims.ny = ny; dims.nd = 0; dims.Hp = Hp; dims.Hc = 1; dims.neps = 1;
    mpcqp_handle h = nullptr;
    CHECK(mpcqp_create(&dims, &h));
    std::vector<double> A(B * nx * nx, 0.0), Bu(B * nx * nu, 0.0), C(B * ny * nx, 0.0), dop(B * nx, 0.25);
    std::vector<double> As(B * nxs * nxs, 0.0), Bs(B * nxs * nym, 0.0), Cs(B * nym * nxs, 0.0), Ds(B * nym * nym, 0.0);
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < nx; ++i) {
            A[b * nx * nx + i + nx * i] = 0.9 - 0.05 * b;
            if (i + 1 < nx) A[b * nx * nx + i + nx * (i + 1)] = 0.1;
            for (int c = 0; c < nu; ++c) Bu[b * nx * nu + i + nx * c] = 0.1 * (i + c + 1);
            for (int a = 0; a < ny; ++a) C[b * ny * nx + a + ny * i] = std::sin(1.0 + a + 2.0 * i + b);
        }
        for (int i = 0; i < nxs; ++i) {
            As[b * nxs * nxs + i + nxs * i] = i == 0 ? 1.0 : 0.8 - 0.1 * i;
            for (int j = 0; j < nym; ++j) {
                Bs[b * nxs * nym + i + nxs * j] = 0.3 * std::cos(1.0 + i + j + b);
                Cs[b * nym * nxs + j + nym * i] = 0.4 * std::sin(2.0 + i - j + b);
            }
        }
        Ds[b * nym * nym + 0] = 1.0; Ds[b * nym * nym + 3] = 1.0; Ds[b * nym * nym + 1] = 0.2;
    }
    for (int i = 0; i < nym * nym; ++i) Ds[3 * nym * nym + i] = 0.0;           // member 3: a singular Ds
    const int32_t i_ym[nym] = {2, 0}, twice[nym] = {1, 1};
    CHECK(mpcqp_set_model(h, A.data(), Bu.data(), C.data(), nullptr, nullptr, dop.data()));
    std::vector<double> x(B * nx, 0.5), y(B * nym, 1.0), u(B * nu, -0.2);
    std::vector<double> xs(B * nxs), ys(B * ny), Yhs(B * ny * Hp), Bv(B * ny * Hp);
    std::vector<int32_t> st(B, -1), ist(B, -1);
    EXPECT(mpcqp_im_correct(h, x.data(), y.data(), nullptr), MPCQP_ERR_ORDER);
    EXPECT(mpcqp_get(h, MPCQP_GET_IM_XS, xs.data()), MPCQP_ERR_ORDER);
    CHECK(mpcqp_im_set(h, nxs, As.data(), Bs.data(), Cs.data(), Ds.data(), i_ym, nym));
    CHECK(mpcqp_im_status(h, st.data()));
    for (int b = 0; b < B; ++b)
        if (st[b] != (b == 3 ? 2 : 0)) { printf("status[%d] = %d\n", b, st[b]); return 1; }
    y[1 * nym + 1] = NAN;                                                       // a missing measurement of member 1
    for (int k = 0; k < 3; ++k) {
        CHECK(mpcqp_im_correct(h, x.data(), y.data(), nullptr));
        CHECK(mpcqp_im_update(h, x.data(), u.data(), nullptr));
    }
    CHECK(mpcqp_im_correct(h, x.data(), y.data(), nullptr));
    // refusals leave the state alone
    EXPECT(mpcqp_im_set(h, nxs, As.data(), Bs.data(), Cs.data(), Ds.data(), twice, nym), MPCQP_ERR_ARG);
    EXPECT(mpcqp_im_set(h, nxs, As.data(), Bs.data(), Cs.data(), Ds.data(), i_ym, ny + 1), MPCQP_ERR_DIMS);
    EXPECT(mpcqp_im_set(h, nxs, As.data(), nullptr, Cs.data(), Ds.data(), i_ym, nym), MPCQP_ERR_ARG);
    EXPECT(mpcqp_kf_set_direct(h, 0), MPCQP_ERR_ARG);
    EXPECT(mpcqp_explicit_prepare(h, 0), MPCQP_ERR_UNSUPPORTED);
    CHECK(mpcqp_get(h, MPCQP_GET_IM_XS, xs.data()));
    CHECK(mpcqp_get(h, MPCQP_GET_IM_YS, ys.data()));
    CHECK(mpcqp_get(h, MPCQP_GET_IM_YHATS, Yhs.data()));
    double big = 0.0;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < ny * Hp; ++i) {
            const double v = Yhs[b * ny * Hp + i];
            if (!std::isfinite(v) || (b == 3 && v != 0.0)) { printf("Yhs[%d][%d] = %g\n", b, i, v); return 1; }
            big = std::fmax(big, std::fabs(v));
        }
    if (!(big > 1e-3) || ys[1 * ny + 0] != 0.0 || ys[1 * ny + 1] != 0.0 || !(ys[1 * ny + 2] != 0.0)) {     // i_ym = {2, 0}: y0m[1] is output 0
        printf("max |Yhs| %g, ys of member 1: %g %g %g\n", big, ys[ny], ys[ny + 1], ys[ny + 2]);
        return 1;
    }
    for (auto& v : A) v *= 0.5;
    CHECK(mpcqp_set_model(h, A.data(), Bu.data(), C.data(), nullptr, nullptr, dop.data()));
    CHECK(mpcqp_get(h, MPCQP_GET_BVEC, Bv.data()));
    y[1 * nym + 1] = 1.0;
    CHECK(mpcqp_est_initstate(h, x.data(), u.data(), y.data(), nullptr, ist.data()));
    for (int b = 0; b < B; ++b)
        if (ist[b] != 0 || !std::isfinite(x[b * nx])) { printf("initstate status[%d] = %d\n", b, ist[b]); return 1; }
    CHECK(mpcqp_im_set(h, 0, nullptr, nullptr, nullptr, nullptr, i_ym, nym));   // the default model: nxs = nym
    xs.assign(B * nym, -1.0);
    CHECK(mpcqp_get(h, MPCQP_GET_IM_XS, xs.data()));
    for (double v : xs)
        if (v != 0.0) { printf("x̂s after the set-up: %g\n", v); return 1; }
    CHECK(mpcqp_im_correct(h, x.data(), y.data(), nullptr));
    CHECK(mpcqp_im_update(h, x.data(), u.data(), nullptr));
    CHECK(mpcqp_destroy(h));
    printf("im asan ok (max |Yhs| %.3f)\n", big);
    return 0;
}
