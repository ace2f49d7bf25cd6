// TEST INFRASTRUCTURE ONLY (tests/test_c2d.py): a stand-alone program around csrc/mpcqp_host.hip compiled for the host with
// -fsanitize=address,undefined and linked with the CPU emulator objects.  It discretises a batch of diagonal continuous-time
// models with a measured disturbance and integrators (both d_methods), checks Φ = exp(λ Ts) and the shape of the augmented
// model, runs the handle path (host-synchronous and on a stream) with one refused member, reads the model back, walks through
// the refusals and destroys the handle: the allocations, uploads, launches and read-backs of the new entry points under the
// sanitizers.
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
#define REQUIRE(cond)                                                               \
    do {                                                                            \
        if (!(cond)) { printf("%s failed (line %d)\n", #cond, __LINE__); return 1; } \
    } while (0)

int main() {
    const int B = 4, nx = 3, nu = 2, ny = 2, nd = 1;
    const int32_t nint_u[nu] = {1, 0}, nint_ym[ny] = {2, 1}, i_ym[ny] = {1, 0};
    std::vector<double> A(B * nx * nx, 0.0), Bu(B * nx * nu), C(B * ny * nx), Bd(B * nx * nd), Dd(B * ny * nd), Ts(B), dop;
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < nx; ++i) A[b * nx * nx + i + nx * i] = -0.2 * (i + 1) - 0.1 * b;
        Ts[b] = 0.5 + b;
    }
    for (size_t i = 0; i < Bu.size(); ++i) Bu[i] = 0.1 * (double)(i % 7) - 0.2;
    for (size_t i = 0; i < C.size(); ++i) C[i] = 0.3 * (double)(i % 5) - 0.5;
    for (size_t i = 0; i < Bd.size(); ++i) Bd[i] = 0.2 + 0.1 * (double)(i % 3);
    for (size_t i = 0; i < Dd.size(); ++i) Dd[i] = 0.05 * (double)i;

    for (int method : {MPCQP_C2D_TUSTIN, MPCQP_C2D_ZOH}) {
        mpcqp_c2d_spec spec{B, nx, nu, ny, nd, ny, method, nint_u, nint_ym, i_ym};
        int32_t nxd = 0, nxh = 0;
        CHECK(mpcqp_c2d_sizes(&spec, &nxd, &nxh));
        REQUIRE(nxd == (method == MPCQP_C2D_TUSTIN ? 2 * nx : nx) && nxh == nxd + 4);
        dop.assign((size_t)B * nxd, 0.25);
        std::vector<double> Ah((size_t)B * nxh * nxh, 9.0), Bh((size_t)B * nxh * nu, 9.0), Ch((size_t)B * ny * nxh, 9.0),
            Bdh((size_t)B * nxh * nd, 9.0), Ddh((size_t)B * ny * nd, 9.0), doph((size_t)B * nxh, 9.0);
        std::vector<int32_t> st(B, -1);
        std::vector<double> Tb = Ts;
        Tb[2] = -1.0;                               // member 2 is refused: nothing of it is written
        mpcqp_c2d_in in{A.data(), Bu.data(), C.data(), Bd.data(), Dd.data(), Tb.data(), dop.data()};
        mpcqp_c2d_out out{Ah.data(), Bh.data(), Ch.data(), Bdh.data(), Ddh.data(), doph.data()};
        CHECK(mpcqp_c2d(&spec, &in, &out, st.data()));
        for (int b = 0; b < B; ++b) {
            REQUIRE(st[b] == (b == 2 ? 2 : 0));
            const double* Ab = &Ah[(size_t)b * nxh * nxh];
            if (b == 2) {
                REQUIRE(Ab[0] == 9.0 && doph[(size_t)b * nxh] == 9.0);
                continue;
            }
            for (int i = 0; i < nx; ++i)
                REQUIRE(std::fabs(Ab[i + nxh * i] - std::exp(A[b * nx * nx + i + nx * i] * Ts[b])) <= 1e-14);
            REQUIRE(Ab[(nxh - 1) + nxh * (nxh - 1)] == 1.0 && Ab[(nxh - 2) + nxh * (nxh - 3)] == 1.0);   // As: the chain of two
            REQUIRE(Ab[0 + nxh * nxd] == Bh[(size_t)b * nxh * nu] + 0.0);                               // Bu Cs_u: column of input 0
            REQUIRE(Ch[(size_t)b * ny * nxh + 1 + ny * (nxd + 2)] == 1.0);                              // Cs_y: ym 0 is output 1
            REQUIRE(doph[(size_t)b * nxh] == 0.25 && doph[(size_t)b * nxh + nxh - 1] == 0.0);
        }

        // the handle path
        mpcqp_dims dims{};
        dims.batch = B; dims.nxhat = nxh; dims.nu = nu; dims.ny = ny; dims.nd = nd; dims.Hp = 4; dims.Hc = 2; dims.neps = 1;
        mpcqp_handle h = nullptr;
        CHECK(mpcqp_create(&dims, &h));
        mpcqp_sizes sz{};
        CHECK(mpcqp_get_sizes(h, &sz));
        std::vector<double> M((size_t)B * sz.nY, 1.0), N((size_t)B * sz.nDU, 0.1), L((size_t)B * sz.nU, 0.0), Cw(B, 1e5);
        CHECK(mpcqp_set_weights(h, M.data(), N.data(), L.data(), Cw.data()));
        std::vector<double> back((size_t)B * nxh * nxh);
        EXPECT(mpcqp_get(h, MPCQP_GET_MODEL_AHAT, back.data()), MPCQP_ERR_ORDER);
        CHECK(mpcqp_set_model_continuous(h, &spec, &in, st.data()));
        REQUIRE(st[2] == 2 && st[0] == 0);
        CHECK(mpcqp_get(h, MPCQP_GET_MODEL_AHAT, back.data()));
        for (size_t i = 0; i < back.size(); ++i) {
            const bool refused = i / ((size_t)nxh * nxh) == 2;
            REQUIRE(back[i] == (refused ? 0.0 : Ah[i]));
        }
        in.Ts = Ts.data();
        in.dop = nullptr;
        CHECK(mpcqp_set_model_continuous_device(h, &spec, &in, st.data(), nullptr));       // (the emulator: host = device)
        REQUIRE(st[2] == 0);
        std::vector<double> H((size_t)B * sz.nZ * sz.nZ), dopb((size_t)B * nxh, 1.0);
        CHECK(mpcqp_get(h, MPCQP_GET_HESSIAN, H.data()));
        CHECK(mpcqp_get(h, MPCQP_GET_MODEL_DOP, dopb.data()));
        REQUIRE(H[0] > 0.0 && dopb[0] == 0.0);
        // refusals: the handle keeps what it had
        mpcqp_c2d_spec other = spec;
        other.nint_u = nullptr;
        EXPECT(mpcqp_set_model_continuous(h, &other, &in, st.data()), MPCQP_ERR_ARG);
        other = spec; other.d_method = 7;
        EXPECT(mpcqp_set_model_continuous(h, &other, &in, st.data()), MPCQP_ERR_ARG);
        other = spec; other.nym = ny + 1;
        EXPECT(mpcqp_set_model_continuous(h, &other, &in, st.data()), MPCQP_ERR_DIMS);
        EXPECT(mpcqp_set_model_continuous(h, &spec, nullptr, st.data()), MPCQP_ERR_NULL);
        mpcqp_c2d_in miss = in;
        miss.Bd = nullptr;
        EXPECT(mpcqp_set_model_continuous(h, &spec, &miss, st.data()), MPCQP_ERR_NULL);
        EXPECT(mpcqp_c2d(&spec, &miss, &out, st.data()), MPCQP_ERR_NULL);
        std::vector<double> H2(H.size());
        CHECK(mpcqp_get(h, MPCQP_GET_HESSIAN, H2.data()));
        REQUIRE(H2 == H);
        CHECK(mpcqp_destroy(h));
    }
    // beyond the limits
    const int32_t many[1] = {62};
    mpcqp_c2d_spec big{1, 2, 1, 1, 0, 1, MPCQP_C2D_TUSTIN, nullptr, many, nullptr};
    int32_t nxd = 0, nxh = 0;
    CHECK(mpcqp_c2d_sizes(&big, &nxd, &nxh));
    REQUIRE(nxh == 64);
    const int32_t more[1] = {63};
    big.nint_ym = more;
    EXPECT(mpcqp_c2d_sizes(&big, &nxd, &nxh), MPCQP_ERR_UNSUPPORTED);
    printf("c2d asan ok\n");
    return 0;
}
