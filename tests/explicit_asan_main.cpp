// TEST INFRASTRUCTURE ONLY: stand-alone program (own main) of tests/test_explicit.py::test_host_code_under_sanitizers -- the
// ExplicitMPC entry points of csrc/mpcqp_host.hip, compiled with -fsanitize=address,undefined, on the emulator objects.
#include <cmath>
#include <cstdio>
#include <vector>
#include "../include/mpcqp.h"
#define CHECK(x) do { int rc_ = (x); if (rc_ != 0) { std::printf("%s -> %d\n", #x, rc_); return 1; } } while (0)
int main() {
    const int B = 5, nx = 3, nu = 2, ny = 2, nd = 1, Hp = 7, Hc = 3, n = nu * Hc;
    mpcqp_dims d{};
    d.batch = B; d.nxhat = nx; d.nu = nu; d.ny = ny; d.nd = nd; d.Hp = Hp; d.Hc = Hc; d.neps = 0; d.flags = MPCQP_FLAG_RY_CONSTANT | MPCQP_FLAG_KEEP_QP;
    mpcqp_handle h = nullptr;
    CHECK(mpcqp_create(&d, &h));
    if (mpcqp_explicit_prepare(h, 1) != MPCQP_ERR_ORDER) return 2;
    std::vector<double> A(B * nx * nx), Bu(B * nx * nu), C(B * ny * nx), Bd(B * nx * nd), Dd(B * ny * nd);
    unsigned s = 12345;
    auto rnd = [&] { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (1u << 24) - 0.5; };
    for (auto* v : {&A, &Bu, &C, &Bd, &Dd}) for (auto& x : *v) x = 0.8 * rnd();
    CHECK(mpcqp_set_model(h, A.data(), Bu.data(), C.data(), Bd.data(), Dd.data(), nullptr));
    std::vector<double> M(B * ny * Hp, 1.0), N(B * n, 0.1), L(B * nu * Hp, 0.05);
    for (int i = 0; i < ny * Hp; ++i) M[2 * ny * Hp + i] = 0.0;          // member 2: H = 0 -> status 2
    for (int i = 0; i < n; ++i) N[2 * n + i] = 0.0;
    for (int i = 0; i < nu * Hp; ++i) L[2 * nu * Hp + i] = 0.0;
    CHECK(mpcqp_set_weights(h, M.data(), N.data(), L.data(), nullptr));
    if (mpcqp_explicit_prepare(h, 8) != MPCQP_ERR_ARG) return 3;
    if (mpcqp_explicit_prepare(h, 2) != MPCQP_ERR_ARG) return 3;
    for (int mode : {1, 1}) {      // (the second prepare finds the tables allocated)
        CHECK(mpcqp_explicit_prepare(h, mode));
        std::vector<int32_t> fst(B), st(B), stl(B);
        CHECK(mpcqp_explicit_status(h, fst.data()));
        std::vector<double> x(B * nx), lu(B * nu), ry(B * ny), d0(B * nd), Dh(B * nd * Hp), Z(B * n), u0(B * nu), Y(B * ny * Hp), Zl(B * n), ul(B * nu), ul2(B * nu);
        for (auto* v : {&x, &lu, &ry, &d0}) for (auto& e : *v) e = rnd();
        for (int b = 0; b < B; ++b) for (int t = 0; t < Hp; ++t) Dh[(b * Hp + t) * nd] = d0[b];
        CHECK(mpcqp_explicit_step(h, x.data(), lu.data(), ry.data(), nullptr, d0.data(), Dh.data(), Z.data(), u0.data(), st.data(), Y.data()));
        CHECK(mpcqp_explicit_law(h, x.data(), lu.data(), ry.data(), d0.data(), Zl.data(), ul.data(), stl.data()));
        CHECK(mpcqp_explicit_law(h, x.data(), lu.data(), ry.data(), d0.data(), nullptr, ul2.data(), stl.data()));
        std::vector<double> law((size_t)B * n * (1 + nx + nu + ny + nd)), q(B * n);
        CHECK(mpcqp_get(h, MPCQP_GET_EXPLICIT_LAW, law.data()));
        CHECK(mpcqp_get(h, MPCQP_GET_QTILDE, q.data()));
        for (int b = 0; b < B; ++b) {
            if (fst[b] != (b == 2 ? 2 : 0) || st[b] != fst[b] || stl[b] != fst[b]) return 4;
            for (int i = 0; i < n; ++i) {
                if (b == 2 && (Z[b * n + i] != 0.0 || Zl[b * n + i] != 0.0)) return 5;
                if (!(std::fabs(Z[b * n + i] - Zl[b * n + i]) <= 1e-9 * (1.0 + std::fabs(Z[b * n + i])))) return 6;
            }
            for (int c = 0; c < nu; ++c) if (ul[b * nu + c] != ul2[b * nu + c] || (b == 2 && u0[b * nu + c] != lu[b * nu + c])) return 7;
        }
        CHECK(mpcqp_set_model(h, A.data(), Bu.data(), C.data(), Bd.data(), Dd.data(), nullptr));      // refresh
        CHECK(mpcqp_recondense_device(h, nullptr));
    }
    mpcqp_bounds bd{};
    std::vector<double> um(B * nu * Hp, 1.0);
    bd.U0max = um.data();
    CHECK(mpcqp_set_bounds(h, &bd));
    std::vector<double> x(B * nx), lu(B * nu), ry(B * ny), d0(B * nd), Z(B * n), u0(B * nu);
    std::vector<int32_t> st(B);
    if (mpcqp_explicit_law(h, x.data(), lu.data(), ry.data(), d0.data(), Z.data(), u0.data(), st.data()) != MPCQP_ERR_ORDER) return 8;
    CHECK(mpcqp_set_weights(h, M.data(), N.data(), L.data(), nullptr));      // a setter of the constrained handle: no factor, no error
    if (mpcqp_explicit_status(h, st.data()) != MPCQP_ERR_ORDER) return 9;
    CHECK(mpcqp_destroy(h));
    std::printf("explicit sanitizer run: ok\n");
    return 0;
}
