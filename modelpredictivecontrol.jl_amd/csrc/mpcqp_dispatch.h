// mpcqp_dispatch.h -- ahead-of-time specialisations of the step kernel (compile-time dims).
// X(NU, NY, NXH, HP, HC, NEPS, GMASK): any handle whose dimensions, constraint-group pattern
// (Dims::gmask) and default move blocking match one entry runs the specialised kernel; every
// other handle runs the generic runtime-dims kernel (same source, same numerics).
//   C2 = BASELINE.json configs[1]: hard u and Δu box      -> groups box-lo, box-hi, Umin, Umax
//   C3 = BASELINE.json configs[2..3]: hard u, soft ymax    -> groups Umin, Umax, Ymax (the row ϵ >= 0 rides in Ymax: eps_host_group)
#pragma once
#define MPCQP_SPECIALIZATIONS(X)        \
    X(2, 2, 6, 20, 5, 1, 0x0Fu)         \
    X(4, 4, 16, 30, 10, 1, 0x8Cu)

// One visit of the list per library:  template <class F> static bool first_aot(F&& f) { MPCQP_SPECIALIZATIONS(MPCQP_AOT_TRY)
// return false; }  calls f(AotEntry<SD>{}) with the StaticDims types of the entries in order and stops at the first call that
// returns true.  MPCQP_AOT_TRY_NB: an entry for any move-blocking vector (the CPU emulator's extra shapes).
namespace mpcqp {
template <class SD> struct AotEntry { using type = SD; };
}
#define MPCQP_AOT_TRY(...) if (f(mpcqp::AotEntry<mpcqp::StaticDims<__VA_ARGS__, 1>>{})) return true;
#define MPCQP_AOT_TRY_NB(...) if (f(mpcqp::AotEntry<mpcqp::StaticDims<__VA_ARGS__, 0>>{})) return true;
