// mhe_dispatch.h -- the one switch over the register columns NX of the estimator launchers: the device units
// (mhe_kernels.hip, mhe_wide_kernels.hip, kf_kernels.hip) and the CPU emulator's launchers (tests/emu/emu_rowwave.h)
// include it.  A header of its own next to mhe_types.h, which stays plain data without <hip/hip_runtime.h>.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "mhe_types.h"

namespace mpcqp {
namespace mhe {

// f(Cols<NX>) for the register columns of a handle: 4 ... 16 (NX_NARROW: 16 lanes per estimator), 24 and 32 (NX_WIDE: 64);
// any other value is hipErrorInvalidValue and f is not instantiated for it.  On the device (C++17) f takes `auto nx` and
// reads decltype(nx)::value; in the emulator f may be []<int NX>(Cols<NX>).
enum { NX_NARROW = 1, NX_WIDE = 2 };
template <int NX>
using Cols = std::integral_constant<int, NX>;
template <int SETS, class F>
hipError_t dispatch_nx(int NX, F f) {
    bool known = true;
    auto at = [&](auto nx) {
        if constexpr ((SETS & (decltype(nx)::value > RL ? NX_WIDE : NX_NARROW)) != 0) f(nx);
        else known = false;
    };
    switch (NX) {
        case 4: at(Cols<4>{}); break;
        case 8: at(Cols<8>{}); break;
        case 12: at(Cols<12>{}); break;
        case 16: at(Cols<16>{}); break;
        case 24: at(Cols<24>{}); break;
        case 32: at(Cols<32>{}); break;
        default: known = false;
    }
    return known ? hipSuccess : hipErrorInvalidValue;
}

}  // namespace mhe
}  // namespace mpcqp
