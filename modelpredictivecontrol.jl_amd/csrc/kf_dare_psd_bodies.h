// kf_dare_psd_bodies.h -- the second pass of the steady-state Riccati solve by name: kf_dare_psd_body is the square-root
// form of the one doubling body of kf_dare_bodies.h, where the iteration, the convergence condition, the second-pass rules
// and the zeroing are described.  Included by the units that build the second-pass kernels (kf_kernels.hip,
// tests/emu/emu_kf_dare_psd.cpp).
#pragma once
#include "kf_dare_bodies.h"

namespace mpcqp {
namespace kf {

template <class W, int NX>
MPCQP_HD void kf_dare_psd_body(W& w, const DareArgs& a, int wave_id) { kf_dare_body<W, NX, true>(w, a, wave_id); }

}  // namespace kf
}  // namespace mpcqp
