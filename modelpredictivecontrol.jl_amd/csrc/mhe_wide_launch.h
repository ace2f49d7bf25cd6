// mhe_wide_launch.h -- host-side launch entry points of the wide kernels (mhe_wide_kernels.hip: one estimator per
// wavefront, 16 < max(nx̂, nym) <= 32).  WEAK declarations: a library linked without that unit (the stock CPU emulator
// tests/emu/libmpcqp_emu.so, which defines the entry points of mhe_launch.h only; libmpcqp_emu_est.so has the wide ones of
// tests/emu/emu_mhe_wide.cpp) still links, and mpcqp_mhe_create refuses the dimensions these kernels would serve
// (wide_available()).
#pragma once
#include <hip/hip_runtime.h>

#include "mhe_types.h"

namespace mpcqp {
namespace mhe {
__attribute__((weak)) hipError_t launch_wide_setup(const Dims& d, const Raw& in, double* cst, hipStream_t st);
__attribute__((weak)) hipError_t launch_wide_cov(const Dims& d, const Args& a, int mode, const double* P0, double* Pout, hipStream_t st);
__attribute__((weak)) hipError_t launch_wide_step(const Dims& d, const Args& a, hipStream_t st);
__attribute__((weak)) int wide_waves_for(int device, int B, int NX);      // size of the persistent grid (LDS-bound)
inline bool wide_available() { return launch_wide_setup && launch_wide_cov && launch_wide_step && wide_waves_for; }
// register columns of a handle: a multiple of four up to 16 (one DPP row per estimator), of eight above (24, 32: wide)
inline int register_columns_for(int nmax) { return nmax <= RL ? 4 * ((nmax + 3) / 4) : 8 * ((nmax + 7) / 8); }
}  // namespace mhe
}  // namespace mpcqp
