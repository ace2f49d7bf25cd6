// spec_cache.h -- the cache of on-demand step-kernel objects (spec_cache.cpp): host-only C++, no HIP.
// An object exports mpcqp_spec_matches / _matches_dims / _launch_step / _launch_hessian (csrc/mpcqp_spec.hip); the
// launchers take the stream as void* and return the hipError_t as int.
#pragma once
#include <string>

#include "mpcqp_types.h"

namespace mpcqp {
// entry points of a loaded object, handed out BY VALUE (reject_spec may empty the cache's own entry at any time)
struct SpecEntry {
    int (*matches)(const Dims*) = nullptr;
    int (*matches_dims)(const Dims*) = nullptr;
    int (*step)(const Dims*, const Model*, const StepIO*, void*) = nullptr;      // null: no object
    int (*hessian)(const Dims*, const Model*, void*) = nullptr;
    bool verified = false;        // compared with the runtime-dimension kernel on this machine (marker <object>.ok)
    bool no_marker = false;       // the marker was looked for and not found: steps do not stat() again (mpcqp_prepare does)
};
bool force_generic();                       // MPCQP_FORCE_GENERIC=1 (read once): runtime-dimension kernels only
bool spec_enabled(const Dims& d);           // on-demand kernels are on (MPCQP_JIT) and `d` is within their limit
// Both load from the cache and never compile; a miss is remembered, so a later call does no file-system work.
SpecEntry spec_find(const Dims& d);             // loaded, verified or not
SpecEntry spec_find_verified(const Dims& d);    // what a STEP may run: loaded AND verified
void spec_forget_miss(const Dims& d);           // mpcqp_prepare: look (and load) again at the next spec_find
// compile the specialisation of `d` into the cache unless it is there already; 0 = present afterwards (no load)
int spec_build(const Dims& d, std::string* path_out, std::string* err);
// one-time check of an on-demand kernel against the runtime-dimension kernel (see mpcqp_prepare)
bool spec_verified(const Dims& d);
bool spec_present(const Dims& d);      // an on-demand object of this shape is loaded / loadable (verified or not)
void mark_spec_verified(const Dims& d);
void reject_spec(const Dims& d);
}  // namespace mpcqp
