// naf_host.h -- host-side helpers shared by the translation units of libnaf_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/naf_hip.h"

namespace naf {

// Records `msg` as the calling thread's last error and returns `code` (see naf_last_error()).
int fail(int code, const char *msg);
// The one refusal "<who>: <what>"; returns `code`.
int fail_who(const char *who, const char *what, int code = NAF_ERR_INVALID_ARGUMENT);
// "<who>: workspace too small (<bytes> bytes, need <need>)" and "<who>: <what> must be <bytes>-byte aligned", both
// NAF_ERR_INVALID_ARGUMENT.  There is no combined workspace check: the entry points test null, size and alignment in different
// orders, and each keeps its own.
int workspace_too_small(const char *who, uint64_t bytes, uint64_t need);
int misaligned(const char *who, const char *what, uint32_t bytes);
// True when `a` has none of the low bits in `mask` set (a null pointer has none).
inline bool aligned(const void *a, uintptr_t mask) { return (((uintptr_t)a) & mask) == 0; }
// hipGetLastError() -> NAF_OK / NAF_ERR_LAUNCH (message names the kernel).
int check_launch(const char *kernel);

// Raise a kernel's dynamic-LDS limit.  The attribute is per device and the call is a cheap host-side table update, so it
// is simply made before every launch of a kernel that may need more than the default: no cached flag to go stale when the
// same process drives a second GPU or a second thread (the ABI takes a stream per call and keeps no state of its own).
template <typename K>
static int raise_lds_limit(K kernel, uint32_t bytes, const char *who) {
    if (hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
        return fail(NAF_ERR_LAUNCH, who);
    return NAF_OK;
}

// Optional per-kernel timing (naf_profile_enable / naf_profile_collect): a pair of HIP events on the launch stream
// around every kernel, so bench.py can time one kernel inside the real pipeline.  Costs nothing when disabled.
class ProfScope {
   public:
    ProfScope(const char *kernel, hipStream_t stream);
    ~ProfScope();
    ProfScope(const ProfScope &) = delete;
    ProfScope &operator=(const ProfScope &) = delete;

   private:
    int slot_;
    hipStream_t stream_;
};

// One launch under two names: times `kernel` under `timed` when profiling is on (the aggregate name bench.py's per-kernel table reads:
// mlp_forward_kernel for every forward instantiation, a level's own name on the per-level diagnostic path), launches it, and reports a
// failed launch under `name`, the kernel's own.
template <typename K, typename... Args>
static int launch_as(const char *timed, const char *name, K kernel, dim3 grid, dim3 block, uint32_t lds_bytes, hipStream_t stream, Args... args) {
    { ProfScope prof_(timed, stream);
      hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...); }
    return check_launch(name);
}
// One launch, timed and reported under the same name.  A site that picks one of several instantiations under one name calls this once
// per branch, or picks the kernel first.
template <typename K, typename... Args>
static int launch(const char *name, K kernel, dim3 grid, dim3 block, uint32_t lds_bytes, hipStream_t stream, Args... args) {
    return launch_as(name, name, kernel, grid, block, lds_bytes, stream, args...);
}

}  // namespace naf
