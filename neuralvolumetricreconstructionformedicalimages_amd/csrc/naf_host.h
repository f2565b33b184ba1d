// naf_host.h -- host-side helpers shared by the translation units of libnaf_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/naf_hip.h"

namespace naf {

// Records `msg` as the calling thread's last error and returns `code` (see naf_last_error()).
int fail(int code, const char *msg);
// The same for a refused argument, NAF_ERR_INVALID_ARGUMENT, with the message "<who>: <what>".
int fail_who(const char *who, const char *what);
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

}  // namespace naf
