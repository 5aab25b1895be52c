// vrc_host.h -- the error plumbing the host-side translation units share on top of vrc_internal.h.
#pragma once
#include "vrc_internal.h"

namespace vrc {
// a failed HIP call as the library's error "<what>: <HIP's text>"; out of memory has a code of its own
inline int fail_hip(hipError_t e, const char* what)
{
    return fail(e == hipErrorOutOfMemory ? VRC_ERR_OOM : VRC_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}
}  // namespace vrc
using vrc::fail;

// the C ABI of vrc_api.cpp / vrc_renderer.cpp / vrc_ipc.cpp reports every failed call as VRC_ERR_HIP
#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) return fail(VRC_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
