// The library's error state as every translation unit sees it: the text bd_last_error() returns is kept per thread in
// engine.hip, and an entry point that refuses a call or meets a HIP error leaves its message there through these.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/buzzdetect_hip.h"

namespace bd {

void set_error(const std::string& msg);     // engine.hip: the text bd_last_error() returns on this thread

inline int fail(int code, const std::string& msg) {
    set_error(msg);
    return code;
}

// What the launches of entry point `fn` ("bd_x: ") left behind: BD_OK, or BD_EHIP with the runtime's text behind fn
inline int hip_result(const std::string& fn) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return BD_OK;
    return fail(BD_EHIP, fn + hipGetErrorString(e));
}

}  // namespace bd

#define BD_HIP(expr)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return bd::fail(BD_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)
