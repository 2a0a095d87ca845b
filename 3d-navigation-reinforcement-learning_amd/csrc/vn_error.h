// vn_error.h -- error reporting across the C-ABI: negative VN_ERR_* codes
// plus a thread-local message returned by vn_last_error().  Plain C++ (no HIP
// include), so the host-only planning code (env_plan.h) can report errors
// too; vn_common.h includes it, and the inline definitions below are the one
// copy for the whole library.
#pragma once

#include <cstdarg>
#include <cstdio>
#include <string>

#include "voxnav.h"

namespace vn_detail {

inline thread_local std::string g_last_error;

inline int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

}  // namespace vn_detail
