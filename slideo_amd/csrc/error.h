// error.h — the one error type of the host runtime: a code of include/slideo_amd.h and a message.  Plain C++ (no HIP include), so
// that host-only headers (frame_settings.h) and their stand-alone checks can fail the way the library does.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>

#include "slideo_amd.h"

namespace slideo {

struct Error : std::runtime_error {
    int32_t code;
    Error(int32_t c, const std::string& m) : std::runtime_error(m), code(c) {}
};

[[noreturn]] inline void fail(int32_t code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    throw Error(code, buf);
}

}  // namespace slideo
