// common.hpp -- error plumbing shared by the C-ABI entry points, and the workspace arena every carve uses.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/ldpc_amd.h"

namespace ldpc {

void set_error(const std::string &msg);

inline int fail(int code, const std::string &msg) {
    set_error(msg);
    return code;
}

// Workspace arena: a call's buffers lie in one caller allocation in the order they are taken, each
// size rounded up to `align` bytes, so a buffer that is left out or taken with 0 bytes moves nothing
// but what follows it.  base may be null (sizing): every pointer is then null and bytes still counts.
struct Arena {
    char *base;
    int64_t bytes = 0;
    explicit Arena(void *b) : base(static_cast<char *>(b)) {}
    template <typename T>
    T *take(int64_t n, int64_t align = 256) {
        T *q = base ? reinterpret_cast<T *>(base + bytes) : nullptr;
        bytes += (n + align - 1) / align * align;
        return q;
    }
};

}  // namespace ldpc

#define LDPC_HIP(call)                                                                        \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return ::ldpc::fail(LDPC_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define LDPC_CHECK_LAUNCH(what)                                                                  \
    do {                                                                                         \
        hipError_t e_ = hipGetLastError();                                                       \
        if (e_ != hipSuccess)                                                                    \
            return ::ldpc::fail(LDPC_EHIP, std::string(what) + " launch: " + hipGetErrorString(e_)); \
    } while (0)
