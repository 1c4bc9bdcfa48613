// error.cpp -- the thread-local error message and dllm_last_error() (no HIP).
#include "error.hpp"

#include "dllm_quant.h"

namespace dllm {

static thread_local std::string g_last_error;

void set_error(const std::string &msg) { g_last_error = msg; }

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

}  // namespace dllm

extern "C" {

const char *dllm_last_error(void) { return dllm::g_last_error.c_str(); }

}  // extern "C"
