// error.hpp -- the thread-local error message behind dllm_last_error() (plain C++: usable without HIP).
#pragma once

#include <string>

namespace dllm {

void set_error(const std::string &msg);
// Sets the message and returns `code`: `return fail(DLLM_ERR_..., "...")`.
int fail(int code, const std::string &msg);

}  // namespace dllm
