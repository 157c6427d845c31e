// Error reporting of libsem_hip.so, for units that include no HIP header
// (sem_plan.cpp) as well as those that do (through sem_internal.h).
#pragma once
#include <string>

namespace sem {

// thread-local error message behind sem_last_error()
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);

}  // namespace sem
