// The host scaffold of a side library (libvmlmf_beam.so, libvmlmf_decode.so, libvmlmf_score.so: one translation unit each, so what
// is static here is the library's own): the calling thread's error text, fail(), the tail of a launch, and the two exports every
// side library has, <prefix>_abi_version and <prefix>_last_error.  Host code only - nothing here is compiled for the device.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace vmlmf_side {

static thread_local std::string g_error;
// the text is what <prefix>_last_error() returns to this thread until its next failure
static int fail(int code, const std::string& msg) {
  g_error = msg;
  return code;
}
// behind a launch: 0, or HIP's error as the code and "<what>: <HIP's text>"
static int launch_tail(const char* what) {
  const hipError_t rc = hipGetLastError();
  return rc == hipSuccess ? 0 : fail((int)rc, std::string(what) + ": " + hipGetErrorString(rc));
}

}  // namespace vmlmf_side

#define VMLMF_SIDE_LIBRARY(prefix, version)                     \
  extern "C" int prefix##_abi_version(void) { return version; } \
  extern "C" const char* prefix##_last_error(void) { return vmlmf_side::g_error.c_str(); }
