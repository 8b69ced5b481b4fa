// What the C ABI's HIP sources (handle.hip, begin.hip, sequence.hip,
// validate_api.hip) share: the thread's last error (host_api.hpp), HIP error
// checking and a scratch allocator for the entry points that use no handle.
// Internal to the library.
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <vector>

#include "host_api.hpp"

namespace mpcmmd {

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define HIPC(x)                                                                                     \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess)                                                                           \
      throw ::mpcmmd::HipError(std::string(#x) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + ":" + \
                               std::to_string(__LINE__) + ")");                                     \
  } while (0)

template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const HipError& e) {
    return fail(MPCMMD_E_HIP, e.what());
  } catch (const std::invalid_argument& e) {
    return fail(MPCMMD_E_INVALID, e.what());
  } catch (const std::exception& e) {
    return fail(MPCMMD_E_INVALID, e.what());
  }
}

// device buffers of one call, freed when it returns or throws
struct Scratch {
  std::vector<void*> bufs;
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() {
    for (void* d : bufs) (void)hipFree(d);
  }
  // `bytes` of device memory, filled from src unless it is null
  void* up(const void* src, size_t bytes) {
    void* d = nullptr;
    HIPC(hipMalloc(&d, bytes));
    bufs.push_back(d);
    if (src) HIPC(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
    return d;
  }
};

}  // namespace mpcmmd
