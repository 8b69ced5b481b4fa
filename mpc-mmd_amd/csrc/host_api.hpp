// What the C ABI's HIP sources share with its host-only entry points
// (host_api.cpp): the thread's last error and the argument checks that need no
// device.  No HIP; api_common.hpp includes this.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/mpcmmd.h"
#include "solve_host.hpp"

namespace mpcmmd {

// records msg as the calling thread's mpcmmd_last_error and returns code
__attribute__((visibility("hidden"))) int fail(int code, const std::string& msg);

// mpcmmd_create_batch's range checks of the configuration: MPCMMD_OK, or the
// error code with its message recorded
__attribute__((visibility("hidden"))) int check_create_ranges(const mpcmmd_config& c, int32_t max_configs);

PathView view_of(const mpcmmd_path& p);

}  // namespace mpcmmd
