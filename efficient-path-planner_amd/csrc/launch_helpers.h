// launch_helpers.h — the host-side launch helpers every device file uses, defined once in
// runtime.cpp: the device's CU count, the persistent grid size, integer test-hook variables
// and the launch status.
#pragma once
#include <cstdint>

#include "epp_internal.h"

namespace epp {

constexpr int kBlock = 256;
constexpr uint32_t kLdsBudget = 150 * 1024;

// the current device's CU count (asked once per device; 256 when it cannot be asked)
int cu_count();

// integer environment variable (test hooks only)
int env_int(const char* name, int dflt);

// Persistent grid: at most `per_cu` resident 256-thread blocks per CU (LDS permitting),
// each looping over item groups, so the world is staged into LDS once per block.
int grid_for(int64_t groups, uint32_t lds_bytes);

// hipGetLastError as a status (sets the error text)
epp_status launch_error(const char* what);

}  // namespace epp
