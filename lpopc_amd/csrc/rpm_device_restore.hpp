// rpm_device_restore.hpp — the guard every entry point that changes the calling thread's current device holds.  Host only: the
// runtime's API header and nothing of the engine, so rpm_sweep.cpp can use it without the device side.
#pragma once
#include <hip/hip_runtime_api.h>

namespace rpm {

struct DeviceRestore {   // the calling thread's current device, put back on every exit path
  int prev = -1;
  DeviceRestore() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
  ~DeviceRestore() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace rpm
