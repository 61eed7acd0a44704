// device_scope.h -- flex::DeviceScope, the one scoped device switch of both libraries (plan.h includes it; axw.cpp includes it alone).
#pragma once
#include <hip/hip_runtime.h>

namespace flex {

// `dev` is the current device for the length of a scope: one hipGetDevice, a hipSetDevice only when the device differs, and the
// caller's device set back on exit only then.  error(): the get or set failed (the scope then changed nothing).
class DeviceScope {
  public:
    explicit DeviceScope(int dev) {
        err_ = hipGetDevice(&prev_);
        if (err_ == hipSuccess && prev_ != dev) {
            err_ = hipSetDevice(dev);
            switched_ = err_ == hipSuccess;
        }
    }
    ~DeviceScope() { if (switched_) (void)hipSetDevice(prev_); }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
    hipError_t error() const { return err_; }

  private:
    int prev_ = -1;
    bool switched_ = false;
    hipError_t err_ = hipSuccess;
};

}  // namespace flex
