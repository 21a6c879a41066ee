// wtp_device_scope.hpp — "make a device current, do something, restore the caller's device"
// for the host-side units (wtp_host.cpp, wtp_group.cpp).  Internal, and on its own: nothing
// else of csrc/ is needed to use it.
#pragma once
#include <hip/hip_runtime.h>

namespace wtp {

// Records the current device; its destructor makes that device current again, so no exit of
// the enclosing block can leave another one behind.  ok() tells whether the record and the
// latest use() worked; a scope that recorded nothing restores nothing.  Hidden: the libraries
// that use it export their C-ABI and nothing of this.
class __attribute__((visibility("hidden"))) DeviceScope {
    int prev_ = 0;
    const bool saved_;
    bool ok_;

  public:
    DeviceScope() : saved_(hipGetDevice(&prev_) == hipSuccess), ok_(saved_) {}
    explicit DeviceScope(int d) : DeviceScope() { use(d); }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
    ~DeviceScope() {
        if (saved_) (void)hipSetDevice(prev_);
    }
    bool use(int d) { return ok_ = saved_ && hipSetDevice(d) == hipSuccess; }
    bool ok() const { return ok_; }
};

}  // namespace wtp
