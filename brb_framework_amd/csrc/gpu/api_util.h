// api_util.h -- the per-thread runtime (api_runtime.hip) as the C-ABI translation units use it
// (batch_api.hip, host_pipe.hip, transform_batcher.hip): error reporting, device selection, the
// device workspace and the call's wave-pair fault word.  The message is per thread and read by
// BRB_CryptoGPU_LastError().
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace brb_api {

extern thread_local std::string t_err;
void clear_err();
void set_err(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
int fail_hip(const char *what, hipError_t e);   // sets the message, returns BRB_BATCH_NOT_DONE
int device_ok();                                // BRB_BATCH_OK if a HIP device is visible
int device_count();                             // visible HIP devices (probed once per process), 0 if none
void release_thread_resources();                // the calling thread's workspaces, streams and events

// The calling thread's grow-only device scratch on its current device, at least `bytes` long
// (nullptr and *err on failure).  A call that uses it drains its streams before it returns.
void *workspace(size_t bytes, hipError_t *err);

inline size_t align_up(size_t x, size_t a)
{
    return (x + a - 1) / a * a;
}

// Arms the thread's fault word for one synchronous call (pair_fault.h); check() after the stream
// has drained turns a fault into BRB_BATCH_FAULT.  A device-mode async call returns before its
// kernels run: it arms the thread's sticky async word instead, which BRB_CryptoGPU_AsyncFaultCheck
// reads (and clears) once the caller has synchronised its streams.  ready() before the launch:
// BRB_BATCH_OK, or the call's error when the thread's word could not be allocated -- no call, a
// captured one least of all, is launched with no word to report into.
struct PairFault {
    uint32_t *w = nullptr;
    explicit PairFault(unsigned flags);
    ~PairFault();
    int ready() const;
    PairFault(const PairFault &) = delete;
    PairFault &operator=(const PairFault &) = delete;
    int check(int rc) const;
};

// Makes `dev` the calling thread's current HIP device for one scope and restores the caller's
// device on exit: every batch call runs on the caller's current device, so library code that
// switches devices (a batcher created on another GPU, an all-devices split) must switch back.
class DeviceGuard {
public:
    explicit DeviceGuard(int dev)
    {
        int cur = -1;
        if ((err_ = hipGetDevice(&cur)) != hipSuccess)
            return;
        if (cur != dev) {
            if ((err_ = hipSetDevice(dev)) != hipSuccess)
                return;
            prev_ = cur;
        }
    }
    ~DeviceGuard()
    {
        if (prev_ >= 0)
            (void)hipSetDevice(prev_);
    }
    hipError_t error() const { return err_; }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;

private:
    int prev_ = -1;
    hipError_t err_ = hipSuccess;
};

}  // namespace brb_api
