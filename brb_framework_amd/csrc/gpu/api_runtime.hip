// api_runtime.hip -- the per-thread runtime behind the batch calls (api_util.h, pair_fault.h): the
// error string, the device probe, the per-thread device workspaces and wave-pair fault words, and the
// exported BRB_CryptoGPU_* runtime calls.  The batch entry points that use it are in batch_api.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "brb_crypto.h"
#include "api_util.h"
#include "fixed_route.h"
#include "host_pipe.h"
#include "pair_fault.h"
#include "test_options.h"

namespace brb_api {

thread_local std::string t_err;

void clear_err()
{
    t_err.clear();
}

void set_err(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    t_err = buf;
}

int fail_hip(const char *what, hipError_t e)
{
    set_err("%s: %s (%d)", what, hipGetErrorString(e), int(e));
    return BRB_BATCH_NOT_DONE;
}

// The device count is cached once a probe has found a device: a batch call from the event loop
// should not pay a runtime query per call, and the set of visible devices does not change while a
// process runs.  A failed probe is not cached (a transient hipGetDeviceCount error must not disable
// the library for the rest of the process): the next call probes again.
namespace {
std::atomic<int> g_count{0};
std::mutex g_count_mu;
}  // namespace

int device_count()
{
    const int n = g_count.load(std::memory_order_acquire);
    if (n > 0)
        return n;
    std::lock_guard<std::mutex> lk(g_count_mu);
    if (g_count.load(std::memory_order_relaxed) > 0)
        return g_count.load(std::memory_order_relaxed);
    int m = 0;
    if (hipGetDeviceCount(&m) != hipSuccess || m < 0)
        m = 0;
    if (m > 0)
        g_count.store(m, std::memory_order_release);
    return m;
}

int device_ok()
{
    if (device_count() > 0)
        return BRB_BATCH_OK;
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess)
        set_err("hipGetDeviceCount: %s (%d)", hipGetErrorString(e), int(e));
    else
        set_err("no HIP device visible to this process");
    (void)hipGetLastError();
    return BRB_BATCH_NOT_DONE;
}

namespace {

// Per-thread, per-device grow-only scratch for host-mode batches.  Freed when the thread exits
// (an event thread that ends returns its HBM) or by BRB_CryptoGPU_ThreadCleanup().
struct Workspaces {
    std::vector<std::pair<void *, size_t>> by_dev;   // (ptr, capacity) per device ordinal
    uint32_t *fault_word = nullptr;                   // pair_fault.h: the thread's fault word
    uint32_t *async_word = nullptr;                   // ... and its sticky word for ASYNC calls
    // Devices on which a device-mode ASYNC call armed async_word (bit d; bit 63 also stands for every
    // device >= 63).  Those calls return before their kernels run, so a pair kernel may still write
    // the word after the thread cleans up: release() first drains these devices.
    uint64_t async_devs = 0;
    void release()
    {
        for (size_t d = 0; d < by_dev.size(); d++)
            if (by_dev[d].first) {
                DeviceGuard g{int(d)};
                (void)hipFree(by_dev[d].first);
                by_dev[d] = {nullptr, 0};
            }
        if (async_word && async_devs) {
            int n = 0;
            if (hipGetDeviceCount(&n) != hipSuccess)
                n = 0;
            for (int d = 0; d < n; d++)
                if (async_devs & (uint64_t(1) << (d < 63 ? d : 63))) {
                    DeviceGuard g{d};
                    if (g.error() == hipSuccess)
                        (void)hipDeviceSynchronize();
                }
            (void)hipGetLastError();
            async_devs = 0;
        }
        for (uint32_t **w : {&fault_word, &async_word})
            if (*w) {
                (void)hipHostFree(*w);
                *w = nullptr;
            }
    }
    ~Workspaces() { release(); }
};
thread_local Workspaces t_ws;
thread_local uint32_t *t_fault_armed = nullptr;       // the word the pair kernels' launchers pass

// The calling thread's fault word: page-locked, device-mapped, coherent host memory, portable to
// every device (one word serves the thread whatever device it calls on; the kernel's store is visible
// once the stream has drained).  Allocated on the thread's first armed call; nullptr if it cannot be
// had.  The word is 0 between calls (check() clears it), so arming a call is one thread-local store
// and nothing runs between the caller and the launch (the bench's events see no host work).
//
// That first call may be made while a stream is capturing (a thread new to the library that records
// a graph).  A page-locked allocation is refused under the global and thread-local capture modes, and
// the refusal invalidates the capture; it enqueues nothing on any stream, so this one allocation is
// made with the thread's capture mode exchanged for the relaxed one and the mode is put back.  The
// exchange runs on the allocating call only.  A word that cannot be had is an error of the call
// (PairFault::ready), never a launch without a word.
thread_local hipError_t t_fault_alloc_err = hipSuccess;

uint32_t *alloc_fault_word(uint32_t **slot)
{
    if (!*slot) {
        hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
        const bool exchanged = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess;
        void *p = nullptr;
        t_fault_alloc_err = hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable);
        if (exchanged)
            (void)hipThreadExchangeStreamCaptureMode(&mode);
        if (t_fault_alloc_err != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        *slot = static_cast<uint32_t *>(p);
        **slot = 0;
    }
    return *slot;
}

}  // namespace

PairFault::PairFault(unsigned flags)
{
    if ((flags & BRB_BATCH_DEVICE) && (flags & BRB_BATCH_ASYNC)) {
        t_fault_armed = alloc_fault_word(&t_ws.async_word);
        int dev = 0;
        if (t_fault_armed && hipGetDevice(&dev) == hipSuccess && dev >= 0)
            t_ws.async_devs |= uint64_t(1) << (dev < 63 ? dev : 63);
        return;
    }
    w = alloc_fault_word(&t_ws.fault_word);
    t_fault_armed = w;
}

PairFault::~PairFault()
{
    t_fault_armed = nullptr;
}

int PairFault::ready() const
{
    if (t_fault_armed)
        return BRB_BATCH_OK;
    return fail_hip("hipHostMalloc of the thread's wave-pair fault word", t_fault_alloc_err);
}

int PairFault::check(int rc) const
{
    if (!w || __atomic_load_n(w, __ATOMIC_ACQUIRE) == 0)
        return rc;
    __atomic_store_n(w, 0u, __ATOMIC_RELAXED);      // clean for the thread's next call
    if (rc != BRB_BATCH_OK)
        return rc;
    set_err("wave-pair protocol fault: a kernel's bounded wait on its partner wave gave up; the "
            "outputs (and RC4 states) of this call are wrong");
    return BRB_BATCH_FAULT;
}

void release_thread_resources()
{
    // host-mode calls have drained their streams before returning; device-mode ASYNC calls may not
    // have, and release() drains the devices they armed the async fault word on before freeing it
    if (device_count() > 0) {
        t_ws.release();
        brb_host::release_thread_pipes();
    }
}

// Every host-mode call synchronises its stream before it returns (also on its error paths), so a
// workspace is never freed or regrown while a copy into it is still in flight.
void *workspace(size_t bytes, hipError_t *err)
{
    int dev = 0;
    *err = hipGetDevice(&dev);
    if (*err != hipSuccess)
        return nullptr;
    if (t_ws.by_dev.size() <= size_t(dev))
        t_ws.by_dev.resize(dev + 1, {nullptr, 0});
    auto &w = t_ws.by_dev[dev];
    if (w.first && w.second < bytes) {
        (void)hipFree(w.first);
        w = {nullptr, 0};
    }
    if (!w.first) {
        size_t cap = std::max<size_t>(bytes, size_t(1) << 20);
        void *p = nullptr;
        *err = hipMalloc(&p, cap);
        if (*err != hipSuccess)
            return nullptr;
        w = {p, cap};
    }
    return w.first;
}

}  // namespace brb_api

namespace brb {
uint32_t *pair_fault_word()
{
    return brb_api::t_fault_armed;
}
uint32_t *pair_fault_arm(uint32_t *w)
{
    uint32_t *prev = brb_api::t_fault_armed;
    brb_api::t_fault_armed = w;
    return prev;
}
}  // namespace brb

using brb_api::clear_err;
using brb_api::device_ok;
using brb_api::fail_hip;
using brb_api::set_err;

extern "C" {

int BRB_CryptoGPU_Available(void)
{
    clear_err();
    return device_ok() == BRB_BATCH_OK ? 1 : 0;
}

int BRB_CryptoGPU_DeviceCount(void)
{
    clear_err();
    const int n = brb_api::device_count();
    if (n == 0)
        (void)device_ok();   // sets the reason
    return n;
}

int BRB_CryptoGPU_SetDevice(int dev)
{
    clear_err();
    if (int ok = device_ok(); ok != BRB_BATCH_OK)
        return ok;
    if (dev < 0 || dev >= brb_api::device_count()) {
        set_err("device %d out of range (%d visible)", dev, brb_api::device_count());
        return BRB_BATCH_BADARG;
    }
    hipError_t e = hipSetDevice(dev);
    return e == hipSuccess ? BRB_BATCH_OK : fail_hip("hipSetDevice", e);
}

int BRB_CryptoGPU_GetDevice(void)
{
    clear_err();
    if (device_ok() != BRB_BATCH_OK)
        return -1;
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) {
        fail_hip("hipGetDevice", e);
        return -1;
    }
    return dev;
}

void BRB_CryptoGPU_ThreadCleanup(void)
{
    clear_err();
    brb_api::release_thread_resources();
}

const char *BRB_CryptoGPU_LastError(void)
{
    return brb_api::t_err.c_str();
}

int BRB_CryptoGPU_AsyncFaultCheck(void)
{
    clear_err();
    uint32_t *w = brb_api::t_ws.async_word;
    if (!w || __atomic_load_n(w, __ATOMIC_ACQUIRE) == 0)
        return BRB_BATCH_OK;
    __atomic_store_n(w, 0u, __ATOMIC_RELAXED);
    set_err("wave-pair protocol fault in a device-mode BRB_BATCH_ASYNC call of this thread since the last check: "
            "that call's outputs (and RC4 states) are wrong");
    return BRB_BATCH_FAULT;
}

const char *BRB_CryptoGPU_Version(void)
{
    return "brb_crypto_gpu 0.1 (gfx950)";
}

int BRB_CryptoGPU_TestOption(const char *name, int value, int *old)
{
    clear_err();
    static const struct {
        const char *name;
        brb_opt::Opt opt;
        int lo, hi;
    } known[] = {{"rc4_sector", brb_opt::kRc4Sector, -1, 1},
                 {"var_line", brb_opt::kVarLine, 0, 1},
                 {"fixed_var_line", brb_opt::kFixedVarLine, 0, 1},
                 {"var_sort", brb_opt::kVarSort, 0, 2},
                 {"devices", brb_opt::kDevices, 0, 16},   // an all-devices batcher takes at most 16 parts
                 {"b64_group", brb_opt::kB64Group, -1, 6},
                 {"host_chunk_mib", brb_opt::kHostChunkMiB, 0, 1024},
                 {"host_digest_chunk_mib", brb_opt::kHostDigestChunkMiB, 0, 1024},
                 {"seg_line", brb_opt::kSegLine, 0, 2},
                 {"b64_kernel", brb_opt::kB64Kernel, 0, 3},
                 {"line_slots", brb_opt::kLineSlots, 0, 3},
                 {"rc4md5_pair", brb_opt::kRc4Pair, 0, 1},
                 {"rc4_pair", brb_opt::kRc4CryptPair, 0, 1},
                 {"pair_stall", brb_opt::kPairStall, 0, 1},
                 {"bf_keyed", brb_opt::kBfKeyed, 0, 2},
                 {"rc4_list_coop", brb_opt::kRc4ListCoop, 0, 1}};
    if (!name) {
        set_err("NULL option name");
        return BRB_BATCH_BADARG;
    }
    for (const auto &k : known)
        if (strcmp(name, k.name) == 0) {
            if (value < k.lo || value > k.hi) {
                set_err("test option %s: value %d out of [%d, %d]", name, value, k.lo, k.hi);
                return BRB_BATCH_BADARG;
            }
            const int prev = brb_opt::g_opt[k.opt].exchange(value, std::memory_order_relaxed);
            if (old)
                *old = prev;
            return BRB_BATCH_OK;
        }
    set_err("unknown test option '%s'", name);
    return BRB_BATCH_BADARG;
}

int BRB_CryptoGPU_TestFixedRoute(uint64_t data_addr, uint32_t rec_len)
{
    return brb_digest::fixed_route(uintptr_t(data_addr), rec_len);
}

}  // extern "C"
