// ct_devmem.hpp -- the owners of device memory, pinned host memory and events.  Every hipMalloc / hipHostMalloc allocation of
// the library belongs to exactly one DevBuf / HostBuf, which frees it when it goes out of scope; nothing else in csrc calls
// hipMalloc, hipFree, hipHostMalloc or hipHostFree ("Ownership").  Depends on the HIP runtime only.
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

#include <hip/hip_runtime.h>

namespace ct {

// What the process holds right now (ct_debug_allocations): [0] device buffers, [1] their bytes, [2] pinned host buffers,
// [3] their bytes.  Bumped in hold() and release() below and nowhere else.  The physical chunks behind the virtual range of
// the CT_EXPERIMENTS build's CT_FLAG_VMM_BRICKS are hipMemCreate'd, not hipMalloc'ed, and are NOT counted; the range itself
// counts as one buffer of its address size while the handle's d_mbricks holds it.
inline std::atomic<uint64_t> g_live_allocations[4];

struct DeviceMem {
    static constexpr int kCounter = 0;
    static hipError_t get(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t put(void *p) { return hipFree(p); }
};

struct PinnedMem {
    static constexpr int kCounter = 2;
    static hipError_t get(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t put(void *p) { return hipHostFree(p); }
};

// A move-only owner of one allocation of `capacity()` elements.  Converts to T *, so launches and DevScene / BatchArgs
// assignments read as with a raw pointer.  A temporary is a Buf that goes out of scope -- which its user places after the
// stream synchronise that follows the temporary's last use.  Two ways to grow, and a site keeps to its own:
//   free, then allocate:  buf.reserve(need, slack) -- the old contents are dead, or both copies would not fit;
//   allocate, then swap:  a local Buf, alloc(), and buf = std::move(local) on success -- a failed growth leaves what was there.
template <typename T, typename Mem>
class Buf {
    T *p_ = nullptr;
    size_t cap_ = 0;

public:
    Buf() = default;
    Buf(Buf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~Buf() { reset(); }

    operator T *() const { return p_; }
    T *get() const { return p_; }
    size_t capacity() const { return cap_; }

    // Takes over `count` elements at p, which must be empty-handed before.  (From outside: the virtual range of the VMM bricks.)
    void hold(T *p, size_t count)
    {
        p_ = p;
        cap_ = p ? count : 0;
        if (p) {
            g_live_allocations[Mem::kCounter] += 1;
            g_live_allocations[Mem::kCounter + 1] += cap_ * sizeof(T);
        }
    }
    // Gives the memory up WITHOUT freeing it.
    T *release()
    {
        if (p_) {
            g_live_allocations[Mem::kCounter] -= 1;
            g_live_allocations[Mem::kCounter + 1] -= cap_ * sizeof(T);
        }
        cap_ = 0;
        return std::exchange(p_, nullptr);
    }
    // Frees now.  Empty afterwards whatever the runtime answers.
    hipError_t reset()
    {
        T *p = release();
        return p ? Mem::put(p) : hipSuccess;
    }
    // For an empty buffer (one that is not is freed first).
    hipError_t alloc(size_t count)
    {
        hipError_t e = reset();
        void *p = nullptr;
        e = e == hipSuccess ? Mem::get(&p, count * sizeof(T)) : e;
        if (e == hipSuccess) {
            hold((T *)p, count);
        }
        return e;
    }
    // No-op while need <= capacity(); else frees, then allocates need + slack.  Returns the first error, and holds either the
    // new memory or nothing.  (Re)allocation waits for the device, so callers grow only when a call outgrows every call before it.
    hipError_t reserve(size_t need, size_t slack = 0) { return need <= cap_ ? hipSuccess : alloc(need + slack); }
};

template <typename T>
using DevBuf = Buf<T, DeviceMem>;
template <typename T>
using HostBuf = Buf<T, PinnedMem>;

// ... and of one event, so that nothing has to list the events either.
class Event {
    hipEvent_t e_ = nullptr;

public:
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event()
    {
        if (e_) {
            hipEventDestroy(e_);
        }
    }
    operator hipEvent_t() const { return e_; }
    hipError_t create() { return e_ ? hipSuccess : hipEventCreate(&e_); }
};

} // namespace ct
