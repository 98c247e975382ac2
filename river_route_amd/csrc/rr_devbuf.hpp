// rr_devbuf.hpp -- DevBuf<T>: the owner of one device allocation.  Every device array of the engine is a DevBuf (a member of
// rr_plan or a local of an entry point), so nothing is released by hand: a buffer frees its block when it is destroyed, reset or
// given another block.  The header knows nothing of HIP: it reaches the device through the two functions declared below, which
// rr_exec.hpp defines over hipMalloc / hipFree (tests/devbuf_main.cpp: over malloc / free).
#pragma once

#include <cstddef>
#include <cstdint>

namespace rr {

int dev_mem_alloc(void **p, size_t bytes);      // 0, or the status of a refused allocation (*p is NULL then; the message is set)
void dev_mem_free(void *p);

template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), count_(o.count_) { o.p_ = nullptr; o.count_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; count_ = o.count_; o.p_ = nullptr; o.count_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }

    T *get() const { return p_; }
    operator T *() const { return p_; }
    int64_t count() const { return count_; }      // capacity in elements, 0 when empty

    // Releases what the buffer holds, THEN allocates (the record ring can be most of the card: old and new never coexist).
    // count <= 0 allocates one element.  On failure the buffer is empty.
    int alloc(int64_t count)
    {
        reset();
        if (count <= 0) count = 1;
        void *p = nullptr;
        if (int rc = dev_mem_alloc(&p, (size_t)count * sizeof(T))) return rc;
        p_ = (T *)p; count_ = count;
        return 0;
    }
    int reserve(int64_t count) { return count_ >= count ? 0 : alloc(count); }
    void reset()
    {
        if (p_) dev_mem_free(p_);
        p_ = nullptr; count_ = 0;
    }

private:
    T *p_ = nullptr;
    int64_t count_ = 0;
};

}  // namespace rr
