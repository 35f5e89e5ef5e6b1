// devbuf.h -- the owner of one cached device block (devcache.h: cached_malloc / cached_free).
//
// DevBuf<T> is a move-only pointer plus the element count that was asked for.  A plan's device memory is a set of these: releasing the
// plan's device state is assigning a default-constructed one (every block goes back to the cache, every count is 0), and the bytes a plan
// holds are a sum of bytes() -- there is no second copy of a size to keep in step with its allocation.
//
// Pointers INTO a block (several arrays laid out in one allocation) stay raw and own nothing; they die with the state that holds them.
// Host only, no HIP language: tests/devbuf_check.cpp builds it with g++ against a cache of its own.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

namespace genphi {

hipError_t cached_malloc(void **ptr, size_t bytes);      // devcache.h
hipError_t cached_free(void *ptr);

template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : ptr_(o.ptr_), count_(o.count_) { o.ptr_ = nullptr; o.count_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); ptr_ = o.ptr_; count_ = o.count_; o.ptr_ = nullptr; o.count_ = 0; }
        return *this;
    }
    ~DevBuf() { release(); }

    void release()
    {
        if (ptr_) (void)cached_free(ptr_);
        ptr_ = nullptr; count_ = 0;
    }
    // A block of >= n elements: the one held when it has that many, else a new one (the old one is freed first; contents undefined, as
    // with hipMalloc).  count() is then n -- also for n = 0, which still allocates an element so that the pointer is one.  A failed
    // allocation leaves the buffer empty: no pointer, count 0, and the next reserve allocates whatever it is asked for.
    hipError_t reserve(size_t n)
    {
        if (ptr_ && count_ >= n) return hipSuccess;
        release();
        void *q = nullptr;
        const hipError_t e = cached_malloc(&q, (n ? n : 1) * sizeof(T));
        if (e != hipSuccess) return e;
        ptr_ = static_cast<T *>(q); count_ = n;
        return hipSuccess;
    }

    T *get() const { return ptr_; }
    operator T *() const { return ptr_; }      // (reads like the raw pointer it replaces: launches, copies, pointer arithmetic)
    size_t count() const { return count_; }
    size_t bytes() const { return count_ * sizeof(T); }

private:
    T *ptr_ = nullptr;
    size_t count_ = 0;
};

}  // namespace genphi
