// devbuf.h -- the owner of one cached device block (devcache.h: cached_malloc / cached_free).
//
// DevBuf<T> is a move-only pointer plus the size that was asked for: the typed view of a DevBlock.  A plan's device memory is a set of
// these: releasing the plan's device state is assigning a default-constructed one (every block goes back to the cache, every count is 0),
// and the bytes a plan holds are a sum of bytes() -- there is no second copy of a size to keep in step with its allocation.
//
// Pointers INTO a block (several arrays laid out in one allocation) stay raw and own nothing; they die with the state that holds them.
// Host only, no HIP language: tests/devbuf_check.cpp builds it with g++ against a cache of its own.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>

namespace genphi {

hipError_t cached_malloc(void **ptr, size_t bytes);      // devcache.h
hipError_t cached_free(void *ptr);

// The untyped part: the pointer, the bytes asked for and the release.  What holds blocks of several element types (SweepDevice's
// list of a handle's blocks) keeps DevBlock pointers: releasing and summing need no type.
class DevBlock {
public:
    DevBlock() = default;
    DevBlock(const DevBlock &) = delete;
    DevBlock &operator=(const DevBlock &) = delete;
    DevBlock(DevBlock &&o) noexcept : ptr_(o.ptr_), bytes_(o.bytes_) { o.ptr_ = nullptr; o.bytes_ = 0; }
    DevBlock &operator=(DevBlock &&o) noexcept
    {
        if (this != &o) { release(); ptr_ = o.ptr_; bytes_ = o.bytes_; o.ptr_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~DevBlock() { release(); }

    void release()
    {
        if (ptr_) (void)cached_free(ptr_);
        ptr_ = nullptr; bytes_ = 0;
    }
    size_t bytes() const { return bytes_; }

protected:
    // (DevBuf<T>::reserve; least: what a request of no bytes allocates)
    hipError_t reserve_bytes(size_t bytes, size_t least)
    {
        if (ptr_ && bytes_ >= bytes) return hipSuccess;
        release();
        const hipError_t e = cached_malloc(&ptr_, bytes ? bytes : least);
        if (e != hipSuccess) { ptr_ = nullptr; return e; }
        bytes_ = bytes;
        return hipSuccess;
    }
    void *ptr_ = nullptr;
    size_t bytes_ = 0;
};

template <class T>
class DevBuf : public DevBlock {
public:
    // A block of >= n elements: the one held when it has that many, else a new one (the old one is freed first; contents undefined, as
    // with hipMalloc).  count() is then n -- also for n = 0, which still allocates an element so that the pointer is one.  A failed
    // allocation leaves the buffer empty: no pointer, count 0, and the next reserve allocates whatever it is asked for.
    hipError_t reserve(size_t n) { return reserve_bytes(n * sizeof(T), sizeof(T)); }

    T *get() const { return static_cast<T *>(ptr_); }
    operator T *() const { return get(); }      // (reads like the raw pointer it replaces: launches, copies, pointer arithmetic)
    size_t count() const { return bytes_ / sizeof(T); }
};

}  // namespace genphi
