// devmem.hpp -- owners of device and pinned host memory: the only place that frees either.
//
// DevBuf<T> owns one hipMalloc allocation of T (DevBuf<void>: of bytes), PinBuf<T> one hipHostMalloc allocation.  Both are move-only
// handles: a struct of them is reset by assigning a default-constructed one, std::swap exchanges the pointers, and a buffer held in a
// local is freed on every exit of its scope, an early return on a failed HIP call included.  They convert to T *, so they are passed to
// kernels and to the HIP runtime as the raw pointers were.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>

namespace emsar {

namespace detail {
struct DeviceMem {
    static hipError_t get(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void put(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
    static hipError_t get(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void put(void *p) { (void)hipHostFree(p); }
};
}  // namespace detail

template <class T, class Mem>
class OwnedBuf {
    T *p_ = nullptr;
    static constexpr size_t kElem = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);

public:
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    OwnedBuf(const OwnedBuf &) = delete;
    OwnedBuf &operator=(const OwnedBuf &) = delete;
    ~OwnedBuf() { reset(); }

    void reset() { if (p_) Mem::put(p_); p_ = nullptr; }
    // n elements, 16 bytes at least (n == 0 still gives a pointer a kernel may be handed); what was held before is freed
    hipError_t alloc(size_t n) {
        reset();
        return Mem::get((void **)&p_, std::max<size_t>(n * kElem, 16));
    }
    // the same, filled from n elements of host memory
    hipError_t upload(const T *src, size_t n) {
        hipError_t e = alloc(n);
        if (e == hipSuccess && n) e = hipMemcpy(p_, src, n * kElem, hipMemcpyHostToDevice);
        return e;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *operator->() const { return p_; }
};

template <class T> using DevBuf = OwnedBuf<T, detail::DeviceMem>;
template <class T> using PinBuf = OwnedBuf<T, detail::PinnedMem>;

}  // namespace emsar
