// Stand-in of this repository for Thrust's header of the same name (TEST INFRASTRUCTURE): thrust::device_ptr over host memory.
#pragma once
#include <cstddef>
namespace thrust {
template <class T>
struct device_ptr {
    T* p;
    explicit device_ptr(T* q = nullptr) : p(q) {}
    T* get() const { return p; }
};
template <class T> inline device_ptr<T> operator+(device_ptr<T> a, std::ptrdiff_t n) { return device_ptr<T>(a.p + n); }
template <class T> inline std::ptrdiff_t operator-(device_ptr<T> a, device_ptr<T> b) { return a.p - b.p; }
}  // namespace thrust
