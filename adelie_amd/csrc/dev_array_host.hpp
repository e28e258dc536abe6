// dev_array_host.hpp — an array that a design handle owns or borrows.  Host-only (no HIP): `Mem` says where the bytes come from,
// so that tests/native/dev_array_main.cpp runs the type on malloc/free under the sanitizers; common.hpp supplies the HIP policy.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>

namespace ahip {

// util/exceptions.hpp:8-55 — same prefixes so that the Python layer's error-vs-warning split keeps working
struct core_error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// bytes that the OwnedArrs of this process own right now (adelie_hip_design_owned_bytes)
inline std::atomic<int64_t>& owned_arr_bytes() {
    static std::atomic<int64_t> b{0};
    return b;
}

// Mem: static void* alloc(size_t bytes) (null on refusal, nothing left pending) and static void free(void*).
// Move-only.  An array either owns its block (alloc / try_alloc: freed by reset() and the destructor) or points at memory
// someone else frees (borrow).  T = void counts in bytes.
template <class T, class Mem>
class OwnedArr {
    T* p_ = nullptr;
    size_t bytes_ = 0;
    bool owns_ = false;
    static constexpr size_t elem() { return sizeof(typename std::conditional<std::is_void<T>::value, char, T>::type); }

public:
    OwnedArr() = default;
    OwnedArr(const OwnedArr&) = delete;
    OwnedArr& operator=(const OwnedArr&) = delete;
    OwnedArr(OwnedArr&& o) noexcept : p_(o.p_), bytes_(o.bytes_), owns_(o.owns_) { o.forget(); }
    OwnedArr& operator=(OwnedArr&& o) noexcept {
        if (this != &o) reset(), p_ = o.p_, bytes_ = o.bytes_, owns_ = o.owns_, o.forget();
        return *this;
    }
    ~OwnedArr() { reset(); }

    // false (and empty) when the memory is refused
    bool try_alloc(size_t count) {
        reset();
        void* q = Mem::alloc(count * elem());
        if (!q) return false;
        p_ = static_cast<T*>(q), bytes_ = count * elem(), owns_ = true;
        owned_arr_bytes() += int64_t(bytes_);
        return true;
    }
    void alloc(size_t count) {
        if (!try_alloc(count))
            throw core_error("adelie_hip: could not allocate " + std::to_string(count * elem()) + " bytes of device memory.");
    }
    void borrow(T* p) { reset(), p_ = p; }
    void borrow(const OwnedArr& o) { if (&o != this) borrow(o.p_); }
    void reset() {
        if (owns_) Mem::free(p_), owned_arr_bytes() -= int64_t(bytes_);
        forget();
    }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    // static_cast<const double*>(arr) on an array whose element type follows the design's dtype
    template <class U, class V = T, class = typename std::enable_if<std::is_void<V>::value>::type>
    explicit operator U*() const { return static_cast<U*>(p_); }

private:
    void forget() { p_ = nullptr, bytes_ = 0, owns_ = false; }
};

} // namespace ahip
