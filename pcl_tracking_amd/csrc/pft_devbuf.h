// pft_devbuf.h -- the one owner of device memory for the four handles (tracker, filter, segmenter, model), host side only:
// no HIP header is needed to read this file, and tests/cpp/devbuf_tool.cpp compiles it with a plain C++ compiler.
//
// Allocation goes through two plain functions.  The library defines them once (pft_api.hip: hipMalloc / hipFree, the
// sticky HIP error cleared after a failure); the host test defines its own over malloc.
//
// Freeing never synchronises by itself: the caller drains the stream that may still touch a buffer BEFORE a call that can
// free it (reserve past the capacity, alloc, reset, swap followed by destruction), as every growth path of the handles does.
#pragma once
#include <stddef.h>

#include <string>

int pft_dev_alloc(void** p, size_t bytes);  // 0 on success (the library: the hipError_t of hipMalloc), *p null otherwise
void pft_dev_free(void* p);
const char* pft_dev_alloc_error();  // the library: hipGetErrorString of this thread's last failed pft_dev_alloc

// raw-pointer form, for the by-value buffer structs that are kernel arguments themselves (FDev, SgBufs, ...)
template <typename T>
static inline int pft_dalloc(T** p, size_t n) {
  return pft_dev_alloc(reinterpret_cast<void**>(p), (n ? n : 1) * sizeof(T));
}
template <typename T>
static inline void pft_dfree(T*& p) {
  if (p) pft_dev_free((void*)p);
  p = nullptr;
}

// A device array and its capacity in elements, kept together: null with capacity 0, or cap() elements at get().
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) {
    o.p_ = nullptr;
    o.cap_ = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      swap(o);
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }
  size_t cap() const { return cap_; }

  // room for n elements; the contents are NOT kept across a growth.  False: the buffer is null, its capacity 0
  bool reserve(size_t n) { return n <= cap_ ? true : alloc(n); }
  // a fresh array of max(n, 1) elements whatever the capacity was, with the same failure rule
  bool alloc(size_t n) {
    reset();
    const size_t c = n ? n : 1;
    if (pft_dalloc(&p_, c) != 0) {
      p_ = nullptr;
      return false;
    }
    cap_ = c;
    return true;
  }
  void reset() {
    pft_dfree(p_);
    cap_ = 0;
  }
  void swap(DevBuf& o) noexcept {
    T* p = p_;
    const size_t c = cap_;
    p_ = o.p_;
    cap_ = o.cap_;
    o.p_ = p;
    o.cap_ = c;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// One error macro for any handle with a `std::string err` (used from the HIP translation units only: hipError_t,
// hipGetErrorString and PFT_ERR_HIP come from their includes).  `call` yields a hipError_t, or pft_dalloc's int.
#define PFT_HIPCHK(h, call)                                                                   \
  do {                                                                                        \
    const hipError_t e_ = static_cast<hipError_t>(call);                                      \
    if (e_ != hipSuccess) {                                                                   \
      (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                           \
      return PFT_ERR_HIP;                                                                     \
    }                                                                                         \
  } while (0)
