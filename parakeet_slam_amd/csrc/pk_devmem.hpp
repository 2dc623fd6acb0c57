// The owner of a filter's device and pinned host memory: every block is recorded when it is made, so that freeing names no
// buffer (release_all) and the bytes held are a sum over what is live, whatever was grown and freed before.
//
// Host code with no HIP in it.  Raw supplies the four calls that touch the runtime, each returning a status (0: fine) that
// comes back unchanged:
//   int  device_alloc(void** p, size_t bytes);   void device_free(void* p);
//   int  host_alloc(void** p, size_t bytes, unsigned flags);   void host_free(void* p);
// so the bookkeeping also runs over malloc / free (tests/test_devmem_host.py).
#pragma once

#include <cstddef>
#include <vector>

namespace pk {

// one member of a reserve: the pointer and the elements it gets
template <typename T>
struct Want { T** p; size_t n; };
template <typename T>
Want<T> want(T** p, size_t n) { return Want<T>{p, n}; }

template <class Raw>
class DevMem {
 public:
  explicit DevMem(Raw raw = Raw()) : raw_(raw) {}
  DevMem(const DevMem&) = delete;
  DevMem& operator=(const DevMem&) = delete;
  ~DevMem() { release_all(); }

  // n elements of device memory; *p is null where it failed
  template <typename T>
  int alloc(T** p, size_t n) { return take(reinterpret_cast<void**>(p), n * sizeof(T), false, 0); }
  // ... of pinned host memory: recorded and freed like the others, not counted in device_bytes()
  template <typename T>
  int alloc_host(T** p, size_t n, unsigned flags) { return take(reinterpret_cast<void**>(p), n * sizeof(T), true, flags); }

  // Frees the block that starts at ptr.  Null, or a pointer that is not (or no longer) a live block: nothing happens.
  void release(const void* ptr) {
    if (!ptr) return;
    for (size_t i = blocks_.size(); i-- > 0;)
      if (blocks_[i].ptr == ptr) {
        drop(blocks_[i]);
        blocks_.erase(blocks_.begin() + (std::ptrdiff_t)i);
        return;
      }
  }
  void release_all() {
    while (!blocks_.empty()) {
      drop(blocks_.back());
      blocks_.pop_back();
    }
  }

  // The grow pattern, for buffers that share one capacity.  need <= *cap: nothing happens, and quiesce is not called.  Otherwise
  // quiesce() -- what has to finish before the old blocks may go; a status like Raw's -- then every member is freed and allocated
  // afresh, in the order given, and *cap becomes new_cap last: a failure leaves *cap at 0, the members before it allocated (and
  // recorded), the failed one and those behind it null.
  template <typename C, typename Quiesce, typename... T>
  int reserve(C* cap, C need, C new_cap, Quiesce&& quiesce, Want<T>... w) {
    if (need <= *cap) return 0;
    int rc = quiesce();
    if (rc) return rc;
    *cap = 0;
    (free_and_null(w.p), ...);
    ((rc = rc ? rc : alloc(w.p, w.n)), ...);
    if (rc) return rc;
    *cap = new_cap;
    return 0;
  }

  size_t device_bytes() const { return device_bytes_; }
  size_t host_bytes() const { return host_bytes_; }
  size_t live_blocks() const { return blocks_.size(); }

 private:
  struct Block { void* ptr; size_t bytes; bool host; };
  int take(void** p, size_t bytes, bool host, unsigned flags) {
    *p = nullptr;
    blocks_.reserve(blocks_.size() + 1);  // (no exception between the allocation and its record)
    const int rc = host ? raw_.host_alloc(p, bytes, flags) : raw_.device_alloc(p, bytes);
    if (rc) {
      *p = nullptr;
      return rc;
    }
    blocks_.push_back(Block{*p, bytes, host});
    (host ? host_bytes_ : device_bytes_) += bytes;
    return 0;
  }
  void drop(const Block& b) {
    b.host ? raw_.host_free(b.ptr) : raw_.device_free(b.ptr);
    (b.host ? host_bytes_ : device_bytes_) -= b.bytes;
  }
  template <typename T>
  void free_and_null(T** p) {
    release(*p);
    *p = nullptr;
  }

  Raw raw_;
  std::vector<Block> blocks_;
  size_t device_bytes_ = 0, host_bytes_ = 0;
};

}  // namespace pk
