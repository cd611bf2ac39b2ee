// Caller-provided workspaces (host code): every layout is written ONCE, as a function that walks the buffer and takes
// its regions in order.  The `*_bytes` query runs that function on a sizing walk (no base) and returns used(); the entry
// point runs it on the caller's buffer and gets typed pointers back - the size and the carve cannot drift apart.
#pragma once
#include <stddef.h>
#include <stdint.h>

__host__ constexpr size_t round_up(size_t v, size_t q) { return (v + q - 1) / q * q; }

class WsWalk {
 public:
  explicit WsWalk(void* base = nullptr) : base_(static_cast<char*>(base)) {}
  // The next region: `count` elements of T in a slot of round_up(count * sizeof(T), pad) bytes (pad 1 = packed; a fixed
  // slot is one element padded to the slot size).  Null on a sizing walk: offsets are kept, the base is added last.
  template <class T>
  T* take(size_t count, size_t pad = 1) {
    const size_t at = off_;
    off_ += round_up(count * sizeof(T), pad);
    return base_ ? reinterpret_cast<T*>(base_ + at) : nullptr;
  }
  size_t used() const { return off_; }

 private:
  char* base_;
  size_t off_ = 0;
};

// Bytes a layout takes: `layout(w)` run on a sizing walk.
template <class F>
size_t ws_bytes(F&& layout) {
  WsWalk w;
  layout(w);
  return w.used();
}

// The one refusal rule (RUNIA_E_WORKSPACE): no buffer, a short one, or a base that is not a multiple of `base_align`
// bytes (1 = any).  Preconditions such as "only when something is needed" stay at the call site.
static inline bool ws_refused(const void* base, size_t bytes, size_t need, size_t base_align) {
  return !base || bytes < need || reinterpret_cast<uintptr_t>(base) % base_align != 0;
}
