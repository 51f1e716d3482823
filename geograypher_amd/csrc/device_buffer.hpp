#pragma once
// geograypher_amd/csrc/device_buffer.hpp -- how a context owns device memory: Buf, reserve (THE grow rule), reserve_group (buffers
// that live and die together), release, release_all (one walk over an owner's buffers).  No HIP: the allocator is a policy `A` of
// three functions -- void *alloc(size_t bytes, const char *what) (null on failure, and it words the error), void free(void *),
// void quiesce() (wait for the work that can still use the owner's buffers) --, which gr_internal.hpp instantiates once
// (DeviceMem) and tests/device_buffer_main.cpp with malloc / free.
#include <cstddef>
#include <cstdint>

#include "geograster.h"

namespace grimpl {

template <class T> struct Buf { T *ptr = nullptr; int64_t have = 0; operator T *() const { return ptr; } };   // have: ELEMENTS

template <class A, class T> void release(A &a, Buf<T> &b) { if (b.ptr) a.free(b.ptr); b.ptr = nullptr; b.have = 0; }

// Grow-only, to exactly n >= 1 elements (headroom is the caller's: with_headroom).  A buffer that is large enough is left alone:
// a new mesh or image size does not touch it.  Otherwise quiesce, free, allocate; *fresh says that the block is new (contents
// undefined).  GR_ENOMEM leaves the buffer {nullptr, 0}.
template <class A, class T> int reserve(A &a, Buf<T> &b, int64_t n, const char *what, bool *fresh = nullptr) {
  if (fresh) *fresh = false;
  if (b.ptr && b.have >= n) return GR_OK;
  if (b.ptr) a.quiesce();
  release(a, b);
  b.ptr = static_cast<T *>(a.alloc(sizeof(T) * (size_t)n, what));
  if (!b.ptr) return GR_ENOMEM;
  b.have = n;
  if (fresh) *fresh = true;
  return GR_OK;
}

// reserve_group(a, want(x, n, "x"), want(y, m, "y"), ...): every member holds what was asked of it, or -- GR_ENOMEM -- every
// member is released, those that were large enough included.
template <class T> struct Want { Buf<T> &buf; int64_t n; const char *what; };
template <class T> Want<T> want(Buf<T> &b, int64_t n, const char *what) { return {b, n, what}; }
template <class A, class... T> int reserve_group(A &a, Want<T>... w) {
  if ((... && (reserve(a, w.buf, w.n, w.what) == GR_OK))) return GR_OK;
  a.quiesce();
  (release(a, w.buf), ...);
  return GR_ENOMEM;
}

// Every buffer of `owner`, whose each_buffer(visitor) is the one place that says which buffers it has; the owner's work has ended.
template <class A, class Owner> void release_all(A &a, Owner &owner) { owner.each_buffer([&a](auto &b) { release(a, b); }); }

}  // namespace grimpl
