#pragma once
// geograypher_amd/csrc/scratch_layout.hpp -- how a stage call lays its arrays out in the stage arena (gr_internal.hpp: Scratch,
// stage_acquire).  Integer arithmetic only, no HIP: tests/scratch_layout_main.cpp compiles it on its own.
#include <cstddef>
#include <cstdint>

namespace grimpl {

inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }
inline int bit_length(int64_t v) { int n = 0; while (v > 0) { ++n; v >>= 1; } return n; }

// An array of a layout: its offset, the ONE element type its pointer can be taken at, and -- once the block is acquired and
// Carve::base set -- that pointer: slot().
template <class T> struct Slot {
  size_t off = 0;
  void *const *base = nullptr;
  operator size_t() const { return off; }
  T *operator()() const { return (T *)((unsigned char *)*base + off); }
};

// A bump pointer over one scratch block.  Every array starts at a multiple of 256 bytes; an array of no elements takes no
// space.  Overlays: m = mark(); carve one phase; rewind(m); carve the other -- total() is the peak over both.
struct Carve {
  size_t top = 0, peak = 0;
  void *base = nullptr;   // the block these offsets are in, set by the call that acquired it
  size_t bytes(size_t n) { const size_t o = top; top += up256(n); peak = top > peak ? top : peak; return o; }
  template <class T> Slot<T> array(int64_t n) { return {bytes(sizeof(T) * (size_t)(n > 0 ? n : 0)), &base}; }
  size_t mark() const { return top; }
  void rewind(size_t m) { top = m; }
  size_t total() const { return peak; }
};

// A layout and the temporaries of the library steps that run in it (cub_steps.hpp): every step folds the size it asks for into
// need(), finish() places the largest behind the peak of everything carved -- no phase overlays it -- and returns the block's size.
struct Plan : Carve {
  size_t tmp_bytes = 0, tmp_off = 0;
  void need(size_t b) { tmp_bytes = b > tmp_bytes ? b : tmp_bytes; }
  size_t finish() { rewind(total()); tmp_off = bytes(tmp_bytes); return total(); }
  void *tmp() const { return (unsigned char *)base + tmp_off; }
};

}  // namespace grimpl
