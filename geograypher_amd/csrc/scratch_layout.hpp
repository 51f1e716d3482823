#pragma once
// geograypher_amd/csrc/scratch_layout.hpp -- how a stage call lays its arrays out in the stage arena (gr_internal.hpp: Scratch,
// stage_acquire).  Integer arithmetic only, no HIP: tests/scratch_layout_main.cpp compiles it on its own.
#include <cstddef>
#include <cstdint>

namespace grimpl {

inline size_t up256(size_t b) { return (b + 255) / 256 * 256; }
inline int bit_length(int64_t v) { int n = 0; while (v > 0) { ++n; v >>= 1; } return n; }

// A bump pointer over one scratch block.  Every array starts at a multiple of 256 bytes; an array of no elements takes no
// space.  Overlays: m = mark(); carve one phase; rewind(m); carve the other -- total() is the peak over both.
struct Carve {
  size_t top = 0, peak = 0;
  size_t bytes(size_t n) { const size_t o = top; top += up256(n); peak = top > peak ? top : peak; return o; }
  template <class T> size_t array(int64_t n) { return bytes(sizeof(T) * (size_t)(n > 0 ? n : 0)); }
  size_t mark() const { return top; }
  void rewind(size_t m) { top = m; }
  size_t total() const { return peak; }
  template <class T> static T *at(void *base, size_t off) { return (T *)((unsigned char *)base + off); }
};

}  // namespace grimpl
