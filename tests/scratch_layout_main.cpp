// tests/scratch_layout_main.cpp -- a stand-alone check of csrc/scratch_layout.hpp (test_scratch_layout_host.py builds it with
// -fsanitize=address,undefined and runs it): offsets, overlays through mark / rewind, the peak, empty arrays.  The arrays are
// written through at<T>() into a heap block of exactly total() bytes, so an offset or a size that is off trips the sanitizer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scratch_layout.hpp"

using grimpl::Carve;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct Span { size_t off, bytes; };

template <class T> static Span take(Carve &cv, int64_t n) { return {cv.array<T>(n), sizeof(T) * (size_t)(n > 0 ? n : 0)}; }

// the spans of one overlay branch are live together: aligned, inside the block, pairwise disjoint
static void check_disjoint(const std::vector<Span> &spans, size_t total) {
  for (size_t i = 0; i < spans.size(); ++i) {
    CHECK(spans[i].off % 256 == 0);
    CHECK(spans[i].off + spans[i].bytes <= total);
    for (size_t j = 0; j < i; ++j)
      CHECK(spans[i].bytes == 0 || spans[j].bytes == 0 || spans[i].off + spans[i].bytes <= spans[j].off ||
            spans[j].off + spans[j].bytes <= spans[i].off);
  }
}

// fill every span with its own byte, then read all of them back: a span that another one overlaps has lost its pattern
static void fill_and_verify(const std::vector<Span> &spans, unsigned char *base) {
  for (size_t i = 0; i < spans.size(); ++i) std::memset(Carve::at<unsigned char>(base, spans[i].off), (int)(i + 1), spans[i].bytes);
  for (size_t i = 0; i < spans.size(); ++i) {
    const unsigned char *p = Carve::at<unsigned char>(base, spans[i].off);
    size_t bad = 0;
    for (size_t k = 0; k < spans[i].bytes; ++k) bad += p[k] != (unsigned char)(i + 1);
    CHECK(bad == 0);
  }
}

int main() {
  CHECK(grimpl::up256(0) == 0 && grimpl::up256(1) == 256 && grimpl::up256(256) == 256 && grimpl::up256(257) == 512);
  CHECK(grimpl::bit_length(0) == 0 && grimpl::bit_length(1) == 1 && grimpl::bit_length(255) == 8 && grimpl::bit_length(256) == 9 &&
        grimpl::bit_length(-5) == 0 && grimpl::bit_length(((int64_t)1 << 40) - 1) == 40);

  // sizes around the alignment, odd element sizes, more than 2^32 bytes of layout (arithmetic only)
  for (int64_t n : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)450, (int64_t)1351, (int64_t)100003}) {
    Carve cv;
    std::vector<Span> common = {take<unsigned long long>(cv, 8), take<int32_t>(cv, n)};
    const size_t m = cv.mark();
    CHECK(m % 256 == 0 && m == cv.total());
    std::vector<Span> va = common, vb = common;   // two overlay branches behind the common head, as in gr_class_outlines
    for (Span sp : {take<int64_t>(cv, n), take<int64_t>(cv, n), take<int32_t>(cv, n), take<unsigned char>(cv, n)}) va.push_back(sp);
    const size_t end_a = cv.mark();
    cv.rewind(m);
    CHECK(cv.mark() == m);
    const Span first_b = take<unsigned long long>(cv, 3 * n);
    CHECK(first_b.off == m);   // rewind puts the next array at the mark
    vb.push_back(first_b);
    for (Span sp : {take<uint32_t>(cv, 3 * n), take<int32_t>(cv, 3 * n + 1), take<char[12]>(cv, n)}) vb.push_back(sp);
    const size_t end_b = cv.mark();
    CHECK(cv.total() == (end_a > end_b ? end_a : end_b));   // the peak over both branches
    cv.rewind(cv.total());
    const Span tail = {cv.bytes(1000), 1000};   // what follows both branches (hipcub's temporaries)
    CHECK(tail.off == (end_a > end_b ? end_a : end_b) && cv.total() == tail.off + 1024);
    va.push_back(tail); vb.push_back(tail);
    check_disjoint(va, cv.total());
    check_disjoint(vb, cv.total());
    unsigned char *base = (unsigned char *)std::malloc(cv.total());
    CHECK(base != nullptr);
    if (base) { fill_and_verify(va, base); fill_and_verify(vb, base); }
    std::free(base);
  }

  {  // the vertex branch larger than the edge branch: the peak is still the maximum
    Carve cv;
    const size_t m = cv.mark();
    cv.array<int64_t>(1000);
    const size_t end_a = cv.mark();
    cv.rewind(m);
    cv.array<int32_t>(10);
    CHECK(cv.mark() == 256 && cv.total() == end_a && end_a == grimpl::up256(8000));
  }

  {  // arrays of no elements (and a negative count) take no space; their successor starts where they would have
    Carve cv;
    const Span a = take<int32_t>(cv, 5), z0 = take<double>(cv, 0), zn = take<int64_t>(cv, -3), b = take<int32_t>(cv, 7), z1 = take<char>(cv, 0);
    CHECK(a.off == 0 && z0.off == 256 && zn.off == 256 && b.off == 256 && z1.off == 512 && cv.total() == 512);
    CHECK(z0.bytes == 0 && zn.bytes == 0 && z1.bytes == 0);
    check_disjoint({a, z0, zn, b, z1}, cv.total());
    unsigned char *base = (unsigned char *)std::malloc(cv.total());
    CHECK(base != nullptr);
    if (base) fill_and_verify({a, z0, zn, b, z1}, base);   // writing "all" of an empty array leaves b's pattern alone
    std::free(base);
    Carve empty;
    CHECK(empty.array<int>(0) == 0 && empty.total() == 0);
  }

  {  // offsets beyond 2^32 stay exact
    Carve cv;
    const size_t o0 = cv.array<unsigned long long>((int64_t)1 << 30), o1 = cv.array<int32_t>(((int64_t)1 << 31) + 1), o2 = cv.bytes(1);
    CHECK(o0 == 0 && o1 == (size_t)8 << 30 && o2 == o1 + ((size_t)8 << 30) + 256 && cv.total() == o2 + 256);
  }

  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("ok: scratch layout\n");
  return 0;
}
