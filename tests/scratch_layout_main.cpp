// tests/scratch_layout_main.cpp -- a stand-alone check of csrc/scratch_layout.hpp (test_scratch_layout_host.py builds it with
// -fsanitize=address,undefined and runs it): offsets, overlays through mark / rewind, the peak, empty arrays.  The arrays are
// written into a heap block of exactly total() bytes, so an offset or a size that is off trips the sanitizer.  Then the typed
// slots and the Plan: a slot is its raw offset and points at base + offset; the plan puts the temporaries behind the peak; the
// layouts of gr_cluster_decimate and of outline_trace's block A, carved by hand as they were, against the plan's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "scratch_layout.hpp"

using grimpl::Carve;
using grimpl::Plan;

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
  for (size_t i = 0; i < spans.size(); ++i) std::memset(base + spans[i].off, (int)(i + 1), spans[i].bytes);
  for (size_t i = 0; i < spans.size(); ++i) {
    const unsigned char *p = base + spans[i].off;
    size_t bad = 0;
    for (size_t k = 0; k < spans[i].bytes; ++k) bad += p[k] != (unsigned char)(i + 1);
    CHECK(bad == 0);
  }
}

// A call's layout: the head every phase keeps, two phases that overlay each other, the temporaries behind both.
struct Layout { std::vector<Span> head, a, b; Span tmp; size_t total; };

static void raw(Carve &cv, std::vector<Span> &v, size_t elem, int64_t n, int times = 1) {   // bytes() arithmetic, no types
  for (int k = 0; k < times; ++k) { const size_t b = elem * (size_t)(n > 0 ? n : 0); v.push_back({cv.bytes(b), b}); }
}
static void finish_by_hand(Carve &cv, Layout &l, size_t cub) { cv.rewind(cv.total()); l.tmp = {cv.bytes(cub), cub}; l.total = cv.total(); }
static void finish_by_plan(Plan &p, Layout &l) { l.total = p.finish(); l.tmp = {p.tmp_off, p.tmp_bytes}; }

// gr_cluster_decimate: vused, vpos [V] | key, d2, alt [V] u64, idx, idx_a, hp, hpm [V] or rf [3 F], major, major_a, major_s [F] u64,
// minor, minor_s [F], fidx, fidx_a, fidx_s, fflag, fpos [F] | temporaries
static Layout decimate_by_hand(int64_t V, int64_t F, size_t cub) {
  Layout l; Carve cv;
  raw(cv, l.head, 4, V, 2);
  const size_t phase = cv.mark();
  raw(cv, l.a, 8, V, 3); raw(cv, l.a, 4, V, 4);
  cv.rewind(phase);
  raw(cv, l.b, 4, 3 * F); raw(cv, l.b, 8, F, 3); raw(cv, l.b, 4, F, 2); raw(cv, l.b, 4, F, 5);
  finish_by_hand(cv, l, cub);
  return l;
}
static Layout decimate_by_plan(int64_t V, int64_t F, size_t cub) {   // the steps fold their needs in where they are declared
  Layout l; Plan p;
  l.head = {take<int32_t>(p, V), take<int32_t>(p, V)}; p.need(cub / 3);
  const size_t phase = p.mark();
  for (int k = 0; k < 3; ++k) l.a.push_back(take<unsigned long long>(p, V));
  for (int k = 0; k < 4; ++k) l.a.push_back(take<int32_t>(p, V));
  p.need(cub / 2); p.need(cub); p.need(cub / 3);
  p.rewind(phase);
  l.b.push_back(take<int32_t>(p, 3 * F));
  for (int k = 0; k < 3; ++k) l.b.push_back(take<unsigned long long>(p, F));
  for (int k = 0; k < 2; ++k) l.b.push_back(take<uint32_t>(p, F));
  for (int k = 0; k < 3; ++k) l.b.push_back(take<int32_t>(p, F));
  p.need(cub / 2); p.need(cub / 4);
  l.b.push_back(take<int32_t>(p, F)); l.b.push_back(take<int32_t>(p, F)); p.need(cub / 3);
  finish_by_plan(p, l);
  return l;
}

// outline_trace, block A: head [32] u64, canon [V] | key, key_s [V] i64, idx, idx_s, hp, hpm [V] or pair, pair_s [N3] u64, cl, cl_s,
// flag, ex [N3], ustart, surv, soff [N3 + 1] | temporaries
static Layout outline_a_by_hand(int64_t V, int64_t N3, size_t cub) {
  Layout l; Carve cv;
  raw(cv, l.head, 8, 32); raw(cv, l.head, 4, V);
  const size_t phase = cv.mark();
  raw(cv, l.a, 8, V, 2); raw(cv, l.a, 4, V, 4);
  cv.rewind(phase);
  raw(cv, l.b, 8, N3, 2); raw(cv, l.b, 4, N3, 4); raw(cv, l.b, 4, N3 + 1, 3);
  finish_by_hand(cv, l, cub);
  return l;
}
static Layout outline_a_by_plan(int64_t V, int64_t N3, size_t cub) {
  Layout l; Plan p;
  l.head = {take<unsigned long long>(p, 32), take<int32_t>(p, V)};
  const size_t phase = p.mark();
  l.a = {take<int64_t>(p, V), take<int64_t>(p, V), take<int32_t>(p, V), take<int32_t>(p, V), take<int32_t>(p, V), take<int32_t>(p, V)};
  p.need(cub / 2); p.need(cub / 5);
  p.rewind(phase);
  l.b = {take<unsigned long long>(p, N3), take<unsigned long long>(p, N3), take<uint32_t>(p, N3), take<uint32_t>(p, N3),
         take<int32_t>(p, N3), take<int32_t>(p, N3), take<int32_t>(p, N3 + 1), take<int32_t>(p, N3 + 1), take<int32_t>(p, N3 + 1)};
  p.need(cub); p.need(cub / 7); p.need(0); p.need(cub / 2);
  finish_by_plan(p, l);
  return l;
}

// every offset, every size and the total equal; both phases written and read back in a block of exactly that total
static void same_layout(const Layout &hand, const Layout &plan) {
  const std::vector<Span> *h[3] = {&hand.head, &hand.a, &hand.b}, *p[3] = {&plan.head, &plan.a, &plan.b};
  for (int g = 0; g < 3; ++g) {
    CHECK(h[g]->size() == p[g]->size());
    for (size_t i = 0; i < h[g]->size() && i < p[g]->size(); ++i) CHECK((*h[g])[i].off == (*p[g])[i].off && (*h[g])[i].bytes == (*p[g])[i].bytes);
  }
  CHECK(hand.tmp.off == plan.tmp.off && hand.tmp.bytes == plan.tmp.bytes && hand.total == plan.total);
  CHECK(plan.total == plan.tmp.off + grimpl::up256(plan.tmp.bytes));
  unsigned char *base = (unsigned char *)std::malloc(plan.total ? plan.total : 1);
  CHECK(base != nullptr);
  for (const std::vector<Span> *phase : {&plan.a, &plan.b}) {
    std::vector<Span> live = plan.head;
    live.insert(live.end(), phase->begin(), phase->end());
    live.push_back(plan.tmp);
    check_disjoint(live, plan.total);
    if (base) fill_and_verify(live, base);
  }
  std::free(base);
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

  // typed slots: the offsets of the raw bytes() arithmetic, and a pointer that is base + offset
  for (int64_t n : {(int64_t)1, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)450, (int64_t)1351, (int64_t)100003}) {
    Carve raw, typed;
    const size_t r0 = raw.bytes(8 * (size_t)n), r1 = raw.bytes(4 * (size_t)n), r2 = raw.bytes((size_t)n), r3 = raw.bytes(12 * (size_t)n);
    const grimpl::Slot<int64_t> s0 = typed.array<int64_t>(n);
    const grimpl::Slot<uint32_t> s1 = typed.array<uint32_t>(n);
    const grimpl::Slot<unsigned char> s2 = typed.array<unsigned char>(n);
    const grimpl::Slot<char[12]> s3 = typed.array<char[12]>(n);
    CHECK(s0 == r0 && s1 == r1 && s2 == r2 && s3 == r3 && s0.off == r0 && s3.off == r3 && typed.total() == raw.total());
    unsigned char *base = (unsigned char *)std::malloc(typed.total());
    CHECK(base != nullptr);
    typed.base = base;   // a slot made before the block exists points into it from here on
    if (base) {
      CHECK((unsigned char *)s0() == base + r0 && (unsigned char *)s1() == base + r1 && s2() == base + r2 && (unsigned char *)s3() == base + r3);
      s0()[n - 1] = -1; s1()[n - 1] = 7u; s2()[n - 1] = 9; s3()[n - 1][11] = 3;   // the last element of each
      CHECK(s0()[n - 1] == -1 && s1()[n - 1] == 7u && s2()[n - 1] == 9 && s3()[n - 1][11] == 3);
    }
    std::free(base);
  }

  // a plan: the temporaries behind the peak of both overlay branches, total = peak + up256(the largest need)
  for (int64_t n : {(int64_t)1, (int64_t)65, (int64_t)1351}) {
    for (int order = 0; order < 3; ++order) {
      const size_t needs[3][4] = {{0, 1000, 300, 0}, {1000, 300, 0, 0}, {300, 0, 0, 1000}};   // the maximum in any order
      Plan p;
      std::vector<Span> va = {take<int32_t>(p, n)}, vb = va;
      p.need(needs[order][0]);
      const size_t m = p.mark();
      va.push_back(take<int64_t>(p, 3 * n));
      p.need(needs[order][1]);
      const size_t end_a = p.mark();
      p.rewind(m);
      vb.push_back(take<int32_t>(p, n)); vb.push_back(take<int32_t>(p, n + 1));
      p.need(needs[order][2]); p.need(needs[order][3]);
      const size_t end_b = p.mark(), peak = end_a > end_b ? end_a : end_b;
      CHECK(p.tmp_bytes == 1000 && p.total() == peak);
      const size_t total = p.finish();
      CHECK(p.tmp_off == peak && total == peak + grimpl::up256(1000) && total == p.total());
      const Span tail = {p.tmp_off, p.tmp_bytes};
      va.push_back(tail); vb.push_back(tail);
      check_disjoint(va, total); check_disjoint(vb, total);
      unsigned char *base = (unsigned char *)std::malloc(total);
      CHECK(base != nullptr);
      p.base = base;
      if (base) { CHECK(p.tmp() == base + peak); fill_and_verify(va, base); fill_and_verify(vb, base); }
      std::free(base);
    }
  }
  {  // a need of 0 adds no bytes; neither does no need at all
    Plan p, q;
    p.array<int32_t>(65); q.array<int32_t>(65);
    p.need(0);
    CHECK(p.finish() == 512 && p.tmp_off == 512 && p.tmp_bytes == 0 && q.finish() == 512 && q.tmp_off == 512);
    Plan empty;
    CHECK(empty.finish() == 0);
  }

  // the layouts of gr_cluster_decimate and of outline_trace's block A: the hand-carved sequences they had against the plan's
  for (int64_t V : {(int64_t)0, (int64_t)1, (int64_t)65, (int64_t)1351})
    for (int64_t F : {(int64_t)0, (int64_t)1, (int64_t)65, (int64_t)1351})
      for (size_t tmp : {(size_t)0, (size_t)1, (size_t)1000}) {
        same_layout(decimate_by_hand(V, F, tmp), decimate_by_plan(V, F, tmp));
        same_layout(outline_a_by_hand(V, 3 * F, tmp), outline_a_by_plan(V, 3 * F, tmp));
      }

  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("ok: scratch layout\n");
  return 0;
}
