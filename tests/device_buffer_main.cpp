// tests/device_buffer_main.cpp -- a stand-alone check of csrc/device_buffer.hpp (test_device_buffer_host.py builds it with
// -fsanitize=address,undefined and runs it with the leak detector on): the header under a policy of its own -- malloc / free, a
// quiesce hook that counts, a switch that makes the k-th allocation fail, and a log of the calls in their order.  Every block is
// written through to its last element, so a buffer that holds less than it says trips the sanitizer; a block freed twice or
// never does too.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "device_buffer.hpp"

using namespace grimpl;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

struct HostMem {
  int allocs = 0, frees = 0, quiesces = 0;
  int fail_at = 0;        // > 0: the fail_at-th alloc() from now returns null
  std::string log;        // 'a' alloc, 'x' failed alloc, 'f' free, 'q' quiesce
  std::string last_what;
  size_t last_bytes = 0;
  void *alloc(size_t bytes, const char *what) {
    ++allocs; last_what = what; last_bytes = bytes;
    if (fail_at > 0 && --fail_at == 0) { log += 'x'; return nullptr; }
    log += 'a';
    return std::malloc(bytes);
  }
  void free(void *p) { ++frees; log += 'f'; std::free(p); }
  void quiesce() { ++quiesces; log += 'q'; }
};

template <class T> static void fill(Buf<T> &b) { std::memset(b.ptr, 0x5A, sizeof(T) * (size_t)b.have); }

struct Five {   // the shape of the mesh upload's group: five members of four element types and five lengths
  Buf<float> blk; Buf<float> soup; Buf<int32_t> orig; Buf<double> bvert; Buf<uint32_t> bidx;
  int reserve_all(HostMem &m, int64_t F) {
    return reserve_group(m, want(blk, (F + 63) / 64, "blk"), want(soup, 9 * F, "soup"), want(orig, F, "orig"),
                         want(bvert, 3 * ((F + 63) / 64), "bvert"), want(bidx, F, "bidx"));
  }
  bool empty() const {
    return !blk.ptr && !soup.ptr && !orig.ptr && !bvert.ptr && !bidx.ptr && !blk.have && !soup.have && !orig.have && !bvert.have && !bidx.have;
  }
  template <class V> void each_buffer(V &&v) { v(blk); v(soup); v(orig); v(bvert); v(bidx); }
};

struct Staged : Buf<uint8_t> { int last = 0; };   // a buffer with something beside it, as the stage arena's Scratch

struct Owner {
  Buf<uint32_t> a; Buf<double> b; Buf<char> never; Staged st;
  template <class V> void each_buffer(V &&v) { v(a); v(b); v(never); v(st); }
};

int main() {
  {  // 1-3: exact size, no-op when large enough, grow
    HostMem m;
    Buf<uint32_t> b;
    bool fresh = false;
    CHECK(reserve(m, b, 450, "first", &fresh) == GR_OK && fresh && b.ptr && b.have == 450);
    CHECK(m.log == "a" && m.last_bytes == 450 * sizeof(uint32_t) && m.last_what == "first");   // an empty buffer: nothing to wait for
    fill(b);
    uint32_t *const p = b;   // converts to T *
    CHECK(p == b.ptr);
    for (int64_t n : {(int64_t)450, (int64_t)449, (int64_t)1}) {
      fresh = true;
      CHECK(reserve(m, b, n, "again", &fresh) == GR_OK && !fresh && b.ptr == p && b.have == 450);
    }
    CHECK(reserve(m, b, 450, "no flag") == GR_OK && b.ptr == p);
    CHECK(m.log == "a" && m.allocs == 1 && m.frees == 0 && m.quiesces == 0);
    CHECK(reserve(m, b, 451, "more", &fresh) == GR_OK && fresh && b.ptr && b.have == 451);
    CHECK(m.log == "aqfa" && m.quiesces == 1 && m.frees == 1 && m.last_bytes == 451 * sizeof(uint32_t));   // quiesce, free, allocate
    fill(b);
    release(m, b);
    CHECK(!b.ptr && b.have == 0 && m.frees == 2);
    release(m, b);   // an empty buffer: nothing
    CHECK(m.frees == 2 && m.log == "aqfaf");
  }

  {  // 4: a failing allocation
    HostMem m;
    Buf<double> b;
    bool fresh = true;
    m.fail_at = 1;
    CHECK(reserve(m, b, 7, "none yet", &fresh) == GR_ENOMEM && !fresh && !b.ptr && b.have == 0 && m.log == "x" && m.frees == 0);
    CHECK(reserve(m, b, 7, "now") == GR_OK && b.have == 7);
    fill(b);
    m.log.clear(); m.fail_at = 1; fresh = true;
    CHECK(reserve(m, b, 8, "grow", &fresh) == GR_ENOMEM && !fresh && !b.ptr && b.have == 0);
    CHECK(m.log == "qfx" && m.frees == 1 && m.last_what == "grow" && m.last_bytes == 8 * sizeof(double));   // the old block: freed once
    CHECK(reserve(m, b, 3, "after") == GR_OK && b.have == 3);   // and the buffer is usable again
    fill(b);
    release(m, b);
  }

  // 5: a group of five, the k-th allocation failing -- from empty, and from a group that held blocks
  for (int held = 0; held < 2; ++held)
    for (int k = 1; k <= 5; ++k) {
      HostMem m;
      Five g;
      if (held) {
        CHECK(g.reserve_all(m, 450) == GR_OK && g.blk.have == 8 && g.soup.have == 4050 && g.orig.have == 450 && g.bvert.have == 24 && g.bidx.have == 450);
        fill(g.blk); fill(g.soup); fill(g.orig); fill(g.bvert); fill(g.bidx);
        CHECK(g.reserve_all(m, 450) == GR_OK && g.reserve_all(m, 300) == GR_OK && m.allocs == 5 && m.frees == 0 && m.quiesces == 0);
      }
      const int frees0 = m.frees;
      m.fail_at = k;
      CHECK(g.reserve_all(m, 1922) == GR_ENOMEM && g.empty());
      static const char *const member[5] = {"blk", "soup", "orig", "bvert", "bidx"};
      CHECK(m.last_what == member[k - 1]);   // the error names the member that failed
      // what was held is freed once each (5 old blocks, or none), what was newly allocated too (k - 1 blocks)
      CHECK(m.frees - frees0 == (held ? 5 : 0) + (k - 1));
      CHECK(m.log.find('q') != std::string::npos && m.log.find('q') < m.log.find('f', held ? 5 : 0));   // no free ahead of the first quiesce
      m.fail_at = 0;
      CHECK(g.reserve_all(m, 1922) == GR_OK && g.blk.have == 31 && g.soup.have == 17298 && g.bvert.have == 93 && g.bidx.have == 1922);
      fill(g.blk); fill(g.soup); fill(g.orig); fill(g.bvert); fill(g.bidx);
      // a group that is partly large enough: only the members that are too small move
      float *const soup = g.soup;
      release(m, g.orig);
      CHECK(g.reserve_all(m, 1922) == GR_OK && g.soup.ptr == soup && g.orig.have == 1922);
      release_all(m, g);
      CHECK(g.empty());
    }

  {  // 6: the walk
    HostMem m;
    Owner o;
    CHECK(reserve(m, o.a, 10, "a") == GR_OK && reserve(m, o.b, 20, "b") == GR_OK && reserve(m, o.st, 300, "stage") == GR_OK);
    fill(o.a); fill(o.b); fill(o.st);
    o.st.last = 7;
    release_all(m, o);
    CHECK(m.frees == 3 && !o.a.ptr && !o.b.ptr && !o.never.ptr && !o.st.ptr && !o.a.have && !o.b.have && !o.st.have && o.st.last == 7);
    release_all(m, o);   // a second walk: nothing
    CHECK(m.frees == 3 && m.allocs == 3 && m.quiesces == 0);
  }

  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("ok: device buffer\n");
  return 0;
}
