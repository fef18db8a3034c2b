// Host-only check of okv::Buf (objectkv_amd/csrc/okv_buf.hpp) over a
// malloc-backed memory source that counts live allocations and can fail the
// k-th one.  tests/test_buf.py builds it with -fsanitize=address,undefined and
// runs it; exit status 0 means every check held.  Links no HIP.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>

#include "okv_buf.hpp"

namespace {

struct Counters {
  int live = 0;       // allocations not yet released
  int allocs = 0;     // alloc calls (failed ones included)
  int frees = 0;      // release calls
  int idles = 0;      // idle calls
  int fail_at = 0;    // 1-based alloc call that fails (0: none)
};
Counters g;

struct TestMem {
  using Error = int;
  using Stream = int;
  static Error alloc(void** p, size_t bytes) {
    if (++g.allocs == g.fail_at) return 2;
    *p = malloc(bytes);  // exactly `bytes`: the sanitizer sees any write past the capacity
    if (!*p) return 2;
    memset(*p, 0xa5, bytes);
    ++g.live;
    return 0;
  }
  static void release(void* p) {
    free(p);
    ++g.frees;
    --g.live;
  }
  static Error idle(Stream) {
    ++g.idles;
    return 0;
  }
  static Error copy(void* dst, const void* src, size_t bytes, Stream) {
    memcpy(dst, src, bytes);
    return 0;
  }
};

template <class T>
using Buf = okv::Buf<T, TestMem>;

int failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                                 \
    }                                                             \
  } while (0)

template <class T>
bool invariant(const Buf<T>& b) {
  return b.data() ? b.capacity() > 0 : b.capacity() == 0;
}

// every element of the capacity is writable (the sanitizer checks the bounds)
template <class T>
void touch(Buf<T>& b) {
  if (b.data()) memset(b.data(), 0, b.capacity() * sizeof(T));
}

void test_reserve() {
  g = Counters{};
  {
    Buf<uint32_t> b;
    CHECK(!b.data() && b.capacity() == 0);
    CHECK(b.reserve(0, 100) == 0);
    CHECK(b.data() && b.capacity() == 1024);  // 400 bytes rounded up to 4 KiB
    CHECK(g.allocs == 1 && g.frees == 0 && g.idles == 0);  // nothing to make idle yet
    touch(b);
    uint32_t* p = b.data();
    // smaller or equal: no call reaches the source
    CHECK(b.reserve(0, 10) == 0 && b.reserve(0, 1024) == 0 && b.reserve(0, 0) == 0);
    CHECK(b.data() == p && b.capacity() == 1024);
    CHECK(g.allocs == 1 && g.frees == 0 && g.idles == 0);
    // larger: idle, one free, one allocate; exactly what is asked, rounded to 4 KiB
    CHECK(b.reserve(0, 1025) == 0);
    CHECK(b.capacity() == 2048);
    CHECK(g.allocs == 2 && g.frees == 1 && g.idles == 1 && g.live == 1);
    touch(b);
    // an empty buffer allocates for n == 0 too
    Buf<uint8_t> z;
    CHECK(z.reserve(0, 0) == 0 && z.data() && z.capacity() == 4096);
  }
  CHECK(g.live == 0);
}

void test_fresh() {
  g = Counters{};
  {
    Buf<uint64_t> b;
    bool fresh = false;
    CHECK(b.reserve(0, 8, &fresh) == 0 && fresh);
    fresh = false;
    CHECK(b.reserve(0, 8, &fresh) == 0 && !fresh);
    CHECK(b.reserve(0, 512, &fresh) == 0 && !fresh);  // still inside the first 4 KiB
    CHECK(b.reserve(0, 513, &fresh) == 0 && fresh);
    fresh = false;
    g.fail_at = g.allocs + 1;
    CHECK(b.reserve(0, 5000, &fresh) != 0 && !fresh);  // a failed grow is not fresh
    CHECK(b.reserve(0, 5000, &fresh) == 0 && fresh);
  }
  CHECK(g.live == 0);
}

void test_keep() {
  g = Counters{};
  {
    Buf<uint8_t> b;
    CHECK(b.reserve_keep(0, 1000, 0) == 0 && b.capacity() == 4096);
    for (size_t i = 0; i < 4096; ++i) b.data()[i] = uint8_t(i * 7 + 1);
    CHECK(b.reserve_keep(0, 4096, 4096) == 0 && g.allocs == 1);  // enough room: no call
    const size_t keep = 3000;
    CHECK(b.reserve_keep(0, 4096 + 8192, keep) == 0);
    CHECK(b.capacity() == 4096 + 8192 && g.allocs == 2 && g.frees == 1 && g.live == 1);
    bool same = true;
    for (size_t i = 0; i < keep; ++i) same = same && b.data()[i] == uint8_t(i * 7 + 1);
    CHECK(same);
    touch(b);
    // a failed keeping grow leaves the old allocation and its bytes
    b.data()[5] = 77;
    g.fail_at = g.allocs + 1;
    CHECK(b.reserve_keep(0, 1 << 20, keep) != 0);
    CHECK(b.data() && b.capacity() == 4096 + 8192 && b.data()[5] == 77 && g.live == 1);
    CHECK(b.reserve_keep(0, 1 << 20, keep) == 0 && b.data()[5] == 77 && g.live == 1);
  }
  CHECK(g.live == 0);
}

void test_failed_grow() {
  g = Counters{};
  {
    Buf<uint16_t> b;
    g.fail_at = 1;  // the very first allocation
    CHECK(b.reserve(0, 10) != 0);
    CHECK(!b.data() && b.capacity() == 0 && g.live == 0);
    CHECK(b.reserve(0, 10) == 0 && b.data() && b.capacity() == 2048);
    g.fail_at = g.allocs + 1;  // a grow: the old allocation is gone, the buffer empty
    CHECK(b.reserve(0, 5000) != 0);
    CHECK(!b.data() && b.capacity() == 0 && g.live == 0);
    // the next reserve, even of a size that fitted before, allocates again
    CHECK(b.reserve(0, 10) == 0 && b.data() && b.capacity() == 2048 && g.live == 1);
    touch(b);
  }
  CHECK(g.live == 0);
}

// Six buffers reserved in sequence, as the decode's ensure_blocks does.
struct Group {
  Buf<uint32_t> a, b;
  Buf<uint64_t> c, d;
  Buf<uint8_t> e;
  Buf<uint16_t> f;
  int reserve(size_t n) {
    int rc;
    if ((rc = a.reserve(0, n * 4)) || (rc = b.reserve(0, n + 1)) || (rc = c.reserve(0, n)) ||
        (rc = d.reserve(0, n)) || (rc = e.reserve(0, n / 2 + 1)))
      return rc;
    return f.reserve(0, n);
  }
  bool holds(size_t n) const {
    return a.capacity() >= n * 4 && b.capacity() >= n + 1 && c.capacity() >= n &&
           d.capacity() >= n && e.capacity() >= n / 2 + 1 && f.capacity() >= n && a.data() &&
           b.data() && c.data() && d.data() && e.data() && f.data();
  }
  bool sound() const {
    return invariant(a) && invariant(b) && invariant(c) && invariant(d) && invariant(e) &&
           invariant(f);
  }
  void touch_all() { touch(a), touch(b), touch(c), touch(d), touch(e), touch(f); }
};

void test_group() {
  for (int k = 1; k <= 6; ++k) {
    for (const bool grown : {false, true}) {  // from empty, and from a smaller group
      g = Counters{};
      {
        Group G;
        if (grown) {
          CHECK(G.reserve(300) == 0 && G.holds(300));
          G.touch_all();
        }
        const size_t n = 20000;  // every member has to grow
        g.fail_at = g.allocs + k;
        CHECK(G.reserve(n) != 0);
        CHECK(G.sound() && !G.holds(n));
        G.touch_all();  // what is left is live and as large as it says
        g.fail_at = 0;
        CHECK(G.reserve(n) == 0);
        CHECK(G.sound() && G.holds(n) && g.live == 6);
        G.touch_all();
        const int calls = g.allocs;
        CHECK(G.reserve(n) == 0 && G.reserve(8) == 0 && g.allocs == calls);  // steady state
      }
      CHECK(g.live == 0);
    }
  }
}

void test_move() {
  g = Counters{};
  {
    Buf<uint32_t> a;
    CHECK(a.reserve(0, 10) == 0);
    uint32_t* p = a.data();
    Buf<uint32_t> b(std::move(a));
    CHECK(!a.data() && a.capacity() == 0 && b.data() == p && b.capacity() == 1024);
    Buf<uint32_t> c;
    CHECK(c.reserve(0, 3000) == 0 && g.live == 2);
    c = std::move(b);  // releases c's own allocation
    CHECK(!b.data() && b.capacity() == 0 && c.data() == p && c.capacity() == 1024 && g.live == 1);
    Buf<uint32_t>& self = c;
    c = std::move(self);
    CHECK(c.data() == p && c.capacity() == 1024 && g.live == 1);
    CHECK(a.reserve(0, 1) == 0 && g.live == 2);  // a moved-from buffer is an empty one
    c.reset();
    CHECK(!c.data() && c.capacity() == 0 && g.live == 1);
  }
  CHECK(g.live == 0);
}

}  // namespace

int main() {
  test_reserve();
  test_fresh();
  test_keep();
  test_failed_grow();
  test_group();
  test_move();
  if (failures) {
    fprintf(stderr, "%d checks failed\n", failures);
    return 1;
  }
  puts("okv_buf: all checks passed");
  return 0;
}
