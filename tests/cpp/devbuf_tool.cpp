// devbuf_tool.cpp -- csrc/pft_devbuf.h on the host (tests/test_devbuf_host.py): pft_dev_alloc / pft_dev_free over malloc, with
// a counter that makes the k-th allocation fail and a ledger of the live allocations.  Prints one line per check that
// fails and "ok <checks>" at the end; exit status 0 only when nothing failed and nothing is left allocated.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <utility>

#include "pft_devbuf.h"

static std::set<void*> g_live;
static long g_allocs = 0, g_frees = 0, g_bad_frees = 0;
static long g_fail_at = -1;  // the g_fail_at-th allocation from now (0 = the next one) fails; -1: none

int pft_dev_alloc(void** p, size_t bytes) {
  g_allocs++;
  if (g_fail_at == 0) {
    g_fail_at = -1;
    *p = nullptr;
    return 2;
  }
  if (g_fail_at > 0) g_fail_at--;
  *p = malloc(bytes);
  if (!*p) return 2;
  memset(*p, 0xa5, bytes);
  g_live.insert(*p);
  return 0;
}
void pft_dev_free(void* p) {
  g_frees++;
  if (!g_live.erase(p)) {  // never handed out, or freed twice
    g_bad_frees++;
    return;
  }
  free(p);
}
const char* pft_dev_alloc_error() { return "out of memory"; }

static int g_checks = 0, g_failed = 0;
#define CHECK(c)                                            \
  do {                                                      \
    g_checks++;                                             \
    if (!(c)) {                                             \
      g_failed++;                                           \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                       \
  } while (0)

static void reserve_and_growth() {
  DevBuf<uint32_t> b;
  CHECK(b.get() == nullptr && b.cap() == 0 && !b);
  CHECK(b.reserve(0) && b.get() == nullptr && g_allocs == 0);  // nothing asked for, nothing there
  CHECK(b.reserve(100) && b.cap() == 100 && b.get() != nullptr && g_live.size() == 1);
  uint32_t* p = b;  // the implicit conversion
  for (int i = 0; i < 100; i++) p[i] = (uint32_t)i;  // (the sanitizer build checks the size)
  const long a0 = g_allocs, f0 = g_frees;
  CHECK(b.reserve(100) && b.reserve(7) && b.reserve(0));
  CHECK(b.get() == p && b.cap() == 100 && g_allocs == a0 && g_frees == f0);  // below the capacity: untouched
  CHECK(b.reserve(101) && b.cap() == 101);
  CHECK(g_allocs == a0 + 1 && g_frees == f0 + 1 && g_live.size() == 1);  // growth frees exactly once
  b.get()[100] = 1u;
  CHECK(b.alloc(5) && b.cap() == 5 && g_allocs == a0 + 2 && g_frees == f0 + 2);  // alloc always replaces
  CHECK(b.alloc(0) && b.cap() == 1 && b.get() != nullptr);                       // max(n, 1)
  b.reset();
  CHECK(b.get() == nullptr && b.cap() == 0 && g_live.empty());
  b.reset();  // twice is harmless
  CHECK(g_bad_frees == 0);
  DevBuf<double> d;
  CHECK(d.reserve(3) && g_live.size() == 1);
  d.get()[2] = 1.0;
}  // (d is freed by its destructor)

static void failures() {
  DevBuf<float> b;
  g_fail_at = 0;
  CHECK(!b.reserve(10) && b.get() == nullptr && b.cap() == 0 && g_live.empty());
  CHECK(b.reserve(10) && b.cap() == 10);  // a later reserve succeeds
  const long f0 = g_frees;
  g_fail_at = 0;
  CHECK(!b.reserve(20) && b.get() == nullptr && b.cap() == 0);  // a failed growth: the old array is gone, not leaked
  CHECK(g_frees == f0 + 1 && g_live.empty());
  CHECK(b.reserve(4) && b.cap() == 4);  // (4 <= the capacity before the failure: it must allocate all the same)
  b.get()[3] = 1.0f;
  g_fail_at = 0;
  CHECK(!b.alloc(2) && b.get() == nullptr && b.cap() == 0 && g_live.empty());
  CHECK(b.alloc(2) && b.cap() == 2);
  CHECK(g_bad_frees == 0);
}

static void move_and_swap() {
  DevBuf<uint16_t> a, b;
  CHECK(a.alloc(8) && b.alloc(16));
  uint16_t *pa = a, *pb = b;
  a.swap(b);
  CHECK(a.get() == pb && a.cap() == 16 && b.get() == pa && b.cap() == 8);
  const long f0 = g_frees;
  DevBuf<uint16_t> c(std::move(a));
  CHECK(c.get() == pb && c.cap() == 16 && a.get() == nullptr && a.cap() == 0 && g_frees == f0);
  b = std::move(c);  // b's own array (pa) is freed, pb moves in
  CHECK(b.get() == pb && b.cap() == 16 && c.get() == nullptr && c.cap() == 0);
  CHECK(g_frees == f0 + 1 && g_live.size() == 1 && g_live.count(pb) == 1);
  DevBuf<uint16_t>& self = b;
  b = std::move(self);  // self-assignment keeps the array
  CHECK(b.get() == pb && b.cap() == 16 && g_live.size() == 1);
  struct Group {  // a by-value kernel argument beside its owners, as CdInst in csrc/pft_tracker.h
    uint16_t* raw = nullptr;
    DevBuf<uint16_t> own[2];
  };
  Group g, h;
  CHECK(g.own[0].alloc(3) && g.own[1].alloc(3));
  g.raw = g.own[1];
  std::swap(g, h);
  CHECK(h.raw == h.own[1].get() && g.own[0].get() == nullptr && g.own[1].cap() == 0 && g_live.size() == 3);
  g = Group();
  h = Group();
  CHECK(g_live.size() == 1 && g_bad_frees == 0);
}

// the growth of pftt_cd_reserve and of the exact-NN pool: the new buffers are built in locals and swapped in when all are
// there; the k-th allocation fails in turn, the old buffers must survive intact
static bool grow_by_swap(DevBuf<uint32_t> old[3], size_t n) {
  DevBuf<uint32_t> fresh[3];
  for (int k = 0; k < 3; k++)
    if (!fresh[k].alloc(n)) return false;  // (what was built so far is freed on return)
  for (int k = 0; k < 3; k++) {
    memcpy(fresh[k].get(), old[k].get(), old[k].cap() * sizeof(uint32_t));
    old[k].swap(fresh[k]);
  }
  return true;
}

static void build_in_locals_then_swap() {
  DevBuf<uint32_t> old[3];
  uint32_t* before[3];
  for (int k = 0; k < 3; k++) {
    CHECK(old[k].alloc(4));
    for (uint32_t i = 0; i < 4; i++) old[k].get()[i] = 100u * (uint32_t)k + i;
    before[k] = old[k];
  }
  for (int fail = 0; fail < 3; fail++) {
    g_fail_at = fail;
    CHECK(!grow_by_swap(old, 9));
    CHECK(g_fail_at == -1 && g_live.size() == 3);
    for (int k = 0; k < 3; k++) {
      CHECK(old[k].get() == before[k] && old[k].cap() == 4);
      for (uint32_t i = 0; i < 4; i++) CHECK(old[k].get()[i] == 100u * (uint32_t)k + i);
    }
  }
  CHECK(grow_by_swap(old, 9) && g_live.size() == 3);
  for (int k = 0; k < 3; k++) {
    CHECK(old[k].cap() == 9 && old[k].get() != nullptr && g_live.count(before[k]) == 0);
    for (uint32_t i = 0; i < 4; i++) CHECK(old[k].get()[i] == 100u * (uint32_t)k + i);
    old[k].get()[8] = 0u;
  }
  CHECK(g_bad_frees == 0);
}

int main() {
  reserve_and_growth();
  CHECK(g_live.empty());
  failures();
  CHECK(g_live.empty());
  move_and_swap();
  CHECK(g_live.empty());
  build_in_locals_then_swap();
  CHECK(g_live.empty() && g_bad_frees == 0);  // every array handed out was freed, and freed once
  printf("live %zu bad_frees %ld\n", g_live.size(), g_bad_frees);
  if (g_failed || !g_live.empty() || g_bad_frees) return 1;
  printf("ok %d\n", g_checks);
  return 0;
}
