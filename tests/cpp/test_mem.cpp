// The owning buffer and the growth rule of csrc/eppk_mem.hpp under a counting fake policy: plain malloc, a chosen allocation (or alias)
// fails, every live block is recorded, every policy call is logged in order.  Built with -fsanitize=address,undefined by
// tests/test_mem_cpp.py: the sanitizers' leak and double-free detection is the second witness to the counters.
#include "../../gateway-api-inference-extension_amd/csrc/eppk_mem.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>
#include <vector>

namespace {

int g_checks = 0;
#define CHECK(x) do { ++g_checks; if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

struct Fake {
  static std::set<void*> live;
  static std::vector<std::string> log;     // "alloc" / "alias" / "release" / "drain", in call order
  static int calls, fail_alloc_at, fail_alias_at, allocs, aliases, releases;
  static void (*on_alloc)();               // called inside alloc: what the group looks like while it is being made
  static void reset_counters() { log.clear(); calls = allocs = aliases = releases = 0; fail_alloc_at = fail_alias_at = -1; on_alloc = nullptr; }
  static int alloc(void** p, size_t bytes) {
    ++calls; log.push_back("alloc");
    if (on_alloc) on_alloc();
    if (allocs++ == fail_alloc_at) return 1;
    *p = std::malloc(bytes);
    CHECK(*p != nullptr && bytes != 0);
    live.insert(*p);
    return 0;
  }
  static void release(void* p) {
    ++calls; ++releases; log.push_back("release");
    CHECK(live.erase(p) == 1);             // released exactly once, and only what alloc handed out
    std::free(p);
  }
  static int alias(void** dev, void* host) {
    ++calls; log.push_back("alias");
    if (aliases++ == fail_alias_at) return 1;
    *dev = (char*)host + 1;                // (a pinned buffer's device address is not its host address)
    return 0;
  }
};
std::set<void*> Fake::live;
std::vector<std::string> Fake::log;
int Fake::calls = 0, Fake::fail_alloc_at = -1, Fake::fail_alias_at = -1, Fake::allocs = 0, Fake::aliases = 0, Fake::releases = 0;
void (*Fake::on_alloc)() = nullptr;

template <class T> using B = eppk::Buf<T, Fake>;

struct Group {                               // up to three buffers of different types and unit sizes
  B<uint32_t> a; B<double> b; B<void> c;
  int n;
  explicit Group(int n_) : n(n_) {}
  int grow(size_t need, int* drains, bool* fresh, std::string* err) {
    auto drain = [&] { ++*drains; Fake::log.push_back("drain"); return 0; };
    if (n == 1) return eppk::grow(drain, need, {{a, 4u, "a"}}, fresh, err);
    if (n == 2) return eppk::grow(drain, need, {{a, 4u, "a"}, {b, 8u, "b"}}, fresh, err);
    return eppk::grow(drain, need, {{a, 4u, "a"}, {b, 8u, "b"}, {c, 24u, "c"}}, fresh, err);
  }
  size_t cap(int i) const { return i == 0 ? a.cap() : i == 1 ? b.cap() : c.cap(); }
  const void* ptr(int i) const { return i == 0 ? (const void*)a.get() : i == 1 ? (const void*)b.get() : c.get(); }
  const void* dev(int i) const { return i == 0 ? (const void*)a.dev() : i == 1 ? (const void*)b.dev() : c.dev(); }
  bool empty() const { for (int i = 0; i < n; ++i) if (cap(i) != 0 || ptr(i) != nullptr || dev(i) != nullptr) return false; return true; }
  bool holds(size_t units) const { for (int i = 0; i < n; ++i) if (cap(i) != units || ptr(i) == nullptr || dev(i) != (const char*)ptr(i) + 1) return false; return true; }
};

Group* g_watch = nullptr;
void caps_still_zero() { for (int i = 0; i < g_watch->n; ++i) CHECK(g_watch->cap(i) == 0); }

void test_sequences(int n) {
  Fake::reset_counters();
  {
    Group g(n);
    int drains = 0; bool fresh = false; std::string err;
    // first allocation: nothing to drain, capacity = need, and no capacity is set while the group is still being made
    g_watch = &g; Fake::on_alloc = caps_still_zero;
    CHECK(g.grow(48, &drains, &fresh, &err) == EPPK_OK);
    CHECK(fresh && drains == 0 && g.holds(48) && (int)Fake::live.size() == n && Fake::releases == 0 && Fake::allocs == n && Fake::aliases == n);
    // no-op: enough capacity (the same need, a smaller one, and zero): no drain, no policy call
    Fake::reset_counters();
    for (size_t need : {(size_t)48, (size_t)7, (size_t)0}) {
      CHECK(g.grow(need, &drains, &fresh, &err) == EPPK_OK);
      CHECK(!fresh && drains == 0 && Fake::calls == 0 && g.holds(48));
    }
    // replacing growth: one drain, before the first release; every old block released exactly once (Fake::release checks "once");
    // every release before the first allocation; the new capacity appears only when every allocation has succeeded
    Fake::on_alloc = caps_still_zero;
    CHECK(g.grow(700, &drains, &fresh, &err) == EPPK_OK);
    CHECK(fresh && drains == 1 && g.holds(700) && Fake::releases == n && (int)Fake::live.size() == n);
    CHECK(Fake::log[0] == "drain");
    for (int i = 1; i <= n; ++i) CHECK(Fake::log[i] == "release");
    CHECK(Fake::log[n + 1] == "alloc" && (int)Fake::log.size() == 1 + n + 2 * n);
    // small again: reused; larger again: replaced again
    Fake::reset_counters();
    CHECK(g.grow(64, &drains, &fresh, &err) == EPPK_OK && !fresh && drains == 1 && Fake::calls == 0);
    CHECK(g.grow(1500, &drains, &fresh, &err) == EPPK_OK && fresh && drains == 2 && g.holds(1500) && (int)Fake::live.size() == n);
    Fake::reset_counters();
  }
  // destruction releases every block, once
  CHECK(Fake::releases == n && Fake::live.empty());
}

void test_zero_floor() {
  Fake::reset_counters();
  Group g(2);
  int drains = 0; bool fresh = false; std::string err;
  CHECK(g.grow(0, &drains, &fresh, &err) == EPPK_OK && fresh && drains == 0 && g.holds(1));     // need = 0 allocates one unit
  CHECK(g.grow(0, &drains, &fresh, &err) == EPPK_OK && !fresh && g.holds(1));
  CHECK(g.grow(1, &drains, &fresh, &err) == EPPK_OK && !fresh && g.holds(1));
  CHECK(g.grow(2, &drains, &fresh, &err) == EPPK_OK && fresh && drains == 1 && g.holds(2));
}

// A failure at every position of a three-buffer group -- the allocation itself, or (a pinned buffer) its alias -- on a first allocation
// and on a replacement: EPPK_ERR_NOMEM naming buffer and bytes, the whole group empty, nothing live, and a retry that succeeds.
void test_failures() {
  static const char* const names[3] = {"a", "b", "c"};
  static const size_t units[3] = {4u, 8u, 24u};
  for (int replacing = 0; replacing < 2; ++replacing)
    for (int alias_fails = 0; alias_fails < 2; ++alias_fails)
      for (int pos = 0; pos < 3; ++pos) {
        Fake::reset_counters();
        Group g(3);
        int drains = 0; bool fresh = false; std::string err;
        if (replacing) { CHECK(g.grow(48, &drains, &fresh, &err) == EPPK_OK && g.holds(48)); Fake::reset_counters(); }
        (alias_fails ? Fake::fail_alias_at : Fake::fail_alloc_at) = pos;
        const size_t need = replacing ? 700 : 48;
        fresh = true;
        CHECK(g.grow(need, &drains, &fresh, &err) == EPPK_ERR_NOMEM);
        CHECK(!fresh && g.empty() && Fake::live.empty() && drains == replacing);
        CHECK(err.find(names[pos]) == 0 && err.find(std::to_string(need * units[pos]) + " bytes") != std::string::npos);
        // the retry starts clean: a first allocation again (no drain), the group whole
        Fake::reset_counters();
        CHECK(g.grow(need, &drains, &fresh, &err) == EPPK_OK);
        CHECK(fresh && g.holds(need) && (int)Fake::live.size() == 3 && drains == replacing && Fake::releases == 0);
      }
  CHECK(Fake::live.empty());
}

void test_drain_failure_keeps_the_group() {       // a drain that fails frees nothing: the old buffers may still be read
  Fake::reset_counters();
  B<uint32_t> a;
  auto ok = [] { return 0; };
  auto bad = [] { return (int)EPPK_ERR_DEVICE; };
  CHECK(eppk::grow(ok, 8, {{a, 4u, "a"}}) == EPPK_OK);
  uint32_t* before = a;
  CHECK(eppk::grow(bad, 16, {{a, 4u, "a"}}) == EPPK_ERR_DEVICE && a.get() == before && a.cap() == 8 && Fake::releases == 0);
}

void test_move_and_convert() {
  Fake::reset_counters();
  {
    B<uint32_t> a;
    auto none = [] { return 0; };
    CHECK(eppk::grow(none, 5, {{a, 4u, "a"}}) == EPPK_OK);
    uint32_t* raw = a;                                  // reads as the raw pointer did
    CHECK(raw == a.get() && a && (const uint8_t*)a == (const uint8_t*)raw && a + 2 == raw + 2);
    a[4] = 7u; CHECK(raw[4] == 7u);
    B<uint32_t> b(std::move(a));                        // moving leaves the source empty
    CHECK(!a && a.cap() == 0 && a.dev() == nullptr && b.get() == raw && b.cap() == 5 && Fake::calls == 2);
    B<uint32_t> c;
    CHECK(eppk::grow(none, 3, {{c, 4u, "c"}}) == EPPK_OK);
    c = std::move(b);                                   // move assignment releases what the target held
    CHECK(!b && b.cap() == 0 && c.get() == raw && c.cap() == 5 && Fake::releases == 1 && Fake::live.size() == 1);
    c.reset(); c.reset();
    CHECK(!c && c.cap() == 0 && Fake::releases == 2);
  }
  CHECK(Fake::releases == 2 && Fake::live.empty());
}

}  // namespace

int main() {
  for (int n = 1; n <= 3; ++n) test_sequences(n);
  test_zero_floor();
  test_failures();
  test_drain_failure_keeps_the_group();
  test_move_and_convert();
  CHECK(Fake::live.empty());
  std::printf("mem ok: %d checks\n", g_checks);
  return 0;
}
