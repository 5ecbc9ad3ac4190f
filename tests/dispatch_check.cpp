// Stand-alone check of csrc/lte_dispatch.h (plain C++17, no HIP): built and run
// by test_dispatch_cpu.py.  Exit status 0 and "ok" on success; the first
// failed check is printed otherwise.
#include <cstdio>
#include <vector>

#include "lte_dispatch.h"

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                                    \
    }                                                                \
  } while (0)

// the value as a template argument and as an array bound
template <int V>
struct Tag {
  static constexpr int value = V;
};
template <bool V>
struct Flag {
  static constexpr bool value = V;
};

struct Seen {
  std::vector<int> got;   // one entry per call of the callable
  template <class C>
  void operator()(C c) {
    static_assert(std::is_same<typename C::value_type, int>::value, "an ic<V>");
    char bound[(c() & 7) + 1];           // constant expression: array bound
    got.push_back(Tag<c()>::value);      // ... and template argument
    CHECK(sizeof(bound) == (size_t)(C::value & 7) + 1);
    CHECK(C::value == Tag<c()>::value);
  }
};

template <class Call>
static std::vector<int> calls(Call&& call) {
  Seen s;
  call(s);
  return s.got;
}

int main() {
  using V = std::vector<int>;
  static_assert(std::is_same<ic<3>, std::integral_constant<int, 3>>::value, "ic");
  static_assert(std::is_same<bc<true>, std::integral_constant<bool, true>>::value, "bc");

  // with_int: every listed value reaches the callable as that constant, once
  for (int v : {7, -1, 0, 2048}) {
    bool m = false;
    CHECK(calls([&](Seen& s) { m = with_int<7, -1, 0, 2048>(v, s); }) == V{v});
    CHECK(m);
  }
  // ... an unlisted one calls nothing and reports no match
  for (int v : {1, 8, -2, 2047}) {
    bool m = true;
    CHECK(calls([&](Seen& s) { m = with_int<7, -1, 0, 2048>(v, s); }).empty());
    CHECK(!m);
  }
  // ... a value listed twice is taken once
  CHECK(calls([&](Seen& s) { with_int<4, 4>(4, s); }) == V{4});

  // with_int_or: listed values as themselves, any other as the fallback
  for (int v : {4, 6}) CHECK(calls([&](Seen& s) { with_int_or<0, 4, 6>(v, s); }) == V{v});
  for (int v : {0, 1, 5, 20}) CHECK(calls([&](Seen& s) { with_int_or<0, 4, 6>(v, s); }) == V{0});
  CHECK(calls([&](Seen& s) { with_int_or<3, 1, 2>(9, s); }) == V{3});
  CHECK(calls([&](Seen& s) { with_int_or<4, 2>(4, s); }) == V{4});

  // with_bps: 2 / 4 / 6, nothing else
  for (int v : {2, 4, 6}) {
    bool m = false;
    CHECK(calls([&](Seen& s) { m = with_bps(v, s); }) == V{v});
    CHECK(m);
  }
  for (int v : {0, 1, 3, 5, 8, -2}) {
    bool m = true;
    CHECK(calls([&](Seen& s) { m = with_bps(v, s); }).empty());
    CHECK(!m);
  }

  // with_n: the listed sizes at compile time, any other as 0 (run-time N)
  for (int v : {2048, 1024}) CHECK(calls([&](Seen& s) { with_n<2048, 1024>(v, s); }) == V{v});
  for (int v : {128, 512, 1536, 4096}) CHECK(calls([&](Seen& s) { with_n<2048, 1024>(v, s); }) == V{0});
  CHECK(calls([&](Seen& s) { with_n<2048>(1024, s); }) == V{0});

  // with_bool: a bc<V>, usable as a template argument and in if constexpr
  for (bool v : {false, true}) {
    int n = 0;
    with_bool(v, [&](auto b) {
      static_assert(std::is_same<typename decltype(b)::value_type, bool>::value, "a bc<V>");
      ++n;
      CHECK(Flag<b()>::value == v);
      if constexpr (b()) CHECK(v);
      else CHECK(!v);
    });
    CHECK(n == 1);
  }

  // nested, as a launcher writes it: constants from outer calls stay constant
  // expressions inside, and if constexpr prunes a combination
  int hits = 0, picked = 0;
  const bool matched = with_bps(6, [&](auto Q) {
    with_n<2048>(2048, [&](auto NC) {
      with_bool(true, [&](auto ZN) {
        constexpr int NCE = Q() == 2 && ZN() ? 0 : NC();
        picked = Tag<Q() * 10000 + NCE>::value + (Flag<ZN()>::value ? 1 : 0);
        ++hits;
      });
    });
  });
  CHECK(matched && hits == 1 && picked == 62049);
  with_bps(2, [&](auto Q) {
    with_n<2048>(2048, [&](auto NC) {
      with_bool(true, [&](auto ZN) {
        constexpr int NCE = Q() == 2 && ZN() ? 0 : NC();
        picked = Tag<Q() * 10000 + NCE>::value;
      });
    });
  });
  CHECK(picked == 20000);

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
