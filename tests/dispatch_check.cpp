// Stand-alone check of nesie_amd/csrc/dispatch.h, built by the host compiler (test_dispatch_cpu.py).
// Exit status 0 when every check holds; otherwise the failed checks are printed and the status is 1.
#include <stdio.h>

#include <initializer_list>

#include "dispatch.h"

static int failures = 0;
#define CHECK(cond)                                          \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("line %d: %s\n", __LINE__, #cond);              \
      ++failures;                                            \
    }                                                        \
  } while (0)

// what a kernel instantiation stands for: the template arguments, readable at run time
template <bool R, bool N>
static int bools() { return (R ? 2 : 0) + (N ? 1 : 0); }
template <int V>
static int value() { return V; }
template <int A, bool B>
static int pair() { return A * 2 + (B ? 1 : 0); }

int main() {
  using nesie::with_bool;
  using nesie::with_int;

  // with_bool: each value reaches its own constant, once
  for (int v = 0; v < 2; ++v) {
    int calls = 0, got = -1;
    with_bool(v != 0, [&](auto B) {
      static_assert(std::is_same<decltype(B), std::true_type>::value ||
                    std::is_same<decltype(B), std::false_type>::value, "a bool constant");
      ++calls;
      got = bools<B(), B()>();
    });
    CHECK(calls == 1);
    CHECK(got == (v ? 3 : 0));
  }

  // with_int: each listed value reaches its own constant, once, and the call says so
  const int listed[] = {1, 2, 4, 8, 16};
  for (int v : listed) {
    int calls = 0, got = -1;
    const bool hit = with_int<1, 2, 4, 8, 16>(v, [&](auto V) {
      ++calls;
      got = value<V()>();
    });
    CHECK(hit);
    CHECK(calls == 1);
    CHECK(got == v);
  }
  // ... whatever the order of the list (paconv.hip lists <4, 1>), zero and negatives included
  for (int v : {4, 1}) {
    int calls = 0, got = -1;
    CHECK((with_int<4, 1>(v, [&](auto V) { ++calls; got = value<V()>(); })));
    CHECK(calls == 1 && got == v);
  }
  for (int v : {0, -3}) {
    int calls = 0, got = 99;
    CHECK((with_int<-3, 0, 2>(v, [&](auto V) { ++calls; got = value<V()>(); })));
    CHECK(calls == 1 && got == v);
  }
  // a value listed twice still runs the functor once
  {
    int calls = 0;
    CHECK((with_int<3, 3>(3, [&](auto) { ++calls; })));
    CHECK(calls == 1);
  }

  // an unlisted value: nothing is called and the result is false (there is no catch-all arm)
  for (int v : {0, 3, 5, 17, 32, -1}) {
    int calls = 0;
    const bool hit = with_int<1, 2, 4, 8, 16>(v, [&](auto) { ++calls; });
    CHECK(!hit);
    CHECK(calls == 0);
  }

  // two levels: bool in bool, bool in int and int in int, every combination
  for (int r = 0; r < 2; ++r)
    for (int n = 0; n < 2; ++n) {
      int calls = 0, got = -1;
      with_bool(r != 0, [&](auto R) {
        with_bool(n != 0, [&](auto N) {
          ++calls;
          got = bools<R(), N()>();
        });
      });
      CHECK(calls == 1);
      CHECK(got == r * 2 + n);
    }
  for (int a : {1, 2, 3, 4})
    for (int b = 0; b < 2; ++b) {
      int calls = 0, got = -1;
      const bool hit = with_int<1, 2, 3, 4>(a, [&](auto A) {
        with_bool(b != 0, [&](auto B) {
          ++calls;
          got = pair<A(), B()>();
        });
      });
      CHECK(hit && calls == 1);
      CHECK(got == a * 2 + b);
    }
  for (int a : {1, 3})
    for (int b : {1, 2, 4, 8}) {
      int calls = 0, got = -1;
      bool inner = false;
      const bool outer = with_int<1, 3>(a, [&](auto A) {
        inner = with_int<1, 2, 4, 8>(b, [&](auto B) {
          ++calls;
          got = value<A() * 100 + B()>();
        });
      });
      CHECK(outer && inner && calls == 1);
      CHECK(got == a * 100 + b);
    }
  // an unlisted inner value under a listed outer one: the outer functor ran, the inner did not
  {
    int outer_calls = 0, inner_calls = 0;
    bool inner = true;
    CHECK((with_int<1, 3>(3, [&](auto) {
      ++outer_calls;
      inner = with_int<1, 2>(5, [&](auto) { ++inner_calls; });
    })));
    CHECK(outer_calls == 1 && inner_calls == 0 && !inner);
  }

  if (failures == 0) printf("dispatch.h: ok\n");
  return failures ? 1 : 0;
}
