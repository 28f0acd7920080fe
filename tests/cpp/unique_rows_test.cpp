// unique_rows_test.cpp — kt::unique_rows (kt_rows.h), the row list of kt_delete_pods made unique before it reaches the device:
// against std::set on the shapes a delete batch takes.  Host only: the header needs no HIP and no engine library.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "kt_rows.h"

static int g_fail = 0;
static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {  // splitmix64
  uint64_t z = (g_s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the result equals std::set of the input, in its order; `in_place` says whether the input itself must come back
static void expect(const char* what, const std::vector<int64_t>& in, bool in_place) {
  const std::set<int64_t> want(in.begin(), in.end());
  std::vector<int64_t> scratch;
  const std::vector<int64_t> before = in;
  int64_t n_out = -1;
  const int64_t* got = kt::unique_rows(in.data(), (int64_t)in.size(), scratch, &n_out);
  bool ok = n_out == (int64_t)want.size();
  if (ok) {
    int64_t i = 0;
    for (int64_t w : want) ok = ok && got[i++] == w;
  }
  if (in != before) ok = false, printf("%s: the caller's list was written to\n", what);
  if (in_place && (got != in.data() || scratch.capacity() != 0)) ok = false, printf("%s: an ascending list was copied\n", what);
  if (!in_place && (got != scratch.data() || (int64_t)scratch.size() != n_out)) ok = false, printf("%s: the result is not the scratch list\n", what);
  if (!ok) {
    ++g_fail;
    printf("FAIL %s: %lld entries -> %lld rows, std::set holds %zu\n", what, (long long)in.size(), (long long)n_out, want.size());
  }
}

int main() {
  const int64_t pod_capacity = 1600;
  expect("empty list", {}, true);
  {  // (a null list of no entries: what kt_delete_pods accepts for n = 0)
    std::vector<int64_t> scratch;
    int64_t n_out = -1;
    if (kt::unique_rows(nullptr, 0, scratch, &n_out) != nullptr || n_out != 0 || scratch.capacity() != 0) ++g_fail, printf("FAIL null list\n");
  }
  expect("one entry", {7}, true);
  expect("row 0 alone", {0}, true);
  expect("last row alone", {pod_capacity - 1}, true);
  expect("ascending", {0, 1, 2, 5, 9, 300, pod_capacity - 1}, true);
  expect("two ascending", {3, 4}, true);
  expect("one row twice", {5, 5}, false);
  expect("ascending, then a repeat at the end", {1, 2, 3, 3}, false);
  expect("ascending but for the first pair", {2, 1, 3, 4}, false);
  expect("descending", {pod_capacity - 1, 900, 20, 3, 0}, false);
  expect("all entries equal", std::vector<int64_t>(257, 42), false);
  expect("row 0 and the last row, repeated", {pod_capacity - 1, 0, 0, pod_capacity - 1, 0}, false);
  {
    std::vector<int64_t> v;
    for (int64_t i = 0; i < 8192; ++i) v.push_back(i);
    expect("a full slot, ascending", v, true);
    v.push_back(8191);
    expect("a full slot and one repeat", v, false);
  }
  for (int round = 0; round < 8; ++round) {  // 8193 entries over 300 rows: every row named, many times, scrambled
    std::vector<int64_t> victims;
    std::set<int64_t> seen;
    while (victims.size() < 300) {
      const int64_t r = (int64_t)(rng() % (uint64_t)pod_capacity);
      if (seen.insert(r).second) victims.push_back(r);
    }
    std::vector<int64_t> v;
    for (int i = 0; i < 8193 - 300; ++i) v.push_back(victims[rng() % 300]);
    for (int64_t r : victims) v.insert(v.begin() + (long)(rng() % (v.size() + 1)), r);
    expect("8193 entries over 300 rows", v, false);
  }
  for (int round = 0; round < 200; ++round) {  // short random lists: sorted ones among them
    std::vector<int64_t> v;
    const int n = (int)(rng() % 6);
    for (int i = 0; i < n; ++i) v.push_back((int64_t)(rng() % 4));
    bool asc = true;
    for (int i = 1; i < n; ++i) asc = asc && v[i] > v[i - 1];
    expect("short random list", v, asc);
  }
  if (g_fail) {
    printf("unique_rows_test: %d FAILED\n", g_fail);
    return 1;
  }
  printf("unique_rows_test: ok\n");
  return 0;
}
