// match_codes_test — the match-code record's helpers (kube_throttler_amd/csrc/kt_match_codes.h) on the host: the header alone,
// no HIP, no engine library; built with -fsanitize=address,undefined (kube_throttler_amd/host/Makefile).
//   every count 0..15 round-trips (header, codes, ascending order, decode per list position)
//   16 and more codes give the overflow header, which stays whatever is appended afterwards
//   the run rule on hand-made masks, against a bit-by-bit restatement, and through append_word into a record
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "kt_match_codes.h"

using namespace kt;

static int g_fail = 0;
#define EXPECT(c, ...)                                    \
  do {                                                    \
    if (!(c)) {                                           \
      ++g_fail;                                           \
      printf("FAIL %s:%d: ", __FILE__, __LINE__);         \
      printf(__VA_ARGS__);                                \
      printf("\n");                                       \
    }                                                     \
  } while (0)

// the run rule bit by bit: runs are [lo bit .. the next hi bit]; of the bits of x inside a run the lowest stays
static uint64_t run_rule_slow(uint64_t x, uint64_t lo, uint64_t hi) {
  uint64_t out = 0;
  int k = 0;
  while (k < 64) {
    if (!((lo >> k) & 1ull)) {  // not part of any run (class padding): never matched, never kept
      ++k;
      continue;
    }
    int e = k;
    while (!((hi >> e) & 1ull)) ++e;
    for (int b = k; b <= e; ++b)
      if ((x >> b) & 1ull) {
        out |= 1ull << b;
        break;
      }
    k = e + 1;
  }
  return out;
}

int main() {
  static_assert(sizeof(MatchCodes) == 16 && alignof(MatchCodes) == 16, "one dwordx4");
  // ---- counts 0..15: codes spread over the four list positions, ascending (k, bit)
  for (uint32_t n = 0; n <= 15; ++n) {
    std::vector<uint32_t> want;
    for (uint32_t i = 0; i < n; ++i) want.push_back(match_code(i * 4u / (n ? n : 1u), (i * 37u + 5u * (i / 4u)) & 63u));
    // (make them ascending inside a list position)
    for (size_t i = 1; i < want.size(); ++i)
      if (want[i] <= want[i - 1]) want[i] = want[i - 1] + 1u;
    MatchCodes r{0, 0};
    for (uint32_t c : want) match_codes_append(r, c);
    EXPECT(match_codes_header(r) == n && match_codes_count(r) == n, "count %u: header %u", n, match_codes_header(r));
    uint64_t by_list[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < n; ++i) {
      EXPECT(match_code_at(r, i) == want[i], "count %u: code %u is %u, want %u", n, i, match_code_at(r, i), want[i]);
      EXPECT(i == 0 || match_code_at(r, i) > match_code_at(r, i - 1), "count %u: codes %u, %u not ascending", n, i - 1, i);
      by_list[match_code_list(want[i])] |= 1ull << match_code_bit(want[i]);
    }
    for (uint32_t k = 0; k < 4; ++k) EXPECT(match_codes_word(r, k) == by_list[k], "count %u: decoded word %u", n, k);
    // the bytes behind the last code are zero: a consumer that shifts the record down reads code 0 there, never garbage
    for (uint32_t b = n + 1; b < 16; ++b) EXPECT(((b < 8 ? r.lo >> (8 * b) : r.hi >> (8 * (b - 8))) & 0xFF) == 0, "count %u: byte %u", n, b);
  }
  // ---- the extremes of a code: list 3, bit 63 in the last byte; list 0, bit 0 in the first
  {
    MatchCodes r{0, 0};
    match_codes_append(r, match_code(0, 0));
    for (uint32_t i = 1; i < 14; ++i) match_codes_append(r, match_code(1, i));
    match_codes_append(r, match_code(3, 63));
    EXPECT(match_codes_count(r) == 15 && match_code_at(r, 14) == 0xFFu && (r.hi >> 56) == 0xFFu, "the last byte");
    EXPECT(match_code_at(r, 0) == 0u && match_codes_word(r, 0) == 1ull && match_codes_word(r, 3) == 1ull << 63, "extremes");
    EXPECT(match_codes_header(r) != kMatchCodesOverflow, "15 codes are no overflow (code 0xFF sits in byte 15, not in the header)");
  }
  // ---- 16 and more: the overflow header, for good
  for (uint32_t n = 16; n <= 40; n += 8) {
    MatchCodes r{0, 0};
    for (uint32_t i = 0; i < n; ++i) match_codes_append(r, match_code(i >> 4, i & 15u));
    EXPECT(match_codes_header(r) == kMatchCodesOverflow && match_codes_count(r) == 0, "%u codes: header %u", n, match_codes_header(r));
    for (uint32_t k = 0; k < 4; ++k) EXPECT(match_codes_word(r, k) == 0, "an overflow record names no term");
  }
  // ---- the run rule on hand-made masks
  {
    // runs: [0], [1..3], [4], [5..6], singles up to 61, [62..63]
    uint64_t lo = ~0ull, hi = ~0ull;
    lo &= ~((1ull << 2) | (1ull << 3) | (1ull << 6) | (1ull << 63));
    hi &= ~((1ull << 1) | (1ull << 2) | (1ull << 5) | (1ull << 62));
    EXPECT(match_run_rule(0b1110ull, lo, hi) == 0b0010ull, "all of a run: its lowest");
    EXPECT(match_run_rule(0b1100ull, lo, hi) == 0b0100ull, "the upper two of a run");
    EXPECT(match_run_rule(0b1000ull, lo, hi) == 0b1000ull, "the last of a run");
    EXPECT(match_run_rule(0b1111111ull, lo, hi) == 0b0110011ull, "neighbouring runs do not merge");
    EXPECT(match_run_rule(3ull << 62, lo, hi) == 1ull << 62, "a run at the top of the word");
    EXPECT(match_run_rule(1ull << 63, lo, hi) == 1ull << 63, "... its last term alone");
    EXPECT(match_run_rule(0, lo, hi) == 0, "nothing matched");
    EXPECT(match_run_rule(~0ull, ~0ull, ~0ull) == ~0ull, "runs of one: the rule keeps everything");
    std::mt19937_64 rng(7);
    for (int it = 0; it < 20000; ++it) {
      // random runs over the low `real` bits (the rest: padding, in no run and never matched)
      const int real = 1 + (int)(rng() % 64);
      uint64_t l = 0, h = 0;
      for (int k = 0; k < real;) {
        const int len = 1 + (int)(rng() % 5), e = std::min(real - 1, k + len - 1);
        l |= 1ull << k, h |= 1ull << e;
        k = e + 1;
      }
      const uint64_t mask = real == 64 ? ~0ull : (1ull << real) - 1ull;
      const uint64_t x = rng() & rng() & mask;
      const uint64_t got = match_run_rule(x, l, h), want = run_rule_slow(x, l, h);
      EXPECT(got == want, "run rule: x %016llx lo %016llx hi %016llx: %016llx, want %016llx", (unsigned long long)x, (unsigned long long)l,
             (unsigned long long)h, (unsigned long long)got, (unsigned long long)want);
      // ... and through a record: four words of it
      MatchCodes r{0, 0};
      uint64_t w[4];
      uint32_t total = 0;
      for (uint32_t k = 0; k < 4; ++k) {
        w[k] = k == 0 ? got : match_run_rule(rng() & rng() & rng() & mask, l, h);
        total += (uint32_t)__builtin_popcountll(w[k]);
        match_codes_append_word(r, k, w[k]);
      }
      if (total <= kMatchCodesMax) {
        EXPECT(match_codes_count(r) == total, "record of %u terms: header %u", total, match_codes_header(r));
        for (uint32_t k = 0; k < 4; ++k) EXPECT(match_codes_word(r, k) == w[k], "record of %u terms: word %u", total, k);
        for (uint32_t i = 1; i < total; ++i) EXPECT(match_code_at(r, i) > match_code_at(r, i - 1), "ascending");
      } else {
        EXPECT(match_codes_header(r) == kMatchCodesOverflow, "record of %u terms: header %u", total, match_codes_header(r));
      }
    }
  }
  if (g_fail) {
    printf("match_codes_test: %d expectations failed\n", g_fail);
    return 1;
  }
  printf("match_codes_test: ok\n");
  return 0;
}
