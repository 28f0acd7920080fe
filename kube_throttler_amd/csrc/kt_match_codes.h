// kt_match_codes.h — the match-code record: a pod's matched terms of the match cache as one 16-byte record (host and device).
//
// The planes of the match cache (kt_scan.h) spend 64 bits per list position on the two or three terms a pod matches.  The
// record names the same terms, AFTER the consumer's run rule (a throttle with several terms is reported once: the lowest
// match of every run), as a count and up to 15 one-byte codes:
//   byte 0       the count 0..15, or kMatchCodesOverflow: more than 15 terms — this row is replayed from the planes
//   bytes 1..15  code = k << 6 | bit: k < kMatchCodeLists the position in the namespace's word list (the plane), bit the term's
//                bit in that word; ascending (k, bit), the order in which replay_tile's peel meets them
// Derived from the planes and the program's run masks and from nothing else: written where the planes are written
// (kt_build_match_cache), void where they are void.  The planes stay the authoritative table.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KT_MC_HD __host__ __device__ inline
#else
#define KT_MC_HD inline
#endif

namespace kt {

constexpr uint32_t kMatchCodesMax = 15;           // codes a record holds
constexpr uint32_t kMatchCodesOverflow = 0xFFu;   // header of a row with more
constexpr uint32_t kMatchCodeLists = 4;           // list positions a code can name (= kMatchReplay: kt_index.h asserts it)

struct alignas(16) MatchCodes {
  uint64_t lo, hi;  // bytes 0..7, 8..15
};

// The run rule of the wordwise consumers: of the matched terms x of one word, the lowest of every run [seg_lo bit .. seg_hi bit]
// (a run = the consecutive numbers of one throttle's terms; a term by itself is a run of one; runs never straddle a word).
KT_MC_HD uint64_t match_run_rule(uint64_t x, uint64_t seg_lo, uint64_t seg_hi) {
  const uint64_t v = x | seg_hi;
  return x & ~(v - seg_lo);
}

KT_MC_HD uint32_t match_codes_header(const MatchCodes& r) { return (uint32_t)(r.lo & 0xFFu); }
// codes of the record (0 for an overflow record: its bytes say nothing)
KT_MC_HD uint32_t match_codes_count(const MatchCodes& r) {
  const uint32_t h = match_codes_header(r);
  return h == kMatchCodesOverflow ? 0u : h;
}
KT_MC_HD uint32_t match_code_at(const MatchCodes& r, uint32_t i) {  // i < count
  const uint32_t b = i + 1u;
  return (uint32_t)((b < 8u ? r.lo >> (8u * b) : r.hi >> (8u * (b - 8u))) & 0xFFu);
}
KT_MC_HD uint32_t match_code(uint32_t k, uint32_t bit) { return k << 6 | bit; }
KT_MC_HD uint32_t match_code_list(uint32_t code) { return code >> 6; }
KT_MC_HD uint32_t match_code_bit(uint32_t code) { return code & 63u; }

// one more code behind those the record holds (callers append in ascending order); the sixteenth makes the record an overflow
// record, which stays one whatever follows
KT_MC_HD void match_codes_append(MatchCodes& r, uint32_t code) {
  const uint32_t h = match_codes_header(r);
  if (h == kMatchCodesOverflow) return;
  if (h >= kMatchCodesMax) {
    r.lo |= kMatchCodesOverflow;
    return;
  }
  const uint32_t b = h + 1u;
  if (b < 8u) r.lo |= (uint64_t)(code & 0xFFu) << (8u * b);
  else r.hi |= (uint64_t)(code & 0xFFu) << (8u * (b - 8u));
  r.lo += 1ull;  // (the count: byte 0 never carries, h < 15)
}
// the terms x of list position k (already through the run rule), lowest bit first
KT_MC_HD void match_codes_append_word(MatchCodes& r, uint32_t k, uint64_t x) {
  while (x) {
    uint32_t bit = 0;
    for (uint64_t t = x; !(t & 1ull); t >>= 1) ++bit;
    x &= x - 1ull;
    match_codes_append(r, match_code(k, bit));
  }
}
// decode: the terms of list position k the record names (an overflow record names none: its row is read from the planes)
KT_MC_HD uint64_t match_codes_word(const MatchCodes& r, uint32_t k) {
  uint64_t x = 0;
  const uint32_t n = match_codes_count(r);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t c = match_code_at(r, i);
    if (match_code_list(c) == k) x |= 1ull << match_code_bit(c);
  }
  return x;
}

}  // namespace kt
