// pack_plan_headroom_test.cpp — make_pack_plan with the headroom as a parameter (kt_index.h): the 9-bit plans of the two-per-CU
// aggregate scan, summed over up to 512 slabs the way block_record_sums does (whole words, class by class), against exact sums.
// The 8-bit plans stay with index_sim_test.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "kt_index.h"

using namespace kt;

static int g_fail = 0;
static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {  // splitmix64
  uint64_t z = (g_s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main() {
  int packed = 0, refused = 0, three = 0;
  for (int it = 0; it < 4000; ++it) {
    const int H = it % 4 == 3 ? kPackHeadroomBits : kPackHeadroomBitsTwo;
    const int D = 1 + (int)(rng() % 8);
    const uint64_t n_slab = 1 + rng() % 4000;
    const int n_slabs = it % 7 == 0 ? (1 << H) : 1 + (int)(rng() % (1u << H));
    unsigned __int128 max_abs[16] = {0};
    uint64_t or_abs[16] = {0};
    for (int d = 0; d < D; ++d) {
      const int kind = (int)(rng() % 5);
      if (kind == 0) continue;
      const int unit = kind == 1 ? 0 : (int)(rng() % 30);
      const int bits = 1 + (int)(rng() % (kind == 4 ? 44 : 12));
      const uint64_t x = ((rng() & ((1ull << bits) - 1ull)) | 1ull) << unit;
      max_abs[d] = x, or_abs[d] = x;
    }
    const uint32_t max_words = it % 3 == 0 ? 4u : 3u;
    const PackPlan pk = make_pack_plan(D, max_abs, or_abs, false, n_slab, /*pad_odd=*/false, max_words, H);
    if (pk.nw == 0) {
      ++refused;
      continue;
    }
    ++packed;
    if (pk.nw == 3) ++three;
    if (pk.headroom != (uint32_t)H || pk.nw > max_words || pk.rec_bytes != (pk.nw + 1) * 8u)
      ++g_fail, fprintf(stderr, "FAIL: plan shape nw=%u rec=%u headroom=%u (case %d)\n", pk.nw, pk.rec_bytes, pk.headroom, it);
    if (pk.cnt_width < (uint32_t)H || pk.cnt_width > 64u - (uint32_t)H || (pk.cnt_width < 64 && (n_slab >> pk.cnt_width) != 0))
      ++g_fail, fprintf(stderr, "FAIL: the pod count field (case %d)\n", it);
    for (int d = 0; d < D; ++d)
      if (pk.width[d] && (pk.width[d] < H || pk.width[d] > 64 - H)) ++g_fail, fprintf(stderr, "FAIL: field width %u with %d bits of headroom\n", pk.width[d], H);
    // every slab holds a full workgroup of the per-dimension maxima: the worst case the headroom has to hold
    uint64_t cls[8][3] = {};
    std::vector<unsigned __int128> want(D, 0);
    unsigned __int128 want_pods = 0;
    for (int sl = 0; sl < n_slabs; ++sl) {
      uint64_t acc[8] = {n_slab, 0, 0, 0, 0, 0, 0, 0};
      for (int d = 0; d < D; ++d)
        if (pk.width[d]) {
          acc[pk.word[d]] += (uint64_t)((unsigned __int128)((uint64_t)max_abs[d] >> pk.shift[d]) * n_slab) << pk.pos[d];
          want[d] += max_abs[d] * (unsigned __int128)n_slab;
        }
      want_pods += n_slab;
      for (uint32_t k = 0; k < pk.nw; ++k) {
        const uint64_t low = (1ull << pk.top_pos[k]) - 1ull;
        cls[k][0] += acc[k] & pk.even[k] & low, cls[k][1] += acc[k] & ~pk.even[k] & low, cls[k][2] += acc[k] >> pk.top_pos[k];
      }
    }
    auto field = [&](uint32_t desc) -> unsigned __int128 {  // packed_field (kt_index_device.h)
      const uint32_t sel = desc & 31u, pos = (desc >> 8) & 63u, wext = (desc >> 16) & 127u, shift = (desc >> 24) & 63u;
      if (!wext) return 0;
      return (unsigned __int128)((cls[sel >> 2][sel & 3u] >> pos) & (wext >= 64 ? ~0ull : (1ull << wext) - 1ull)) << shift;
    };
    if (field(pk.cnt_desc) != want_pods) ++g_fail, fprintf(stderr, "FAIL: packed pod count (case %d, %d slabs)\n", it, n_slabs);
    for (int d = 0; d < D; ++d)
      if (field(pk.desc[d]) != want[d]) { ++g_fail, fprintf(stderr, "FAIL: packed sum of dimension %d differs (case %d, %d slabs, headroom %d)\n", d, it, n_slabs, H); break; }
  }
  {  // a field of 56 bits packs with 8 bits of headroom and not with 9; the default is 8
    unsigned __int128 mx[16] = {((unsigned __int128)1 << 45) + 1};
    uint64_t oa[16] = {(1ull << 45) + 1};
    const PackPlan p8 = make_pack_plan(1, mx, oa, false, 1500, false), p9 = make_pack_plan(1, mx, oa, false, 1500, false, 4, kPackHeadroomBitsTwo);
    if (p8.nw == 0 || p8.headroom != (uint32_t)kPackHeadroomBits || p8.width[0] != 56) ++g_fail, fprintf(stderr, "FAIL: the 56-bit field with 8 bits of headroom\n");
    if (p9.nw != 0) ++g_fail, fprintf(stderr, "FAIL: a 56-bit field packed with 9 bits of headroom\n");
  }
  if (packed < 1000 || refused < 10 || three < 50)
    ++g_fail, fprintf(stderr, "FAIL: cases too one-sided (%d packed, %d refused, %d of three words)\n", packed, refused, three);
  printf("pack plan headroom: %d packed (%d of three words), %d refused\n", packed, three, refused);
  printf(g_fail ? "FAILED (%d)\n" : "ok\n", g_fail);
  return g_fail ? 1 : 0;
}
