// kt_kernels_headroom_gangs.hip — how many copies of a whole gang the throttles still admit (kt_headroom_gangs_launch), gfx950.
//
// kt_headroom (kt_kernels_headroom.hip) and gang_walk (kt_admit_common.h) turned towards each other.  headroom(gang, cap) is the
// number of leading admitted gangs of a dry kt_admit_gangs over `cap` consecutive copies of the gang.  Before the first copy that
// is rolled back every earlier copy was admitted in full, so copy j meets on throttle t the stored reserved row plus j * A_t,
// A_t = what one admitted copy reserves on t: one pod per member t affects, the value of every name such a member carries, the
// presence of all those names (zero-valued ones included) — and from copy 1 on the count and those names ARE present.  Given
// that, the throttles are independent: the answer is the minimum over the affecting throttles of h_t, the leading copies t alone
// lets through.  The members of a gang meet different throttles and reserve in front of each other, so there is no closed form
// as headroom_of_term; but with non-negative requests passes_t(j) is monotone in j (sums and presence only grow, the stored
// status.throttled flags do not depend on j): h_t is found by SEARCH, and the judge of every probe is gang_walk itself with the
// candidate's reserved row — the number is held to admission by construction.
//
//   input   status matrix and summary words of ONE check over the members of all gangs, the stored tables, the gang offsets.
//           All read-only; no reconcile, no aggregate, no dry finalize.
//   per gang (one wave, the grid strides) the first member whose PreFilter is an error or whose row is invalid by a ballot over
//           member blocks of 64; the UNION of the members' affecting throttles chunk by chunk through the 4 KiB LDS list; per
//           throttle one batch of wave-uniform loads (threshold by admit_threshold, used, throttled flags, reserved), A_t from
//           one pass over the members, then a 64-ary search: lane l fills a GangThr whose reserved row is that of its own
//           candidate j_l and calls gang_walk (the member loop is wave-uniform), a ballot narrows the range.
//   output  the lexicographic minimum of (h_t, first_t, t), first_t = gang_walk's answer for the probe j = h_t:
//           copies[g] = h; blocker[g] = the queue position of the first member of copy h that is not Success (-1: all cap copies
//           are admitted); limiting[g] = the lowest throttle row that stops that member at its turn (-1: no blocker, or the
//           blocker's verdict is an Error).  A gang with an Error / invalid member: 0 copies, the walk ends in front of that
//           member (an earlier member some throttle stops is the blocker).  A gang no throttle affects: cap, -1, -1.
//
// The range of a throttle.  Only candidates up to the running minimum h (cap - 1 while nothing binds) matter: a throttle that
// passes there changes nothing, and that is the FIRST round's top probe — one walk.  And no lane's state may wrap: for an amount
// the threshold names with A > 0, a copy j that passes has passed step 4 of the last member that asks for it, used + reserved +
// (j + 1) A <= threshold <= INT64_MAX (`used` is a sum of non-negative requests), so every candidate beyond
// J = (INT64_MAX - reserved) / A fails without a walk and the range ends at J: reserved + j A fits int64 for every probe.  (At
// j = J itself — a threshold within A of int64's end — gang_walk's own running sum passes int64 only behind the member that
// already failed, and `first` is settled by then.)  An amount the threshold does NOT name never decides (preempt_fails returns
// before it reads it): its row stays the stored one, nothing is multiplied into it.
//
// Rounds: n candidates, step = ceil(n / 64), lane l probes top - (63 - l) step; the first failing lane becomes the new top
// (known to fail, its `first` kept), the lane before it + 1 the new bottom: n < step afterwards.  cap = 2^31 - 1 takes six
// rounds (2^31 -> 2^25 -> 2^19 -> 2^13 -> 2^7 -> 2 -> 1), a running minimum below 64 one.
#include "kt_admit_common.h"

namespace kt {

struct HeadroomGangArgs {
  AdmitPage pg;             // pod flags, request rows and the throttle tables of the engine (state offsets unused)
  const int64_t* rows;      // [n] pod table rows: the members of all gangs
  const int64_t* gang_off;  // [n_gangs + 1] queue positions
  int64_t n_gangs;
  const uint8_t* status;    // [n][T]
  const uint64_t* summary;  // [n]
  int64_t* copies;          // [n_gangs] out
  int32_t* limiting;        // [n_gangs] out
  int64_t* blocker;         // [n_gangs] out
  int32_t T, on_equal;
  uint32_t cap;  // 1 .. 2^31 - 1
};

constexpr int64_t kInt64Max = 0x7FFFFFFFFFFFFFFFll;

// the candidates of one amount end at (INT64_MAX - base) / per: beyond, reserved + (j + 1) per has left int64 (per > 0)
__device__ __forceinline__ int64_t headroom_gang_fit(int64_t base, int64_t per, int64_t top) {
  const uint64_t q = ((uint64_t)kInt64Max - (uint64_t)base) / (uint64_t)per;  // (base may be negative: the difference fits 64 bits)
  return q < (uint64_t)top ? (int64_t)q : top;
}

// lane l's 64-bit value as a wave-uniform one (l is uniform: it comes out of a ballot)
__device__ __forceinline__ int64_t headroom_gang_lane(int64_t x, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)((uint64_t)x >> 32), l);
  return (int64_t)((uint64_t)hi << 32 | lo);
}

template <int DT>
__global__ __launch_bounds__(kWave) void kt_headroom_gangs(const HeadroomGangArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int T = a.T, D = a.pg.D, DS = a.pg.DS;
  const bool eq = a.on_equal != 0;
  const ThrTables& tt = a.pg.tt;
  const int64_t cap = (int64_t)a.cap;
  for (int64_t gi = blockIdx.x; gi < a.n_gangs; gi += gridDim.x) {  // (wave-uniform: one gang per wave and turn)
    const int64_t i0 = a.gang_off[gi], i1 = a.gang_off[gi + 1];
    // the first member whose PreFilter is an error or whose row is invalid: copy 0 is not admitted, the walk ends in front of it
    int64_t bad = i1;
    for (int64_t j0 = i0; j0 < i1; j0 += kWave) {
      const int64_t j = j0 + lane;
      const uint64_t mk = __ballot(j < i1 && (a.summary[j] == 2ull || !(a.pg.pod_flags[a.rows[j]] & kPodValid)));
      if (mk != 0ull) {
        bad = j0 + (__ffsll((long long)mk) - 1);
        break;
      }
    }
    const bool err = bad < i1;
    // the lexicographic minimum of (h_t, first_t, t) over the throttles so far (wave-uniform).  The row takes part in the
    // comparison: the chunk list is filled round by round over the lanes (admit_append_marked), not in row order
    int64_t best_h = err ? 0 : cap, best_first = bad;
    int32_t best_t = -1;
    for (int c0 = 0; c0 < T; c0 += kPreemptChunk) {
      bool err_c = false;  // (the error rows are the summary's: `bad` above)
      const uint32_t n_c = gang_affected_chunk(a.status, i0, i1, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
      __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
      for (uint32_t ai = 0; ai < n_c; ++ai) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[ai]);
        // ---- the throttle's stored state: one batch of wave-uniform loads
        const uint32_t tf = tt.flags[t];
        const AmountTab& th = admit_threshold(tt, tf);
        GangThr<DT> g;
        GangUsed<DT> u;
        g.eq = eq, g.eq3 = admit_eq3(tf, eq);
        g.th_hc = th.has_count[t] != 0, g.th_c = th.count[t], g.th_p = th.present[t];
        const bool r_hc = tt.reserved.has_count[t] != 0;
        const int64_t r_c = r_hc ? tt.reserved.count[t] : 0;
        const uint32_t r_p = tt.reserved.present[t];
        u.c_flag = (tf & kThrThrottledPod) != 0, u.u_hc = tt.used.has_count[t] != 0, u.u_c = tt.used.count[t];
        u.flag_m = tt.thrl_flag[t] & tt.thrl_has[t], u.pr_m = tt.used.present[t];
        int64_t base[DT], per[DT];  // the stored reserved row (0 where absent) and A_t's values
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          g.tv[d] = base[d] = per[d] = u.u_v[d] = 0;
          if (d >= D) continue;
          g.tv[d] = th.v[(size_t)t * D + d], u.u_v[d] = tt.used.v[(size_t)t * D + d];
          base[d] = ((r_p >> d) & 1u) ? tt.reserved.v[(size_t)t * D + d] : 0;
        }
        int64_t first, h;
        if (err) {  // copy 0 alone, in front of the Error member
          g.r_hc = r_hc, g.r_c = r_c, g.r_p = r_p;
#pragma unroll
          for (int d = 0; d < DT; ++d) g.rv[d] = base[d];
          first = gang_walk<DT>(a, t, i0, bad, g, u), h = 0;
          if (first >= bad) continue;
        } else {
          // ---- A_t: one pass over the members.  Only what the threshold names is summed: the rest is never compared
          int64_t per_c = 0;
          uint32_t per_p = 0;
          for (int64_t i = i0; i < i1; ++i) {
            if (a.status[i * (int64_t)T + t] == 0) continue;
            const int64_t p = a.rows[i];
            const uint32_t present = (a.pg.pod_flags[p] >> kPresentShift) & ((1u << D) - 1u);
            per_c += 1, per_p |= present;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              if (d >= D || !(((present & g.th_p) >> d) & 1u)) continue;
              const int64_t v = a.pg.req[p * DS + d];
              per[d] = v > kInt64Max - per[d] ? kInt64Max : per[d] + v;  // (saturated: the range then ends at copy 0 or 1)
            }
          }
          if (!g.th_hc) per_c = 0;
          // ---- the range: up to the running minimum, and no further than every named amount stays inside int64
          int64_t top = best_h < cap ? best_h : cap - 1;
          if (g.th_hc) top = headroom_gang_fit(r_c, per_c, top);
#pragma unroll
          for (int d = 0; d < DT; ++d)
            if (per[d] > 0) top = headroom_gang_fit(base[d], per[d], top);
          // ---- the 64-ary search for the first candidate in [lo, top] that fails; `known`: top itself has been seen to fail
          int64_t lo = 0;
          bool known = false;
          first = i1;
          for (;;) {
            const int64_t hi = known ? top - 1 : top;  // the highest candidate still to probe
            const int64_t n = hi - lo + 1;
            if (n <= 0) break;
            const int64_t step = (n + kWave - 1) / kWave;
            const int64_t j = hi - (int64_t)(kWave - 1 - lane) * step;
            const bool in = j >= lo;
            const int64_t jj = in ? j : lo;  // (an idle lane walks a candidate of the range: its state fits too)
            g.r_hc = r_hc || jj > 0, g.r_c = r_c + jj * per_c, g.r_p = jj > 0 ? r_p | per_p : r_p;
#pragma unroll
            for (int d = 0; d < DT; ++d) g.rv[d] = base[d] + jj * per[d];
            const int64_t f = gang_walk<DT>(a, t, i0, i1, g, u);
            const uint64_t mk = __ballot(in && f < i1);
            if (mk == 0ull) {  // every probe passes: so does everything below hi
              lo = hi + 1;
              if (!known) break;  // the throttle passes at the running minimum: it changes nothing
              continue;
            }
            const int fl = __ffsll((long long)mk) - 1;
            top = headroom_gang_lane(j, fl), first = headroom_gang_lane(f, fl), known = true;
            const int64_t below = top - step;  // the candidate of the lane before: it passed
            if (fl > 0 && below >= lo) lo = below + 1;
          }
          if (!known) continue;
          h = top;
        }
        if (h < best_h || (h == best_h && (first < best_first || (first == best_first && (int32_t)t < best_t))))
          best_h = h, best_first = first, best_t = (int32_t)t;
      }
      __syncthreads();  // the next chunk rewrites the list
    }
    if (lane == 0) {
      const bool none = !err && best_h >= cap;  // all cap copies are admitted
      a.copies[gi] = best_h;
      a.blocker[gi] = none ? -1 : best_first;
      a.limiting[gi] = none ? -1 : best_t;
    }
  }
}

void launch_headroom_gangs(const AdmitPage& pg, int64_t n_gangs, const int64_t* rows_dev, const int64_t* gang_off_dev, int T, bool on_equal,
                           uint32_t cap, const uint8_t* status, const uint64_t* summary, int64_t* copies, int32_t* limiting, int64_t* blocker,
                           hipStream_t s) {
  if (n_gangs <= 0) return;
  HeadroomGangArgs a{};
  a.pg = pg, a.rows = rows_dev, a.gang_off = gang_off_dev, a.n_gangs = n_gangs, a.status = status, a.summary = summary;
  a.copies = copies, a.limiting = limiting, a.blocker = blocker, a.T = T, a.on_equal = on_equal ? 1 : 0, a.cap = cap;
  const int blocks = (int)(n_gangs < kPreemptMaxBlocks ? n_gangs : kPreemptMaxBlocks);
  const int DT = dt_bucket(pg.D);
  if (DT == 4) hipLaunchKernelGGL(kt_headroom_gangs<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_headroom_gangs<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_headroom_gangs<16>, dim3(blocks), dim3(kWave), 0, s, a);
}

}  // namespace kt
