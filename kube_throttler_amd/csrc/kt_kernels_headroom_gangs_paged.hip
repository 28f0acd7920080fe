// kt_kernels_headroom_gangs_paged.hip — how many copies of a whole gang the throttles still admit, over PAGES of resource names
// (kt_paged_headroom_gangs), gfx950.
//
// The definition is kt_kernels_headroom_gangs.hip's on the cluster of all names; a page is an engine of <= 16 names that holds
// every pod row and every throttle row (kt_engine.h, "PAGES").  headroom(gang, cap) is the number of leading admitted gangs of a
// dry kt_paged_admit_gangs over `cap` consecutive copies of the gang.  An admitted copy reserves on every page: each page its own
// names' values and the presence of the names a member carries there; the pod count is judged once, on page 0.  Copy j passes on
// throttle t iff the in-order member walk passes on EVERY page, each page against its own stored reserved row plus j * A_t of that
// page: passes_t(j) is an AND of monotone predicates and stays monotone, h_t = min_k h_{t,k}.  So every (throttle, page) pair is
// treated as a throttle of its own: the answer is the lexicographic minimum over the pairs of (h, first, t) — a tie in (h, first)
// keeps the lower row, and `first` is the minimum over the pages that stop there.
//
// kt_headroom_gangs_paged<DT> (DT: the bucket of the widest page) is kt_headroom_gangs' body with a page loop inside the throttle
// loop; the per-name register arrays are those of one page at a time, as in kt_preempt_gangs_paged.
//   per gang      (one wave, the grid strides) the first member whose PreFilter is an error (page 0's summary) or whose row is
//                 invalid (page 0's pod_flags) by a ballot over member blocks of 64; the UNION of the members' affecting throttles
//                 chunk by chunk through the 4 KiB LDS list, from page 0's matrix (the selector side is the same in every page).
//   per (t, page) that page's batch of wave-uniform loads: the threshold kt_admit reads ON THAT PAGE (admit_threshold: the page's
//                 own calculatedAt flag, nothing is reconciled), used, throttled flags, reserved.  Pages k != 0 hand the walk a
//                 threshold that does not name the count and a count flag of false (kt_preempt_gangs_paged's way; gang_walk is
//                 untouched).  Then A_t of the page from one member pass — which also says whether an affected member requests
//                 one of the page's names with a non-zero value at all (gang_page_requested's answer): a page k != 0 where none
//                 does is skipped, gang_walk compares only vp != 0 (and of those only names the threshold names or
//                 status.throttled flags can stop anybody) —, the range cut at the RUNNING
//                 minimum — it carries over pages as well as throttles: a pair that still passes at the best answer so far costs
//                 one walk — and per named amount of that page at (INT64_MAX - base) / per (the count's cut on page 0 only), the
//                 64-ary search with gang_walk over a GangPageView of the page, the strict lexicographic update.
//   output        kt_headroom_gangs': copies[g], blocker[g] (queue position, -1: all cap copies are admitted), limiting[g] (-1: no
//                 blocker, or the blocker's verdict is an Error).  A gang with an Error / invalid member: 0 copies, one walk of copy
//                 0 in front of that member per (t, page).  With one page the kernel computes what kt_headroom_gangs computes.
// The range of a pair, the rounds of the search and why no lane's state wraps: kt_kernels_headroom_gangs.hip.
// Every __ballot, __syncthreads and readfirstlane sits where the whole wave arrives: the loops over chunks, throttles, pages,
// rounds and members are wave-uniform.
#include "kt_preempt_paged_common.h"

namespace kt {

struct HeadroomGangsPagedArgs {
  const AdmitPage* pages;   // [n_pages] in device memory (the descriptors kt_admit reads; the state offsets are unused)
  int32_t n_pages;
  const int64_t* rows;      // [n] pod table rows (the same in every page): the members of all gangs
  const int64_t* gang_off;  // [n_gangs + 1] queue positions
  int64_t n_gangs;
  const uint8_t* status;    // [n][T] page 0's check
  const uint64_t* summary;  // [n]
  int64_t* copies;          // [n_gangs] out
  int32_t* limiting;        // [n_gangs] out
  int64_t* blocker;         // [n_gangs] out
  int32_t T, on_equal;
  uint32_t cap;  // 1 .. 2^31 - 1
};

constexpr int64_t kPagedInt64Max = 0x7FFFFFFFFFFFFFFFll;

// the candidates of one amount end at (INT64_MAX - base) / per: beyond, reserved + (j + 1) per has left int64 (per > 0)
__device__ __forceinline__ int64_t headroom_gang_paged_fit(int64_t base, int64_t per, int64_t top) {
  const uint64_t q = ((uint64_t)kPagedInt64Max - (uint64_t)base) / (uint64_t)per;  // (base may be negative: the difference fits 64 bits)
  return q < (uint64_t)top ? (int64_t)q : top;
}

// lane l's 64-bit value as a wave-uniform one (l is uniform: it comes out of a ballot)
__device__ __forceinline__ int64_t headroom_gang_paged_lane(int64_t x, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, l), hi = (uint32_t)__builtin_amdgcn_readlane((int)((uint64_t)x >> 32), l);
  return (int64_t)((uint64_t)hi << 32 | lo);
}

template <int DT>
__global__ __launch_bounds__(kWave) void kt_headroom_gangs_paged(const HeadroomGangsPagedArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int T = a.T, n_pages = a.n_pages;
  const bool eq = a.on_equal != 0;
  const int64_t cap = (int64_t)a.cap;
  const uint32_t* pod_flags0 = admit_page(a.pages, 0).pod_flags;
  for (int64_t gi = blockIdx.x; gi < a.n_gangs; gi += gridDim.x) {  // (wave-uniform: one gang per wave and turn)
    const int64_t i0 = a.gang_off[gi], i1 = a.gang_off[gi + 1];
    // the first member whose PreFilter is an error or whose row is invalid: copy 0 is not admitted, the walk ends in front of it
    int64_t bad = i1;
    for (int64_t j0 = i0; j0 < i1; j0 += kWave) {
      const int64_t j = j0 + lane;
      const uint64_t mk = __ballot(j < i1 && (a.summary[j] == 2ull || !(pod_flags0[a.rows[j]] & kPodValid)));
      if (mk != 0ull) {
        bad = j0 + (__ffsll((long long)mk) - 1);
        break;
      }
    }
    const bool err = bad < i1;
    // the lexicographic minimum of (h, first, t) over the (throttle, page) pairs so far (wave-uniform).  The row takes part in
    // the comparison: the chunk list is filled round by round over the lanes (admit_append_marked), not in row order
    int64_t best_h = err ? 0 : cap, best_first = bad;
    int32_t best_t = -1;
    for (int c0 = 0; c0 < T; c0 += kPreemptChunk) {
      bool err_c = false;  // (the error rows are the summary's: `bad` above)
      const uint32_t n_c = gang_affected_chunk(a.status, i0, i1, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
      __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
      for (uint32_t ai = 0; ai < n_c; ++ai) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[ai]);
        for (int k = 0; k < n_pages; ++k) {
          const GangPageView view{admit_page(a.pages, k), a.rows, a.status, T};
          const int D = view.pg.D, DS = view.pg.DS;
          const ThrTables& tt = view.pg.tt;
          const bool first_page = k == 0;
          // ---- the throttle's stored state on this page: one batch of wave-uniform loads
          const uint32_t tf = tt.flags[t];
          const AmountTab& th = admit_threshold(tt, tf);
          GangThr<DT> g;
          GangUsed<DT> u;
          g.eq = eq, g.eq3 = admit_eq3(tf, eq);
          // the pod count is page 0's: elsewhere the threshold does not name it
          g.th_hc = first_page && th.has_count[t] != 0, g.th_c = th.count[t], g.th_p = th.present[t];
          const bool r_hc = tt.reserved.has_count[t] != 0;
          const int64_t r_c = r_hc ? tt.reserved.count[t] : 0;
          const uint32_t r_p = tt.reserved.present[t];
          u.c_flag = first_page && (tf & kThrThrottledPod) != 0, u.u_hc = tt.used.has_count[t] != 0, u.u_c = tt.used.count[t];
          u.flag_m = tt.thrl_flag[t] & tt.thrl_has[t], u.pr_m = tt.used.present[t];
          // a page k != 0 on which the threshold names nothing and no name is flagged stops nobody, whatever the members ask
          const uint32_t judged = g.th_p | u.flag_m;  // the names some step of gang_walk can fail on
          if (!first_page && judged == 0u) continue;
          int64_t base[DT], per[DT];  // the page's stored reserved row (0 where absent) and A_t's values on this page
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
            first = gang_walk<DT>(view, t, i0, bad, g, u), h = 0;
            if (first >= bad) continue;
          } else {
            // ---- A_t of this page: one pass over the members.  Only what the threshold names is summed: the rest is never
            //      compared.  The same pass says whether anything of this page is compared at all (gang_page_requested's answer:
            //      the member's request row comes in with one batch of loads either way)
            int64_t per_c = 0;
            uint32_t per_p = 0, need = 0;
            for (int64_t i = i0; i < i1; ++i) {
              if (a.status[i * (int64_t)T + t] == 0) continue;
              const int64_t p = a.rows[i];
              const uint32_t present = (view.pg.pod_flags[p] >> kPresentShift) & ((1u << D) - 1u);
              per_c += 1, per_p |= present;
#pragma unroll
              for (int d = 0; d < DT; ++d) {
                if (d >= D) continue;
                const int64_t v = view.pg.req[p * DS + d];
                need |= v != 0 ? 1u << d : 0u;
                if (!(((present & g.th_p) >> d) & 1u)) continue;
                per[d] = v > kPagedInt64Max - per[d] ? kPagedInt64Max : per[d] + v;  // (saturated: the range then ends at copy 0 or 1)
              }
            }
            // (page 0 carries the pod count; elsewhere a page none of whose judged names an affected member requests with a
            // non-zero value stops nobody: gang_walk compares only vp != 0)
            if (!first_page && (need & judged) == 0u) continue;
            if (!g.th_hc) per_c = 0;
            // ---- the range: up to the running minimum over the pairs so far, and no further than every named amount of this
            //      page stays inside int64 (the count's cut applies where the count is judged: g.th_hc is false elsewhere)
            int64_t top = best_h < cap ? best_h : cap - 1;
            if (g.th_hc) top = headroom_gang_paged_fit(r_c, per_c, top);
#pragma unroll
            for (int d = 0; d < DT; ++d)
              if (per[d] > 0) top = headroom_gang_paged_fit(base[d], per[d], top);
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
              const int64_t f = gang_walk<DT>(view, t, i0, i1, g, u);
              const uint64_t mk = __ballot(in && f < i1);
              if (mk == 0ull) {  // every probe passes: so does everything below hi
                lo = hi + 1;
                if (!known) break;  // the pair passes at the running minimum: it changes nothing
                continue;
              }
              const int fl = __ffsll((long long)mk) - 1;
              top = headroom_gang_paged_lane(j, fl), first = headroom_gang_paged_lane(f, fl), known = true;
              const int64_t below = top - step;  // the candidate of the lane before: it passed
              if (fl > 0 && below >= lo) lo = below + 1;
            }
            if (!known) continue;
            h = top;
          }
          if (h < best_h || (h == best_h && (first < best_first || (first == best_first && (int32_t)t < best_t))))
            best_h = h, best_first = first, best_t = (int32_t)t;
        }
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

// pages: the descriptors as launch_headroom takes them; copied to pages_dev, pages_copied recorded behind the copy, as there.
// false: *hip_err says why
bool launch_headroom_gangs_paged(const AdmitPage* pages, int n_pages, AdmitPage* pages_dev, hipEvent_t pages_copied, int64_t n_gangs,
                                 const int64_t* rows_dev, const int64_t* gang_off_dev, int T, bool on_equal, uint32_t cap, const uint8_t* status,
                                 const uint64_t* summary, int64_t* copies, int32_t* limiting, int64_t* blocker, hipStream_t s,
                                 hipError_t* hip_err) {
  *hip_err = hipSuccess;
  if (n_gangs <= 0) return true;
  int maxD = 1;
  for (int k = 0; k < n_pages; ++k) maxD = pages[k].D > maxD ? pages[k].D : maxD;
  HeadroomGangsPagedArgs a{};
  a.pages = pages_dev, a.n_pages = n_pages, a.rows = rows_dev, a.gang_off = gang_off_dev, a.n_gangs = n_gangs, a.status = status;
  a.summary = summary, a.copies = copies, a.limiting = limiting, a.blocker = blocker, a.T = T, a.on_equal = on_equal ? 1 : 0, a.cap = cap;
  if ((*hip_err = hipMemcpyAsync(pages_dev, pages, sizeof(AdmitPage) * (size_t)n_pages, hipMemcpyHostToDevice, s)) != hipSuccess) return false;
  if ((*hip_err = hipEventRecord(pages_copied, s)) != hipSuccess) return false;
  const int blocks = (int)(n_gangs < kPreemptMaxBlocks ? n_gangs : kPreemptMaxBlocks);
  const int DT = dt_bucket(maxD);
  if (DT == 4) hipLaunchKernelGGL(kt_headroom_gangs_paged<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_headroom_gangs_paged<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_headroom_gangs_paged<16>, dim3(blocks), dim3(kWave), 0, s, a);
  return true;
}

}  // namespace kt
