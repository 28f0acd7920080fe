// kt_kernels_preempt_gangs_paged.hip — a gang's victim prefix and its reprieve pass over PAGES of resource names
// (kt_paged_preempt_gangs), gfx950.
//
// The definitions are kt_kernels_preempt_gangs.hip's and kt_kernels_preempt_gangs_reprieve.hip's on the cluster of all names; a page
// is an engine of <= 16 names that holds every pod row and every throttle row (kt_engine.h, "PAGES").  What the pages share is judged
// once, what is per name is judged page by page, and the verdicts meet before anything is decided — the rules of
// kt_kernels_preempt_paged.hip (ONE check of page 0 over members ++ candidates, the pod count on page 0, stored and use-calc by the
// OR over the pages, a stored throttle reads the STORED calculated threshold) and the gang's own:
//   * an admitted member reserves on EVERY page: each page carries its own reserved prefix, from that page's stored reserved row,
//     and a member the throttle affects adds its value of every name of that page it carries, the presence of ALL of them
//     (that page's pod_flags) and, on page 0, count + 1;
//   * the gang passes in S_k iff for every throttle of the union the in-order member walk passes on page 0 with the count part and
//     passes the name part on every page.  Judging member j with the reservations of all earlier affected members stays exact:
//     the gang passes only if every member passes every page;
//   * blocker: the minimum over throttles AND pages of the first stopped queue position in S_0 (the first member that stops on
//     some page has met exact reserved prefixes on that page, and no page stops an earlier one).
// The member walk is gang_walk (kt_admit_common.h) with one page's rows at a time.  The count part is left to page 0 by handing the
// other pages a throttle whose threshold does not name the count and whose count is not flagged: preempt_fails passes that amount
// at once, and gang_walk itself is untouched.
//
// kt_preempt_gangs_paged<DT> (DT: the bucket of the widest page): one wave per gang, lane = candidate position, as kt_preempt_gangs.
//   The union list comes chunk by chunk through the 4 KiB LDS list (gang_affected_chunk on page 0's matrix).  Per throttle first the
//   wave-uniform facts, then page by page the k = 0 judgement, the 64-wide blocks of candidates with THAT page's carries and
//   gang_walk with that page's rows; the per-name register arrays are those of one page at a time.  A page k != 0 is skipped when no
//   affected member requests one of its names under either threshold (a row that keeps its stored status: when no affected member
//   requests one of its names at all).  Fail bits OR into the lane's own victim byte; the candidates a throttle matches are marked
//   once, on page 0; preempt_answer runs once.
// kt_preempt_gangs_reprieve_paged<DT, IN_LDS>: one wave per gang, lanes = list entries, as kt_preempt_gangs_reprieve.  The entry state
//   is kt_preempt_reprieve_paged's over the flat name index F = sum of the pages' D (bit 31 of a throttle row caches use-calc).  The
//   names whose state is kept are, per page, those some member requests (wave-uniform).  The judge of a candidate loops over the
//   pages inside the lane before the ONE ballot — per page GangThr / GangUsed from the state at fb + d, then gang_walk with the lane's
//   own throttle row — and the commit pass updates every page's fields.  No lane indexes private memory dynamically.
#include "kt_preempt_paged_common.h"

namespace kt {

struct GangsPagedArgs {
  const int64_t* gang_off;  // [n_gangs + 1] queue positions
  int64_t n_gangs;
  int64_t* blocker;         // [n_gangs] out (the prefix kernel)
};

template <int DT>
__global__ __launch_bounds__(kWave) void kt_preempt_gangs_paged(const PreemptPagedArgs a, const GangsPagedArgs ga) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int T = a.T;
  const bool eq = a.on_equal != 0;
  const int64_t m = a.m;
  const PreemptArgs a0 = preempt_page_args(a, 0);
  const int64_t m_eff = preempt_m_eff(a0, lane);  // (validity and the error rows are the same in every page)
  for (int64_t gi = blockIdx.x; gi < ga.n_gangs; gi += gridDim.x) {  // (wave-uniform: one gang per wave and turn)
    const int64_t i0 = ga.gang_off[gi], i1 = ga.gang_off[gi + 1];
    uint8_t* vic = a.victims + gi * m;
    for (int64_t q = lane; q < m; q += kWave) vic[q] = 0;
    // the first member whose PreFilter is an error or whose row is invalid: the gang has no prefix, and it is not Success in S_0
    int64_t block0 = i1;  // the first member that is not Success when the gang is walked in S_0
    for (int64_t j0 = i0; j0 < i1; j0 += kWave) {
      const int64_t j = j0 + lane;
      const uint64_t mk = __ballot(j < i1 && (a.summary[j] == 2ull || !(a0.pg.pod_flags[a.rows[j]] & kPodValid)));
      if (mk != 0ull) {
        block0 = j0 + (__ffsll((long long)mk) - 1);
        break;
      }
    }
    bool never = block0 < i1;  // no S_k lets the gang through
    bool fail0 = false;        // some (member, throttle, page, amount) stops the gang in S_0
    for (int c0 = 0; c0 < T; c0 += kPreemptChunk) {
      bool err_c = false;
      const uint32_t n_c = gang_affected_chunk(a.status, i0, i1, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
      never |= __ballot(err_c) != 0ull;
      __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
      for (uint32_t ai = 0; ai < n_c; ++ai) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[ai]);
        bool stored, use_calc;
        paged_thr_facts(a.pages, a.n_pages, t, &stored, &use_calc);
        for (int k = 0; k < a.n_pages; ++k) {
          const PreemptArgs ak = preempt_page_args(a, k);
          const int D = ak.pg.D;
          const ThrTables& tt = ak.pg.tt;
          const uint32_t tf = tt.flags[t];
          // a stored row reads the STORED calculated threshold: a page whose own reconcile were no error would report a fresh one
          const AmountTab& th = use_calc ? (stored ? tt.calc : ak.calc) : tt.spec;
          const bool first_page = k == 0;
          const uint32_t c_p = ak.calc.present[t];
          uint32_t need = gang_page_requested(ak.pg, a.rows, a.status, T, t, i0, i1);
          if (!stored) need &= th.present[t] | c_p;  // the other names pass every step of every member
          if (!first_page && need == 0) continue;    // nothing of this page can fail, and page 0 marks the matched candidates
          GangThr<DT> g;
          g.eq = eq, g.eq3 = admit_eq3(tf, eq);
          // the pod count is page 0's: elsewhere the threshold does not name it
          g.th_hc = first_page && th.has_count[t] != 0, g.r_hc = tt.reserved.has_count[t] != 0;
          g.th_c = th.count[t], g.r_c = tt.reserved.count[t];
          g.th_p = th.present[t], g.r_p = tt.reserved.present[t];
          const bool c_hc = first_page && ak.calc.has_count[t] != 0;
          const int64_t c_c = ak.calc.count[t];
          const unsigned long long* prow = ak.partial + (size_t)t * partial_stride(D);
          const int64_t pods_total = (int64_t)prow[partial_off_pods(D)];
          int64_t cv[DT], tot_v[DT], tot_c[DT];
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            g.tv[d] = g.rv[d] = cv[d] = tot_v[d] = tot_c[d] = 0;
            if (d >= D) continue;
            g.tv[d] = th.v[(size_t)t * D + d], g.rv[d] = tt.reserved.v[(size_t)t * D + d];
            if (!((need >> d) & 1u)) continue;
            cv[d] = ak.calc.v[(size_t)t * D + d];
            tot_v[d] = (int64_t)prow[d], tot_c[d] = (int64_t)prow[partial_off_presence(D) + d];
          }
          GangUsed<DT> u;
          if (stored) {  // this page's stored status, in every S_k
            u.c_flag = first_page && (tf & kThrThrottledPod) != 0, u.u_hc = tt.used.has_count[t] != 0, u.u_c = tt.used.count[t];
            u.flag_m = tt.thrl_flag[t] & tt.thrl_has[t], u.pr_m = tt.used.present[t];
#pragma unroll
            for (int d = 0; d < DT; ++d) u.u_v[d] = d < D ? tt.used.v[(size_t)t * D + d] : 0;
            const int64_t first = gang_walk<DT>(ak, t, i0, i1, g, u);
            never |= first < i1;
            block0 = first < block0 ? first : block0;
          } else {  // k = 0
            u.u_hc = pods_total > 0, u.u_c = pods_total, u.c_flag = c_hc && u.u_hc && pods_total >= c_c;
            u.flag_m = u.pr_m = 0u;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              u.u_v[d] = tot_v[d];
              if (!((need >> d) & 1u)) continue;
              const bool u_pr = tot_c[d] > 0;
              u.pr_m |= u_pr ? 1u << d : 0u;
              u.flag_m |= (((c_p >> d) & 1u) && u_pr && tot_v[d] >= cv[d]) ? 1u << d : 0u;
            }
            const int64_t first = gang_walk<DT>(ak, t, i0, i1, g, u);
            fail0 |= first < i1;
            block0 = first < block0 ? first : block0;
          }
          if (stored && !first_page) continue;  // nothing of it depends on k, and page 0 marks the matched candidates
          // every k >= 1, 64 positions at a time, with this page's carries: the scans once, then the members
          int64_t car_v[DT], car_pods = 0;
          uint32_t car_c[DT];
#pragma unroll
          for (int d = 0; d < DT; ++d) car_v[d] = 0, car_c[d] = 0u;
          for (int64_t q0 = 0; q0 < m_eff && !never; q0 += kWave) {
            const int64_t q = q0 + lane;
            const PreemptCand L = preempt_cand(ak, t, q, m_eff);  // (fl: THIS page's presence bits)
            bool f = false;
            if (!stored) {
              GangUsed<DT> uk;
              uk.u_c = 0, uk.u_hc = false, uk.c_flag = false;
              if (first_page) {
                const int64_t pre_pods = preempt_scan_pods(L, lane, car_pods);
                uk.u_c = pods_total - pre_pods, uk.u_hc = uk.u_c > 0, uk.c_flag = c_hc && uk.u_hc && uk.u_c >= c_c;
              }
              uk.flag_m = uk.pr_m = 0u;
#pragma unroll
              for (int d = 0; d < DT; ++d) {
                uk.u_v[d] = 0;
                if (!((need >> d) & 1u)) continue;  // (wave-uniform)
                int64_t pre_v;
                uint32_t pre_c;
                preempt_scan_name(ak, L, d, lane, car_v[d], car_c[d], &pre_v, &pre_c);
                // presence is exact: the name stays in `used` only while a remaining counted pod carries it
                const bool u_pr = tot_c[d] - (int64_t)pre_c > 0;
                uk.u_v[d] = tot_v[d] - pre_v;
                uk.pr_m |= u_pr ? 1u << d : 0u;
                uk.flag_m |= (((c_p >> d) & 1u) && u_pr && uk.u_v[d] >= cv[d]) ? 1u << d : 0u;
              }
              f = gang_walk<DT>(ak, t, i0, i1, g, uk) < i1;
            }
            const bool mark = first_page && L.contrib;
            if (L.in && (mark || f)) vic[q] |= (uint8_t)((mark ? 1u : 0u) | (f ? 2u : 0u));
          }
        }
      }
      __syncthreads();  // the next chunk rewrites the list
    }
    const int64_t ans = preempt_answer(vic, m, m_eff, !never, fail0, lane);
    if (lane == 0) {
      a.prefix[gi] = ans;
      ga.blocker[gi] = (ans == 0 || block0 >= i1) ? -1 : block0;
    }
  }
}

bool launch_preempt_gangs_paged(const PreemptPage* pages, int n_pages, PreemptPage* pages_dev, hipEvent_t pages_copied, int64_t n, int64_t m,
                                const int64_t* rows_dev, int64_t n_gangs, const int64_t* gang_off_dev, int T, bool on_equal, const uint8_t* status,
                                const uint64_t* summary, int64_t* prefix, uint8_t* victims, int64_t* blocker, hipStream_t s, hipError_t* hip_err) {
  *hip_err = hipSuccess;
  if (n_gangs <= 0) return true;
  int maxD = 1;
  for (int k = 0; k < n_pages; ++k) maxD = pages[k].pg.D > maxD ? pages[k].pg.D : maxD;
  PreemptPagedArgs a{};
  a.pages = pages_dev, a.n_pages = n_pages, a.rows = rows_dev, a.n = n, a.m = m, a.status = status, a.summary = summary;
  a.prefix = prefix, a.victims = victims, a.T = T, a.on_equal = on_equal ? 1 : 0;
  const GangsPagedArgs ga{gang_off_dev, n_gangs, blocker};
  if ((*hip_err = hipMemcpyAsync(pages_dev, pages, sizeof(PreemptPage) * (size_t)n_pages, hipMemcpyHostToDevice, s)) != hipSuccess) return false;
  if ((*hip_err = hipEventRecord(pages_copied, s)) != hipSuccess) return false;
  const int blocks = (int)(n_gangs < kPreemptMaxBlocks ? n_gangs : kPreemptMaxBlocks);
  const int DT = dt_bucket(maxD);
  if (DT == 4) hipLaunchKernelGGL(kt_preempt_gangs_paged<4>, dim3(blocks), dim3(kWave), 0, s, a, ga);
  else if (DT == 8) hipLaunchKernelGGL(kt_preempt_gangs_paged<8>, dim3(blocks), dim3(kWave), 0, s, a, ga);
  else hipLaunchKernelGGL(kt_preempt_gangs_paged<16>, dim3(blocks), dim3(kWave), 0, s, a, ga);
  return true;
}

// ---- the reprieve pass -------------------------------------------------------------------------------------------------------
// Candidate row cb (status-matrix row crow) against the list, for the members [i0, i1).  JUDGE: would some throttle that matches
// the candidate stop some member on some page with the candidate back (per lane: ballot it), nothing is written.  Otherwise the
// candidate's amounts are added (SIGN = 1) to or taken off (SIGN = -1) the state of every entry whose throttle matches it, on
// every page.
template <int DT, bool JUDGE, int SIGN, class ST>
__device__ __forceinline__ bool gang_reprieve_paged_step(const ReprievePagedArgs& a, ST& st, uint32_t n_list, const uint8_t* crow, int64_t cb, int64_t i0,
                                                         int64_t i1, uint32_t lane) {
  const bool eq = a.on_equal != 0;
  bool fail = false;
  uint32_t fb = 0;  // the page's first flat name
  for (int k = 0; k < a.n_pages; ++k) {
    const PreemptPage pp = preempt_page(a.pages, k);
    const int D = pp.pg.D, DS = pp.pg.DS;
    const ThrTables& tt = pp.pg.tt;
    const bool first_page = k == 0;
    const uint32_t cpres = pp.pg.pod_flags[cb] >> kPresentShift;  // the candidate's presence bits of THIS page's names
    uint32_t track = 0;  // the names of this page some member requests: only they are ever judged (wave-uniform)
    for (int64_t i = i0; i < i1; ++i) {
      const int64_t p = a.rows[i];
#pragma unroll
      for (int d = 0; d < DT; ++d)
        if (d < D && pp.pg.req[p * DS + d] != 0) track |= 1u << d;
    }
    if (!first_page && track == 0) {  // (wave-uniform; page 0 carries the pod count)
      fb += (uint32_t)D;
      continue;
    }
    int64_t cv[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d) cv[d] = (d < D && ((track >> d) & 1u) && ((cpres >> d) & 1u)) ? pp.pg.req[cb * DS + d] : 0;
    const GangPageView view{pp.pg, a.rows, a.status, a.T};
    for (uint32_t e = lane; e < n_list; e += kWave) {
      const uint32_t tw = st.tl[e], t = tw & ~kPagedUseCalc;
      if (crow[t] == 0) continue;
      if constexpr (JUDGE) {
        const uint32_t tf = tt.flags[t];
        const AmountTab& th = (tw & kPagedUseCalc) ? pp.calc : tt.spec;
        GangThr<DT> g;
        g.eq = eq, g.eq3 = admit_eq3(tf, eq);
        // the pod count is page 0's: elsewhere the threshold does not name it
        g.th_hc = first_page && th.has_count[t] != 0, g.r_hc = tt.reserved.has_count[t] != 0;
        g.th_c = th.count[t], g.r_c = tt.reserved.count[t];
        g.th_p = th.present[t], g.r_p = tt.reserved.present[t];
        const uint32_t c_p = pp.calc.present[t];
        // the tentative `used` with the candidate back, and the flags of a fresh reconcile of it
        GangUsed<DT> u;
        u.u_c = 0, u.u_hc = false, u.c_flag = false;
        if (first_page) {
          const int64_t pods = st.pods[e] + SIGN;
          u.u_c = pods, u.u_hc = pods > 0, u.c_flag = pp.calc.has_count[t] != 0 && u.u_hc && pods >= pp.calc.count[t];
        }
        u.flag_m = u.pr_m = 0u;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          g.tv[d] = g.rv[d] = u.u_v[d] = 0;
          if (d >= D) continue;
          g.rv[d] = tt.reserved.v[(size_t)t * D + d];  // (every name: Reserve adds to it whoever reads it)
          // a name no member requests, or that neither threshold names, passes every step of every member
          if (!(((track & (g.th_p | c_p)) >> d) & 1u)) continue;
          g.tv[d] = th.v[(size_t)t * D + d];
          const bool has = (cpres >> d) & 1u;
          u.u_v[d] = st.uv[(size_t)(fb + d) * st.cap + e] + (has ? cv[d] : 0);
          // presence is exact: the name is in `used` while a counted pod carries it
          const bool u_pr = st.uc[(size_t)(fb + d) * st.cap + e] + (has ? 1u : 0u) > 0u;
          u.pr_m |= u_pr ? 1u << d : 0u;
          u.flag_m |= (((c_p >> d) & 1u) && u_pr && u.u_v[d] >= pp.calc.v[(size_t)t * D + d]) ? 1u << d : 0u;
        }
        fail |= gang_walk<DT>(view, t, i0, i1, g, u) < i1;
      } else {
        if (first_page) st.pods[e] += SIGN;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          if (d >= D || !((track >> d) & 1u) || !((cpres >> d) & 1u)) continue;  // (wave-uniform)
          st.uv[(size_t)(fb + d) * st.cap + e] += SIGN * cv[d];
          st.uc[(size_t)(fb + d) * st.cap + e] += (uint32_t)SIGN;
        }
      }
    }
    fb += (uint32_t)D;
  }
  return fail;
}

template <int DT, bool IN_LDS, class CHUNK>
__device__ __forceinline__ void gang_reprieve_paged_walk(const ReprievePagedArgs& a, ReprieveState<IN_LDS> st, const CHUNK& chunk, lds_u32wp list,
                                                         int64_t gi, int64_t i0, int64_t i1, int64_t k, uint32_t lane) {
  const int T = a.T;
  const int64_t n = a.n;
  uint8_t* vic = a.victims + gi * a.m;
  const uint32_t n_list = reprieve_paged_list<DT, true>(a, chunk, list, &st, lane);
  __syncthreads();  // an entry is owned by lane (entry mod 64) from here on; another lane wrote it
  // the masked positions of one block of 64 candidates: their rows come in with one load
  auto block = [&](int64_t q0, int64_t& c) -> uint64_t {
    const int64_t q = q0 + lane;
    const bool masked = q < k && vic[q] != 0;
    c = masked ? a.rows[n + q] : 0;
    return __ballot(masked);
  };
  // S_k: the totals minus every masked victim
  for (int64_t q0 = 0; q0 < k; q0 += kWave) {
    int64_t c;
    uint64_t mk = block(q0, c);
    while (mk != 0ull) {
      const int b = __ffsll((long long)mk) - 1;
      mk &= mk - 1ull;
      (void)gang_reprieve_paged_step<DT, false, -1>(a, st, n_list, a.status + (n + q0 + b) * (int64_t)T, __shfl(c, b), i0, i1, lane);
    }
  }
  // the walk: c_{k-1} first
  for (int64_t q0 = ((k - 1) / kWave) * kWave; q0 >= 0; q0 -= kWave) {
    int64_t c;
    uint64_t mk = block(q0, c);
    while (mk != 0ull) {
      const int b = 63 - __clzll((long long)mk);
      mk &= ~(1ull << b);
      const int64_t cb = __shfl(c, b);
      const uint8_t* crow = a.status + (n + q0 + b) * (int64_t)T;
      const bool fail = gang_reprieve_paged_step<DT, true, 1>(a, st, n_list, crow, cb, i0, i1, lane);
      if (__ballot(fail) != 0ull) continue;  // c_j stays a victim
      (void)gang_reprieve_paged_step<DT, false, 1>(a, st, n_list, crow, cb, i0, i1, lane);
      if (lane == 0) vic[q0 + b] = 0;
    }
  }
}

template <int DT, bool IN_LDS>
__global__ __launch_bounds__(kWave) void kt_preempt_gangs_reprieve_paged(const ReprievePagedArgs a, const GangsPagedArgs ga) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  __shared__ __attribute__((aligned(16))) unsigned char state[kReprieveLdsBytes];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  for (int64_t gi = blockIdx.x; gi < ga.n_gangs; gi += gridDim.x) {  // (wave-uniform: one gang per wave and turn)
    const int64_t k = a.prefix[gi];
    if (k <= 0) continue;
    const int64_t i0 = ga.gang_off[gi], i1 = ga.gang_off[gi + 1];
    const auto chunk = [&](int c0, lds_u32wp l, bool* err) {
      return gang_affected_chunk(a.status, i0, i1, a.T, c0, l, (uint32_t)kPreemptChunk, 0u, err);
    };
    if constexpr (IN_LDS) {  // (T <= lds_cap: no list outgrows LDS, nothing is counted first)
      gang_reprieve_paged_walk<DT, true>(a, ReprieveState<true>((KT_LDS unsigned char*)state, a.lds_cap, a.F), chunk, list, gi, i0, i1, k, lane);
    } else {
      const uint32_t n_list = reprieve_paged_list<DT, false, void>(a, chunk, list, nullptr, lane);
      if (n_list <= a.lds_cap)
        gang_reprieve_paged_walk<DT, true>(a, ReprieveState<true>((KT_LDS unsigned char*)state, a.lds_cap, a.F), chunk, list, gi, i0, i1, k, lane);
      else if (a.ws)  // (the launcher gives a workspace whenever T > lds_cap; n_list <= T)
        gang_reprieve_paged_walk<DT, false>(a, ReprieveState<false>(a.ws + (size_t)blockIdx.x * a.ws_slot, (uint32_t)a.T, a.F), chunk, list, gi, i0, i1,
                                            k, lane);
    }
    __syncthreads();  // the next gang rewrites the state
  }
}

void launch_preempt_gangs_reprieve_paged(const PreemptPage* pages, int n_pages, const PreemptPage* pages_dev, int64_t n, int64_t m,
                                         const int64_t* rows_dev, int64_t n_gangs, const int64_t* gang_off_dev, int T, bool on_equal,
                                         const uint8_t* status, const int64_t* prefix, uint8_t* victims, void* ws, uint32_t lds_cap_limit,
                                         hipStream_t s) {
  if (n_gangs <= 0 || m <= 0) return;
  int maxD = 1;
  for (int k = 0; k < n_pages; ++k) maxD = pages[k].pg.D > maxD ? pages[k].pg.D : maxD;
  ReprievePagedArgs a{};
  a.pages = pages_dev, a.n_pages = n_pages, a.F = preempt_paged_names(pages, n_pages), a.rows = rows_dev, a.n = n, a.m = m, a.status = status;
  a.prefix = prefix, a.victims = victims, a.T = T, a.on_equal = on_equal ? 1 : 0;
  a.lds_cap = reprieve_lds_cap(a.F, lds_cap_limit);
  const bool in_lds = (uint32_t)T <= a.lds_cap;
  a.ws = in_lds ? nullptr : (unsigned char*)ws, a.ws_slot = reprieve_slot_bytes(T, a.F);
  const GangsPagedArgs ga{gang_off_dev, n_gangs, nullptr};
  const int blocks = reprieve_blocks(T, a.F, n_gangs, a.lds_cap);
  const int DT = dt_bucket(maxD);
#define KT_LAUNCH_GANG_REPRIEVE_PAGED(DT_)                                                                                     \
  do {                                                                                                                         \
    if (in_lds) hipLaunchKernelGGL((kt_preempt_gangs_reprieve_paged<DT_, true>), dim3(blocks), dim3(kWave), 0, s, a, ga);       \
    else hipLaunchKernelGGL((kt_preempt_gangs_reprieve_paged<DT_, false>), dim3(blocks), dim3(kWave), 0, s, a, ga);             \
  } while (0)
  if (DT == 4) KT_LAUNCH_GANG_REPRIEVE_PAGED(4);
  else if (DT == 8) KT_LAUNCH_GANG_REPRIEVE_PAGED(8);
  else KT_LAUNCH_GANG_REPRIEVE_PAGED(16);
#undef KT_LAUNCH_GANG_REPRIEVE_PAGED
}

}  // namespace kt
