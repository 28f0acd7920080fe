// kt_kernels_preempt_paged.hip — the victim prefix and its reprieve pass over PAGES of resource names (kt_paged_preempt), gfx950.
//
// The definitions are kt_kernels_preempt.hip's and kt_kernels_reprieve.hip's on the cluster of all names; a page is an engine of
// <= 16 names that holds every pod row and every throttle row (kt_engine.h, "PAGES").  What the pages share is judged once, what
// is per name is judged page by page, and the verdicts meet before anything is decided:
//   * which throttles affect which pod, the error rows and the list cut m_eff: ONE check of page 0 over preemptors ++ candidates
//     (the selector side is the same in every page, a pod-level error shows in every page);
//   * the pod count of a throttle: page 0 (every page counts the same pods);
//   * a (throttle, k) pair fails iff the count part or some page's name part fails (the rule of kt_paged_check);
//   * status.calculatedThreshold is replaced AS A WHOLE (throttle_controller.go:116-133 compares it by value over all names): a
//     throttle reads the calculated threshold on EVERY page iff on SOME page calculatedAt is set or the dry finalize replaces it,
//     else spec.threshold on every page;
//   * a throttle keeps its stored status in every state iff its reconcile is an error on SOME page or it is not valid and
//     responsible; the stored status is then read on every page.
//
// kt_preempt_paged<DT> (DT: the bucket of the widest page): one wave per preemptor, lane = candidate position, as kt_preempt.
//   Per affected throttle first the wave-uniform facts (stored and use-calc by the OR over the pages, the count part on page 0),
//   then page by page the k = 0 judgement and the 64-wide blocks of candidates with THAT page's carries — the candidate's presence
//   bits and request row come from that page's pod table, and the per-name register arrays are those of one page at a time.  A page
//   none of whose names the preemptor requests under a threshold of the throttle is skipped (page 0 never: it carries the pod
//   count and the "counted and matched" bit).  Fail bits OR into the lane's own victim bytes: no byte is shared between lanes.
// kt_preempt_reprieve_paged<DT, IN_LDS>: one wave per preemptor, lanes = list entries, as kt_preempt_reprieve.  An entry's state is
//   the counted pods and, for every name of every page, value and contributor count, laid out field by field over the flat name
//   index F = sum of the pages' D (ReprieveState with F in D's place: [cap] pods, [F][cap] values, [F][cap] contributors, [cap]
//   throttle rows — bit 31 of a throttle row caches its use-calc fact).  The judge of a candidate loops over the pages inside the
//   lane before the ONE ballot; the commit pass updates every page's fields.  IN_LDS = true: no list can outgrow LDS (throttle
//   rows <= capacity) and the HBM path is not compiled in; false: the choice is made per preemptor, as kt_preempt_reprieve does.
#include "kt_preempt_paged_common.h"

namespace kt {

// (PreemptPagedArgs, preempt_page_args, paged_thr_facts, ReprievePagedArgs and reprieve_paged_list are kt_preempt_paged_common.h's:
// the gang forms over pages read them too)

template <int DT>
__global__ __launch_bounds__(kWave) void kt_preempt_paged(const PreemptPagedArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int T = a.T;
  const bool eq = a.on_equal != 0;
  const int64_t n = a.n, m = a.m;
  const PreemptArgs a0 = preempt_page_args(a, 0);
  const int64_t m_eff = preempt_m_eff(a0, lane);  // (validity and the error rows are the same in every page)
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {  // (wave-uniform: one preemptor per wave and turn)
    const int64_t p = a.rows[i];
    uint8_t* vic = a.victims + i * m;
    for (int64_t q = lane; q < m; q += kWave) vic[q] = 0;
    const uint8_t* row = a.status + i * T;
    bool err = a.summary[i] == 2ull || !(a0.pg.pod_flags[p] & kPodValid);
    bool fail0 = false;  // some (throttle, amount) stops the pod in S_0
    bool never = false;  // ... in every S_k: a row that keeps its stored status fails
    for (int c0 = 0; c0 < T && !err && !never; c0 += kPreemptChunk) {
      bool err_c = false;
      const uint32_t n_c = admit_affected_chunk(row, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
      err = __ballot(err_c) != 0ull;
      __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
      for (uint32_t ai = 0; ai < n_c && !err && !never; ++ai) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[ai]);
        bool stored, use_calc;
        paged_thr_facts(a.pages, a.n_pages, t, &stored, &use_calc);
        if (stored) {  // the stored status of every page, whatever k
          bool f = false;
          for (int k = 0; k < a.n_pages; ++k) {
            const PreemptPage pp = preempt_page(a.pages, k);
            const int D = pp.pg.D, DS = pp.pg.DS;
            const ThrTables& tt = pp.pg.tt;
            const uint32_t tf = tt.flags[t];
            // the STORED calculated threshold: a page whose own reconcile were no error would report a fresh one in pp.calc
            const AmountTab& th = use_calc ? tt.calc : tt.spec;
            const bool eq3 = admit_eq3(tf, eq);
            if (k == 0)
              f |= preempt_fails(1, th.has_count[t] != 0, th.count[t], (tf & kThrThrottledPod) != 0, tt.used.has_count[t] != 0, tt.used.count[t],
                                 tt.reserved.has_count[t] != 0, tt.reserved.count[t], eq3, eq);
            const uint32_t th_p = th.present[t], u_p = tt.used.present[t], r_p = tt.reserved.present[t], flg = tt.thrl_flag[t] & tt.thrl_has[t];
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              if (d >= D) continue;
              const int64_t vp = pp.pg.req[p * DS + d];
              if (vp == 0) continue;
              f |= preempt_fails(vp, (th_p >> d) & 1u, th.v[(size_t)t * D + d], (flg >> d) & 1u, (u_p >> d) & 1u, tt.used.v[(size_t)t * D + d],
                                 (r_p >> d) & 1u, tt.reserved.v[(size_t)t * D + d], eq3, eq);
            }
          }
          never = f;
          // the candidates it matches are "counted and matched by an affecting throttle" all the same
          for (int64_t q0 = 0; q0 < m_eff && !never; q0 += kWave) {
            const int64_t q = q0 + lane;
            const PreemptCand L = preempt_cand(a0, t, q, m_eff);
            if (L.contrib) vic[q] |= (uint8_t)1;
          }
          continue;
        }
        bool f0 = false;  // k = 0: the count part and every page's name part
        for (int k = 0; k < a.n_pages; ++k) {
          const PreemptArgs ak = preempt_page_args(a, k);
          const int D = ak.pg.D, DS = ak.pg.DS;
          const ThrTables& tt = ak.pg.tt;
          const uint32_t tf = tt.flags[t];
          const AmountTab& th = use_calc ? ak.calc : tt.spec;
          const bool eq3 = admit_eq3(tf, eq);
          const bool th_hc = th.has_count[t] != 0, c_hc = ak.calc.has_count[t] != 0, r_hc = tt.reserved.has_count[t] != 0;
          const int64_t th_c = th.count[t], c_c = ak.calc.count[t], r_c = tt.reserved.count[t];
          const uint32_t th_p = th.present[t], c_p = ak.calc.present[t], r_p = tt.reserved.present[t];
          const unsigned long long* prow = ak.partial + (size_t)t * partial_stride(D);
          const int64_t pods_total = (int64_t)prow[partial_off_pods(D)];
          int64_t vp[DT], tv[DT], cv[DT], rv[DT], tot_v[DT], tot_c[DT];
          bool need[DT], any_need = false;
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            need[d] = false, vp[d] = tv[d] = cv[d] = rv[d] = tot_v[d] = tot_c[d] = 0;
            if (d >= D) continue;
            vp[d] = ak.pg.req[p * DS + d];
            // a name the pod does not request passes every step, and so does one that neither threshold names
            need[d] = vp[d] != 0 && (((th_p | c_p) >> d) & 1u);
            if (!need[d]) continue;
            any_need = true;
            tv[d] = th.v[(size_t)t * D + d], cv[d] = ak.calc.v[(size_t)t * D + d], rv[d] = tt.reserved.v[(size_t)t * D + d];
            tot_v[d] = (int64_t)prow[d], tot_c[d] = (int64_t)prow[partial_off_presence(D) + d];
          }
          if (k != 0 && !any_need) continue;  // nothing of this page can fail, and page 0 has marked the matched candidates
          if (k == 0) f0 |= preempt_count_fails(th_hc, th_c, c_hc, c_c, pods_total, r_hc, r_c, eq3, eq);
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            if (!need[d]) continue;
            f0 |= preempt_name_fails(vp[d], (th_p >> d) & 1u, tv[d], (c_p >> d) & 1u, cv[d], tot_v[d], tot_c[d], (r_p >> d) & 1u, rv[d], eq3, eq);
          }
          // every k >= 1, 64 positions at a time, with this page's carries
          int64_t car_v[DT], car_pods = 0;
          uint32_t car_c[DT];
#pragma unroll
          for (int d = 0; d < DT; ++d) car_v[d] = 0, car_c[d] = 0u;
          for (int64_t q0 = 0; q0 < m_eff; q0 += kWave) {
            const int64_t q = q0 + lane;
            const PreemptCand L = preempt_cand(ak, t, q, m_eff);  // (fl: THIS page's presence bits)
            bool f = false;
            if (k == 0) {
              const int64_t pre_pods = preempt_scan_pods(L, lane, car_pods);
              f = preempt_count_fails(th_hc, th_c, c_hc, c_c, pods_total - pre_pods, r_hc, r_c, eq3, eq);
            }
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              if (!need[d]) continue;  // (wave-uniform)
              int64_t pre_v;
              uint32_t pre_c;
              preempt_scan_name(ak, L, d, lane, car_v[d], car_c[d], &pre_v, &pre_c);
              f |= preempt_name_fails(vp[d], (th_p >> d) & 1u, tv[d], (c_p >> d) & 1u, cv[d], tot_v[d] - pre_v, tot_c[d] - (int64_t)pre_c, (r_p >> d) & 1u,
                                      rv[d], eq3, eq);
            }
            const bool mark = k == 0 && L.contrib;
            if (L.in && (mark || f)) vic[q] |= (uint8_t)((mark ? 1u : 0u) | (f ? 2u : 0u));
          }
        }
        fail0 |= f0;
      }
      __syncthreads();  // the next chunk rewrites the list
    }
    const int64_t ans = preempt_answer(vic, m, m_eff, !err && !never, fail0, lane);
    if (lane == 0) a.prefix[i] = ans;
  }
}

bool launch_preempt_paged(const PreemptPage* pages, int n_pages, PreemptPage* pages_dev, hipEvent_t pages_copied, int64_t n, int64_t m,
                          const int64_t* rows_dev, int T, bool on_equal, const uint8_t* status, const uint64_t* summary, int64_t* prefix,
                          uint8_t* victims, hipStream_t s, hipError_t* hip_err) {
  *hip_err = hipSuccess;
  if (n <= 0) return true;
  int maxD = 1;
  for (int k = 0; k < n_pages; ++k) maxD = pages[k].pg.D > maxD ? pages[k].pg.D : maxD;
  PreemptPagedArgs a{};
  a.pages = pages_dev, a.n_pages = n_pages, a.rows = rows_dev, a.n = n, a.m = m, a.status = status, a.summary = summary;
  a.prefix = prefix, a.victims = victims, a.T = T, a.on_equal = on_equal ? 1 : 0;
  if ((*hip_err = hipMemcpyAsync(pages_dev, pages, sizeof(PreemptPage) * (size_t)n_pages, hipMemcpyHostToDevice, s)) != hipSuccess) return false;
  if ((*hip_err = hipEventRecord(pages_copied, s)) != hipSuccess) return false;
  const int blocks = (int)(n < kPreemptMaxBlocks ? n : kPreemptMaxBlocks);
  const int DT = dt_bucket(maxD);
  if (DT == 4) hipLaunchKernelGGL(kt_preempt_paged<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_preempt_paged<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_preempt_paged<16>, dim3(blocks), dim3(kWave), 0, s, a);
  return true;
}

// ---- the reprieve pass -------------------------------------------------------------------------------------------------------
// Candidate row cb (status-matrix row crow) against the list, for preemptor row p.  JUDGE: would some (throttle, amount) pair of some
// page stop the preemptor with the candidate back (per lane: ballot it), nothing is written.  Otherwise the candidate's amounts
// are added (SIGN = 1) to or taken off (SIGN = -1) the state of every entry whose throttle matches it, on every page.
template <int DT, bool JUDGE, int SIGN, class ST>
__device__ __forceinline__ bool reprieve_paged_step(const ReprievePagedArgs& a, ST& st, uint32_t n_list, const uint8_t* crow, int64_t cb, int64_t p,
                                                    uint32_t lane) {
  const bool eq = a.on_equal != 0;
  bool fail = false;
  uint32_t fb = 0;  // the page's first flat name
  for (int k = 0; k < a.n_pages; ++k) {
    const PreemptPage pp = preempt_page(a.pages, k);
    const int D = pp.pg.D, DS = pp.pg.DS;
    const ThrTables& tt = pp.pg.tt;
    const uint32_t cpres = pp.pg.pod_flags[cb] >> kPresentShift;  // the candidate's presence bits of THIS page's names
    int64_t vp[DT], cv[DT];
    uint32_t track = 0;  // the names of this page the preemptor requests: only they are ever judged
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      vp[d] = d < D ? pp.pg.req[p * DS + d] : 0;
      track |= vp[d] != 0 ? 1u << d : 0u;
      cv[d] = (vp[d] != 0 && ((cpres >> d) & 1u)) ? pp.pg.req[cb * DS + d] : 0;
    }
    if (k != 0 && track == 0) {  // (wave-uniform; page 0 carries the pod count)
      fb += (uint32_t)D;
      continue;
    }
    for (uint32_t e = lane; e < n_list; e += kWave) {
      const uint32_t tw = st.tl[e], t = tw & ~kPagedUseCalc;
      if (crow[t] == 0) continue;
      if constexpr (JUDGE) {
        const uint32_t tf = tt.flags[t];
        const AmountTab& th = (tw & kPagedUseCalc) ? pp.calc : tt.spec;
        const bool eq3 = admit_eq3(tf, eq);
        const uint32_t th_p = th.present[t], c_p = pp.calc.present[t], r_p = tt.reserved.present[t];
        if (k == 0) {
          const int64_t pods = st.pods[e] + SIGN;
          const bool u_hc = pods > 0;
          fail |= preempt_fails(1, th.has_count[t] != 0, th.count[t], pp.calc.has_count[t] != 0 && u_hc && pods >= pp.calc.count[t], u_hc, pods,
                                tt.reserved.has_count[t] != 0, tt.reserved.count[t], eq3, eq);
        }
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          if (!((track >> d) & 1u)) continue;  // (wave-uniform)
          // a name that neither threshold names passes every step
          if (!(((th_p | c_p) >> d) & 1u)) continue;
          const bool has = (cpres >> d) & 1u;
          const int64_t u_v = st.uv[(size_t)(fb + d) * st.cap + e] + (has ? cv[d] : 0);
          // presence is exact: the name is in `used` while a counted pod carries it
          const bool u_pr = st.uc[(size_t)(fb + d) * st.cap + e] + (has ? 1u : 0u) > 0u;
          const bool c_pd = (c_p >> d) & 1u;
          fail |= preempt_fails(vp[d], (th_p >> d) & 1u, th.v[(size_t)t * D + d], c_pd && u_pr && u_v >= pp.calc.v[(size_t)t * D + d], u_pr, u_v,
                                (r_p >> d) & 1u, tt.reserved.v[(size_t)t * D + d], eq3, eq);
        }
      } else {
        if (k == 0) st.pods[e] += SIGN;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          if (!((track >> d) & 1u) || !((cpres >> d) & 1u)) continue;  // (wave-uniform)
          st.uv[(size_t)(fb + d) * st.cap + e] += SIGN * cv[d];
          st.uc[(size_t)(fb + d) * st.cap + e] += (uint32_t)SIGN;
        }
      }
    }
    fb += (uint32_t)D;
  }
  return fail;
}

// one chunk of preemptor i's own matrix row, for reprieve_paged_list
__device__ __forceinline__ auto preemptor_chunk(const ReprievePagedArgs& a, int64_t i) {
  return [&a, i](int c0, lds_u32wp l, bool* err) { return admit_affected_chunk(a.status + i * a.T, a.T, c0, l, (uint32_t)kPreemptChunk, 0u, err); };
}

template <int DT, bool IN_LDS>
__device__ __forceinline__ void reprieve_paged_walk(const ReprievePagedArgs& a, ReprieveState<IN_LDS> st, lds_u32wp list, int64_t i, int64_t k,
                                                    uint32_t lane) {
  const int T = a.T;
  const int64_t n = a.n, p = a.rows[i];
  uint8_t* vic = a.victims + i * a.m;
  const uint32_t n_list = reprieve_paged_list<DT, true>(a, preemptor_chunk(a, i), list, &st, lane);
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
      (void)reprieve_paged_step<DT, false, -1>(a, st, n_list, a.status + (n + q0 + b) * (int64_t)T, __shfl(c, b), p, lane);
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
      const bool fail = reprieve_paged_step<DT, true, 1>(a, st, n_list, crow, cb, p, lane);
      if (__ballot(fail) != 0ull) continue;  // c_j stays a victim
      (void)reprieve_paged_step<DT, false, 1>(a, st, n_list, crow, cb, p, lane);
      if (lane == 0) vic[q0 + b] = 0;
    }
  }
}

template <int DT, bool IN_LDS>
__global__ __launch_bounds__(kWave) void kt_preempt_reprieve_paged(const ReprievePagedArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  __shared__ __attribute__((aligned(16))) unsigned char state[kReprieveLdsBytes];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {  // (wave-uniform: one preemptor per wave and turn)
    const int64_t k = a.prefix[i];
    if (k <= 0) continue;
    if constexpr (IN_LDS) {  // (T <= lds_cap: no list outgrows LDS, nothing is counted first)
      reprieve_paged_walk<DT, true>(a, ReprieveState<true>((KT_LDS unsigned char*)state, a.lds_cap, a.F), list, i, k, lane);
    } else {
      const uint32_t n_list = reprieve_paged_list<DT, false, void>(a, preemptor_chunk(a, i), list, nullptr, lane);
      if (n_list <= a.lds_cap)
        reprieve_paged_walk<DT, true>(a, ReprieveState<true>((KT_LDS unsigned char*)state, a.lds_cap, a.F), list, i, k, lane);
      else if (a.ws)  // (the launcher gives a workspace whenever T > lds_cap; n_list <= T)
        reprieve_paged_walk<DT, false>(a, ReprieveState<false>(a.ws + (size_t)blockIdx.x * a.ws_slot, (uint32_t)a.T, a.F), list, i, k, lane);
    }
    __syncthreads();  // the next preemptor rewrites the state
  }
}

size_t reprieve_paged_ws_bytes(int T, const PreemptPage* pages, int n_pages, int64_t n, uint32_t lds_cap_limit) {
  return reprieve_ws_bytes(T, preempt_paged_names(pages, n_pages), n, lds_cap_limit);
}

void launch_preempt_reprieve_paged(const PreemptPage* pages, int n_pages, const PreemptPage* pages_dev, int64_t n, int64_t m, const int64_t* rows_dev,
                                   int T, bool on_equal, const uint8_t* status, const int64_t* prefix, uint8_t* victims, void* ws,
                                   uint32_t lds_cap_limit, hipStream_t s) {
  if (n <= 0 || m <= 0) return;
  int maxD = 1;
  for (int k = 0; k < n_pages; ++k) maxD = pages[k].pg.D > maxD ? pages[k].pg.D : maxD;
  ReprievePagedArgs a{};
  a.pages = pages_dev, a.n_pages = n_pages, a.F = preempt_paged_names(pages, n_pages), a.rows = rows_dev, a.n = n, a.m = m, a.status = status;
  a.prefix = prefix, a.victims = victims, a.T = T, a.on_equal = on_equal ? 1 : 0;
  a.lds_cap = reprieve_lds_cap(a.F, lds_cap_limit);
  const bool in_lds = (uint32_t)T <= a.lds_cap;
  a.ws = in_lds ? nullptr : (unsigned char*)ws, a.ws_slot = reprieve_slot_bytes(T, a.F);
  const int blocks = reprieve_blocks(T, a.F, n, a.lds_cap);
  const int DT = dt_bucket(maxD);
#define KT_LAUNCH_REPRIEVE_PAGED(DT_)                                                                                 \
  do {                                                                                                                \
    if (in_lds) hipLaunchKernelGGL((kt_preempt_reprieve_paged<DT_, true>), dim3(blocks), dim3(kWave), 0, s, a);        \
    else hipLaunchKernelGGL((kt_preempt_reprieve_paged<DT_, false>), dim3(blocks), dim3(kWave), 0, s, a);              \
  } while (0)
  if (DT == 4) KT_LAUNCH_REPRIEVE_PAGED(4);
  else if (DT == 8) KT_LAUNCH_REPRIEVE_PAGED(8);
  else KT_LAUNCH_REPRIEVE_PAGED(16);
#undef KT_LAUNCH_REPRIEVE_PAGED
}

}  // namespace kt
