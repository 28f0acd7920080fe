// kt_kernels_admit.hip — sequential admission of a pod queue with reservation, gfx950.
//
// The scheduler admits pods one at a time: PreFilter(pod) (plugin.go:148-215) and, on Success, Reserve(pod)
// (plugin.go:217-239 -> [Cluster]ThrottleController.Reserve, throttle_controller.go:271-300 ->
// reservedResourceAmounts.addPod, reserved_resource_amounts.go:66-77), which adds ResourceAmountOfPod(pod) to the
// reserved amount of every throttle that affects the pod; the next pod's CheckThrottledFor sees it in steps 3
// and 4 (throttle_types.go:142-150).  The dependency chain is inherent, so this is ONE wave walking the queue in
// order with the whole mutable state (reserved amounts of all throttles) resident in LDS:
//
//   input   status matrix [n][T] of a preceding kt_check launch over the same queue: which throttles affect
//           which pod (selector side, evaluated for all pods in parallel there), error rows = 255
//   per pod (1) the row's nonzero bytes -> the pod's affected-throttle list (16 bytes per lane, ballot/mbcnt append)
//           (2) lane = (affected throttle, dimension): the four CheckThrottledFor steps against
//               threshold / status.used / status.throttled (HBM, read-only) and the CURRENT reserved row (LDS),
//               verdict bits OR-reduced over the lanes of a throttle
//           (3) summary word as PreFilter would return it at this point; the matrix row is rewritten with the
//               statuses the pod actually met
//           (4) verdict Success => reserved[t] += ResourceAmountOfPod(pod) for every affected throttle (LDS)
//   output  per-pod summary words, the rewritten matrix, and (commit) the reserved tables in HBM.
// When the state does not fit in LDS (thousands of throttles) it lives in an HBM scratch buffer instead (same code,
// L2 latency per step).
// There is ONE kernel, kt_admit<DT, IN_LDS>, over n_pages >= 1 page descriptors in device memory (a page = an engine of
// <= 16 resource names): kt_admit_launch is the one-page case of kt_paged_admit.  Step (2) is the name part of every page
// OR-ed with the count part of page 0, step (4) reserves on every page.
//
// Gangs (kt_admit_gangs<DT, IN_LDS>, kt_admit_gangs_launch): the queue is cut into consecutive groups that are admitted all or
// nothing.  Every member is walked as above; when one of them was not admitted, every member that reserved gets Unreserve
// (plugin.go:240-257 -> reservedResourceAmounts.removePod, reserved_resource_amounts.go:79-90) before the next gang starts.
// The undo costs the touched entries only: values and counts by exact subtraction, the presence word from a copy taken when the
// gang first touched the throttle (`rq`, 4 x T bytes per page, and one gang tag per throttle that says whether the copy is this
// gang's: the reference recomputes the total over the remaining pods, reserved_resource_amounts.go:148-156, so a name only a
// rolled-back pod brought in disappears again).  An admitted gang costs that copy and nothing else.  For the rollback the touched
// throttles are re-derived from the members' matrix rows: step (3) rewrites nonzero bytes with nonzero bytes, the list is the same.
//
// Elastic gangs (kt_admit_gangs_elastic<DT, IN_LDS>, kt_admit_gangs_elastic_launch): the same walk with another rule at the gang's
// end — the gang stays when at least min_members[g] members succeeded and no member flagged KT_GANG_MEMBER_REQUIRED failed
// (PodGroup.minMember / Volcano's minAvailable, a mandatory role).  A kept gang keeps what its succeeded members reserved (the ones
// that failed never stored: nothing to restore); a gang that misses the rule goes through the rollback above, unchanged.
#include "kt_admit_common.h"

namespace kt {

struct AdmitPagedArgs {
  const AdmitPage* pages;  // [n_pages] in device memory (ThrTables is too large to pass by value per page)
  int32_t n_pages;
  const int64_t* rows;  // nullable: queue position -> pod table row (the same rows in every page)
  int64_t n;
  unsigned char* scratch;  // every page's state in HBM when it does not fit LDS (nullable)
  uint8_t* status;    // [n][T] in/out: page 0's matrix in, the combined statuses out
  uint64_t* summary;  // [n] out
  int32_t T, on_equal, commit;
  uint32_t off_list, list_cap;
};
// what the gang form (kt_admit_gangs) takes on top
struct AdmitGangArgs {
  const int64_t* gang_off;  // [n_gangs + 1] queue positions
  int64_t n_gangs;
  uint8_t* gang_out;        // [n_gangs] 1 admitted, 0 rolled back
  uint32_t off_rq, rq_stride;  // page k's saved presence words at off_rq + k * rq_stride (LDS or scratch, as the state)
  uint32_t off_tag;            // [T] 1 + the gang that saved the throttle's presence words last (0: none)
  // the elastic form (kt_admit_gangs_elastic) alone
  const int64_t* min_members;   // [n_gangs] the quorum: members that must succeed, in [1, size of the gang]
  const uint8_t* member_flags;  // [n] nullable: bit 0 = the member is required
  int64_t* members_out;         // [n_gangs] members that stay reserved; 0: rolled back
};
// how a span of the queue ends: never undone (the plain queue), undone unless every member succeeded (gangs), undone unless the
// quorum and every required member succeeded (elastic gangs)
enum AdmitMode { kAdmitQueue = 0, kAdmitGangs = 1, kAdmitElastic = 2 };

// The mutable state (reserved amounts of all throttles) lives in LDS when it fits; otherwise in a scratch buffer in
// HBM that only this wave touches, read and written through L2 (agent-scope atomics: never served from a stale L1 line).
template <bool IN_LDS>
struct AdmitState;
template <>
struct AdmitState<true> {
  KT_LDS int64_t* rv;
  KT_LDS int64_t* rc;
  KT_LDS uint32_t* rp;
  __device__ __forceinline__ int64_t ld_v(int i) const { return rv[i]; }
  __device__ __forceinline__ void st_v(int i, int64_t x) const { rv[i] = x; }
  __device__ __forceinline__ int64_t ld_c(int i) const { return rc[i]; }
  __device__ __forceinline__ void st_c(int i, int64_t x) const { rc[i] = x; }
  __device__ __forceinline__ uint32_t ld_p(int i) const { return rp[i]; }
  __device__ __forceinline__ void st_p(int i, uint32_t x) const { rp[i] = x; }
};
template <>
struct AdmitState<false> {
  int64_t* rv;
  int64_t* rc;
  uint32_t* rp;
  __device__ __forceinline__ int64_t ld_v(int i) const { return __hip_atomic_load(rv + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void st_v(int i, int64_t x) const { __hip_atomic_store(rv + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ int64_t ld_c(int i) const { return __hip_atomic_load(rc + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void st_c(int i, int64_t x) const { __hip_atomic_store(rc + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ uint32_t ld_p(int i) const { return __hip_atomic_load(rp + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void st_p(int i, uint32_t x) const { __hip_atomic_store(rp + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// the state of one engine's T throttle rows at byte offsets of LDS or of the scratch buffer
template <bool IN_LDS>
__device__ __forceinline__ AdmitState<IN_LDS> admit_state_at(KT_LDS unsigned char* lds, unsigned char* scratch, uint32_t off_rv,
                                                             uint32_t off_rc, uint32_t off_rp) {
  AdmitState<IN_LDS> st;
  if constexpr (IN_LDS) {
    st.rv = (KT_LDS int64_t*)(lds + off_rv);    // [T][D] reserved requests
    st.rc = (KT_LDS int64_t*)(lds + off_rc);    // [T]    reserved pod count
    st.rp = (KT_LDS uint32_t*)(lds + off_rp);   // [T]    presence mask | has_count << 31
  } else {
    st.rv = (int64_t*)(scratch + off_rv);
    st.rc = (int64_t*)(scratch + off_rc);
    st.rp = (uint32_t*)(scratch + off_rp);
  }
  return st;
}
// gangs: the presence words as they stood before the current gang touched the throttle, and the gang tags (same home as the state)
template <bool IN_LDS>
struct AdmitPresence;
template <>
struct AdmitPresence<true> {
  KT_LDS uint32_t* rq;
  __device__ __forceinline__ uint32_t ld(int i) const { return rq[i]; }
  __device__ __forceinline__ void st(int i, uint32_t x) const { rq[i] = x; }
};
template <>
struct AdmitPresence<false> {
  uint32_t* rq;
  __device__ __forceinline__ uint32_t ld(int i) const { return __hip_atomic_load(rq + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void st(int i, uint32_t x) const { __hip_atomic_store(rq + i, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
template <bool IN_LDS>
__device__ __forceinline__ AdmitPresence<IN_LDS> admit_presence_at(KT_LDS unsigned char* lds, unsigned char* scratch, uint32_t off) {
  AdmitPresence<IN_LDS> q;
  if constexpr (IN_LDS) q.rq = (KT_LDS uint32_t*)(lds + off);
  else q.rq = (uint32_t*)(scratch + off);
  return q;
}

// reserved tables (HBM) -> state, and back (commit)
template <bool IN_LDS>
__device__ __forceinline__ void admit_load_state(const AdmitState<IN_LDS>& st, const ThrTables& tt, int T, int D) {
  for (int t = (int)threadIdx.x; t < T; t += kWave) {
    const uint32_t p = tt.reserved.present[t];
    for (int d = 0; d < D; ++d) st.st_v(t * D + d, ((p >> d) & 1u) ? tt.reserved.v[(size_t)t * D + d] : 0);
    const bool hc = tt.reserved.has_count[t] != 0;
    st.st_c(t, hc ? tt.reserved.count[t] : 0);
    st.st_p(t, p | (hc ? 0x80000000u : 0u));
  }
}
template <bool IN_LDS>
__device__ __forceinline__ void admit_store_state(const AdmitState<IN_LDS>& st, const ThrTables& tt, int T, int D) {
  for (int t = (int)threadIdx.x; t < T; t += kWave) {
    const uint32_t w = st.ld_p(t);
    for (int dd = 0; dd < D; ++dd) tt.reserved.v[(size_t)t * D + dd] = st.ld_v(t * D + dd);
    tt.reserved.present[t] = w & 0x7FFFFFFFu;
    tt.reserved.has_count[t] = (uint8_t)(w >> 31);
    tt.reserved.count[t] = st.ld_c(t);
  }
}

// (2) resourceCounts.pod of throttle t -> verdict bits (1 exceeds, 2 active, 4 insufficient)
template <bool IN_LDS>
__device__ __forceinline__ uint32_t admit_count_bits(const ThrTables& tt, const AdmitState<IN_LDS>& st, uint32_t t, bool eq) {
  const uint32_t tf = tt.flags[t];
  const AmountTab& th = admit_threshold(tt, tf);
  const bool eq3 = admit_eq3(tf, eq);
  const bool th_hc = th.has_count[t] != 0;
  const int64_t th_c = th.count[t];
  const bool u_hc = tt.used.has_count[t] != 0, r_hc = (st.ld_p(t) >> 31) != 0;
  const int64_t u_c = u_hc ? tt.used.count[t] : 0, r_c = st.ld_c(t);
  uint32_t bits = 0;
  if (th_hc && 1 > th_c) bits |= 1u;
  if ((tf & kThrThrottledPod) || (th_hc && (u_hc || r_hc) && admit_cmp((__int128)u_c + r_c, th_c, eq3))) bits |= 2u;
  if (th_hc && admit_cmp((__int128)u_c + 1 + r_c, th_c, eq)) bits |= 4u;
  return bits;
}

// (2) the name part of one page for lane (t, d): the four CheckThrottledFor steps of dimension d of the page's names for
// pod row p against the page's threshold / status.used / status.throttled and its CURRENT reserved row -> verdict bits
template <bool IN_LDS>
__device__ __forceinline__ uint32_t admit_name_bits(const AdmitPage& pg, const AdmitState<IN_LDS>& st, int64_t p, uint32_t t, uint32_t d,
                                                    bool eq) {
  const ThrTables& tt = pg.tt;
  const int D = pg.D;
  if ((int)d >= D) return 0u;
  const int64_t v = pg.req[p * pg.DS + d];
  if (v == 0) return 0u;  // steps 1-4 of a name the pod does not request
  const uint32_t tf = tt.flags[t];
  const AmountTab& th = admit_threshold(tt, tf);
  const bool eq3 = admit_eq3(tf, eq);
  const uint32_t th_p = th.present[t], u_p = tt.used.present[t], r_pw = st.ld_p(t);
  uint32_t bits = 0;
  if ((th_p >> d) & 1u) {
    const int64_t tv = th.v[(size_t)t * D + d];
    const int64_t uv = ((u_p >> d) & 1u) ? tt.used.v[(size_t)t * D + d] : 0;
    const int64_t rvd = st.ld_v(t * D + d);
    if (v > tv) bits |= 1u;                                                               // step 1
    if ((((u_p | r_pw) >> d) & 1u) && admit_cmp((__int128)uv + rvd, tv, eq3)) bits |= 2u;  // step 3
    if (admit_cmp((__int128)uv + v + rvd, tv, eq)) bits |= 4u;                             // step 4
  }
  if (((tt.thrl_flag[t] & tt.thrl_has[t]) >> d) & 1u) bits |= 2u;                         // step 2
  return bits;
}

// (4) Reserve on one page: its own names' amounts of pod row p, the count and has_count, on every affected throttle
template <int DT, bool IN_LDS>
__device__ __forceinline__ void admit_reserve(const AdmitPage& pg, const AdmitState<IN_LDS>& st, int64_t p, lds_u32wp list, uint32_t n_aff) {
  constexpr int MPW = kWave / DT;
  const uint32_t d = threadIdx.x % DT, ml = threadIdx.x / DT;
  const int D = pg.D;
  const uint32_t present = pg.pod_flags[p] >> kPresentShift;
  const bool d_in = (int)d < D;
  const int64_t v = d_in ? pg.req[p * pg.DS + d] : 0;
  for (uint32_t base = 0; base < n_aff; base += MPW) {
    const uint32_t j = base + ml;
    if (j < n_aff) {
      const uint32_t t = list[j];
      if (d_in && ((present >> d) & 1u)) st.st_v(t * D + d, st.ld_v(t * D + d) + v);
      if (d == 0) {
        st.st_c(t, st.ld_c(t) + 1);
        st.st_p(t, st.ld_p(t) | present | 0x80000000u);
      }
    }
  }
}

// Unreserve on one page: (4) undone by exact subtraction on every affected throttle; the presence word goes back to what it
// was before the gang (idempotent: a throttle several members touched is restored once per member)
template <int DT, bool IN_LDS>
__device__ __forceinline__ void admit_unreserve(const AdmitPage& pg, const AdmitState<IN_LDS>& st, const AdmitPresence<IN_LDS>& q, int64_t p,
                                                lds_u32wp list, uint32_t n_aff) {
  constexpr int MPW = kWave / DT;
  const uint32_t d = threadIdx.x % DT, ml = threadIdx.x / DT;
  const int D = pg.D;
  const uint32_t present = pg.pod_flags[p] >> kPresentShift;
  const bool d_in = (int)d < D;
  const int64_t v = d_in ? pg.req[p * pg.DS + d] : 0;
  for (uint32_t base = 0; base < n_aff; base += MPW) {
    const uint32_t j = base + ml;
    if (j < n_aff) {
      const uint32_t t = list[j];
      if (d_in && ((present >> d) & 1u)) st.st_v(t * D + d, st.ld_v(t * D + d) - v);
      if (d == 0) {
        st.st_c(t, st.ld_c(t) - 1);
        st.st_p(t, q.ld(t));  // (saved by this gang: the member reserved on t)
      }
    }
  }
}
// One wave, the queue in order, the state of every page (an engine of <= 16 resource names; one page is the plain engine) side
// by side.  Page 0's status matrix gives the affected list once per pod (selectors, namespaces and responsibility are the same
// in every page); the name part of the four steps is evaluated against every page's tables and reserved state and OR-ed before
// the reduction (exceeds > active > insufficient, as kt_paged_check combines), the count part once, on page 0; Success
// reserves on every page.
// GANGS: the queue positions [gang_off[g], gang_off[g + 1]) are admitted all or nothing, gang after gang; a gang with a member
// that was not admitted is rolled back (every member that reserved: Unreserve on every page) before the next one starts.  The
// per-pod outputs stay what PreFilter returned at the pod's turn.  Without GANGS the whole queue is one span that is never undone.
// ELASTIC: the gang is kept iff at least min_members[g] members succeeded and no required one failed; the members that failed never
// stored, so a kept partial gang needs no restore, and one that misses the rule takes the same rollback.
template <int DT, bool IN_LDS, int MODE>
__device__ __forceinline__ void admit_walk(const AdmitPagedArgs& a, const AdmitGangArgs& ga) {
  constexpr bool GANGS = MODE != kAdmitQueue, ELASTIC = MODE == kAdmitElastic;
  KT_LDS unsigned char* lds = (KT_LDS unsigned char*)kt_smem;
  lds_u32wp list = (lds_u32wp)(lds + a.off_list);  // affected throttles of the current pod
  const int T = a.T, n_pages = a.n_pages;
  const uint32_t lane = threadIdx.x;
  auto state_of = [&](const AdmitPage& pg) { return admit_state_at<IN_LDS>(lds, a.scratch, pg.off_rv, pg.off_rc, pg.off_rp); };
  auto kept_of = [&](int k) { return admit_presence_at<IN_LDS>(lds, a.scratch, ga.off_rq + (uint32_t)k * ga.rq_stride); };
  for (int k = 0; k < n_pages; ++k) {
    const AdmitPage pg = admit_page(a.pages, k);
    admit_load_state(state_of(pg), pg.tt, T, pg.D);
  }
  const AdmitPresence<IN_LDS> tag = admit_presence_at<IN_LDS>(lds, a.scratch, ga.off_tag);
  if constexpr (GANGS)
    for (int t = (int)lane; t < T; t += kWave) tag.st(t, 0u);
  if (!IN_LDS) __threadfence();
  constexpr int MPW = kWave / DT;
  const uint32_t d = lane % DT, ml = lane / DT;
  const bool eq = a.on_equal != 0;
  const int64_t n_spans = GANGS ? ga.n_gangs : 1;
  int64_t span_begin = 0, span_end = GANGS ? ga.gang_off[n_spans > 0 ? 1 : 0] : a.n;  // (gang_off[0] == 0)
  int64_t quorum_next = 0;  // ELASTIC: min_members of the next gang
  if constexpr (ELASTIC)
    if (n_spans > 0) quorum_next = ga.min_members[0];
  for (int64_t g = 0; g < n_spans; ++g) {
    const int64_t i0 = span_begin, i1 = span_end;
    const int64_t quorum = quorum_next;
    if constexpr (GANGS) {  // the next gang's end is asked for a gang ahead: its trip to HBM runs beside this gang's walk
      span_begin = i1;
      if (g + 1 < n_spans) {
        span_end = ga.gang_off[g + 2];
        if constexpr (ELASTIC) quorum_next = ga.min_members[g + 1];  // ... and its quorum beside it
      }
    }
    bool all_in = true;  // wave-uniform: every member so far was admitted
    int64_t n_in = 0;           // ELASTIC, wave-uniform: members that succeeded so far
    bool required_out = false;  // ELASTIC, wave-uniform: a required member failed
    for (int64_t i = i0; i < i1; ++i) {
      // ELASTIC: the flag byte is asked for in front of the pod row, without a branch (no flags: a byte that is there anyway, masked
      // off below), and first looked at behind the verdict: one trip to memory with the row's
      uint32_t flag_byte = 0;
      int64_t p;
      if constexpr (ELASTIC) {  // (the row without a branch too, so that the two loads leave together)
        flag_byte = *(ga.member_flags ? ga.member_flags + i : (const uint8_t*)ga.gang_off);
        const int64_t r = *(a.rows ? a.rows + i : ga.gang_off);
        p = a.rows ? r : i;
      } else {
        p = a.rows ? a.rows[i] : i;
      }
      uint8_t* row = a.status + i * T;
      // ---- (1) affected throttles: nonzero bytes of the matrix row, 16 per lane and chunk
      bool err;
      const uint32_t n_aff = admit_affected(row, T, list, a.list_cap, &err);
      if (__ballot(err) != 0ull || !(admit_page(a.pages, 0).pod_flags[p] & kPodValid) || n_aff > a.list_cap) {
        // error row (selector / namespace error, plugin.go:154-168), empty row, or a pod affected by more
        // throttles than the list holds: the pre-computed summary stands and nothing is reserved
        if constexpr (GANGS) all_in = false;
        if constexpr (ELASTIC) required_out |= ga.member_flags && (flag_byte & 1u) != 0;
        continue;
      }
      // ---- (2) lane = (affected throttle, dimension), over every page
      uint32_t n_exc = 0, n_act = 0, n_ins = 0;
      for (uint32_t base = 0; base < n_aff; base += MPW) {
        const uint32_t j = base + ml;
        const bool vv = j < n_aff;
        const uint32_t t = list[vv ? j : 0u];
        uint32_t bits = 0;
        for (int k = 0; k < n_pages; ++k) {
          const AdmitPage pg = admit_page(a.pages, k);
          if (!vv) continue;
          const AdmitState<IN_LDS> st = state_of(pg);
          if (k == 0 && d == 0) bits |= admit_count_bits(pg.tt, st, t, eq);  // the same in every page
          bits |= admit_name_bits(pg, st, p, t, d, eq);
        }
#pragma unroll
        for (int o = DT / 2; o >= 1; o >>= 1) bits |= (uint32_t)__shfl_xor((int)bits, o);
        // ---- (3) the status the pod met on throttle t, the summary word as PreFilter would return it at this point
        const uint32_t stc = (bits & 1u) ? 4u : (bits & 2u) ? 2u : (bits & 4u) ? 3u : 1u;
        const bool lead = vv && d == 0;
        if (lead) row[t] = (uint8_t)stc;
        n_exc += (uint32_t)__popcll(__ballot(lead && stc == 4u));
        n_act += (uint32_t)__popcll(__ballot(lead && stc == 2u));
        n_ins += (uint32_t)__popcll(__ballot(lead && stc == 3u));
      }
      if constexpr (GANGS) {
        // the rollback asks this word whether the pod reserved: written and read through L2, as the HBM state is
        if (lane == 0) __hip_atomic_store(a.summary + i, pack_summary(n_exc, n_act, n_ins, false), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        if (lane == 0) a.summary[i] = pack_summary(n_exc, n_act, n_ins, false);
      }
      if ((n_exc | n_act | n_ins) != 0) {
        if constexpr (GANGS) all_in = false;
        if constexpr (ELASTIC) required_out |= ga.member_flags && (flag_byte & 1u) != 0;
        continue;
      }
      if constexpr (ELASTIC) n_in += 1;
      // ---- (4) Success: Reserve on every page
      if constexpr (GANGS) {  // the first touch of a throttle in this gang saves every page's presence word of it
        const uint32_t gt = (uint32_t)g + 1u;
        for (uint32_t j = lane; j < n_aff; j += kWave) {
          const uint32_t t = list[j];
          if (tag.ld(t) == gt) continue;
          for (int k = 0; k < n_pages; ++k) kept_of(k).st(t, state_of(admit_page(a.pages, k)).ld_p(t));
          tag.st(t, gt);
        }
      }
      for (int k = 0; k < n_pages; ++k) {
        const AdmitPage pg = admit_page(a.pages, k);
        admit_reserve<DT>(pg, state_of(pg), p, list, n_aff);
      }
    }
    if constexpr (GANGS) {
      bool kept = all_in;  // wave-uniform: the gang stays
      if constexpr (ELASTIC) {
        kept = n_in >= quorum && !required_out;
        if (lane == 0) ga.members_out[g] = kept ? n_in : 0;
      }
      if (lane == 0) ga.gang_out[g] = kept ? 1 : 0;
      if (!kept) {
        // ---- rolled back: Unreserve of every member that reserved.  A member reserved iff it was not skipped in (1) — decided
        //      again from the same inputs (an error byte is never rewritten, nonzero bytes stay nonzero) — and its summary word,
        //      read back through L2, says Success
        for (int64_t i = i0; i < i1; ++i) {
          const int64_t p = a.rows ? a.rows[i] : i;
          const uint64_t w = __hip_atomic_load(a.summary + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (beside the row's trip)
          bool err;
          const uint32_t n_aff = admit_affected(a.status + i * T, T, list, a.list_cap, &err);
          if (__ballot(err) != 0ull || !(admit_page(a.pages, 0).pod_flags[p] & kPodValid) || n_aff > a.list_cap) continue;
          if (__ballot(w != 0ull) != 0ull) continue;
          for (int k = 0; k < n_pages; ++k) {
            const AdmitPage pg = admit_page(a.pages, k);
            admit_unreserve<DT>(pg, state_of(pg), kept_of(k), p, list, n_aff);
          }
        }
      }
    }
  }
  if (a.commit)
    for (int k = 0; k < n_pages; ++k) {
      const AdmitPage pg = admit_page(a.pages, k);
      admit_store_state(state_of(pg), pg.tt, T, pg.D);
    }
}

// the three kernels: the plain queue, the queue in gangs, and the queue in elastic gangs
template <int DT, bool IN_LDS>
__global__ __launch_bounds__(kWave) void kt_admit(const AdmitPagedArgs a) {
  admit_walk<DT, IN_LDS, kAdmitQueue>(a, AdmitGangArgs{});
}
template <int DT, bool IN_LDS>
__global__ __launch_bounds__(kWave) void kt_admit_gangs(const AdmitPagedArgs a, const AdmitGangArgs ga) {
  admit_walk<DT, IN_LDS, kAdmitGangs>(a, ga);
}
template <int DT, bool IN_LDS>
__global__ __launch_bounds__(kWave) void kt_admit_gangs_elastic(const AdmitPagedArgs a, const AdmitGangArgs ga) {
  admit_walk<DT, IN_LDS, kAdmitElastic>(a, ga);
}

// LDS: state + list when the state fits, else the list alone
size_t admit_state_bytes(int T, int D) {
  return ((size_t)T * D * 8 + 15) / 16 * 16 + ((size_t)T * 8 + 15) / 16 * 16 + ((size_t)T * 4 + 15) / 16 * 16;
}

size_t admit_paged_state_bytes(int T, const AdmitPage* pages, int n_pages) {
  size_t b = 0;
  for (int k = 0; k < n_pages; ++k) b += admit_state_bytes(T, pages[k].D);
  return b;
}

// gangs (both forms): one saved copy of the presence words per page and the gang tags, beside the state (LDS or scratch)
size_t admit_gang_extra_bytes(int T, int n_pages) { return ((size_t)n_pages + 1) * (((size_t)T * 4 + 15) / 16 * 16); }

// scratch: admit_paged_state_bytes (+ admit_gang_extra_bytes with gangs) bytes of device memory, used when the state does not
// fit in LDS (or when forced).  gangs (nullable): the gang form, its extra state counted for it alone; with gangs->min_dev the
// elastic form (the same extra state)
bool launch_admit(AdmitPage* pages, int n_pages, AdmitPage* pages_dev, hipEvent_t pages_copied, int64_t n, const int64_t* rows_dev, int T,
                  bool on_equal, bool commit, uint8_t* status, uint64_t* summary, void* scratch, bool force_global, hipStream_t s,
                  hipError_t* hip_err, const AdmitGangs* gangs) {
  *hip_err = hipSuccess;
  const size_t list_bytes = ((size_t)T * 4 + 15) / 16 * 16;
  const size_t extra = gangs ? admit_gang_extra_bytes(T, n_pages) : 0;
  const bool in_lds = !force_global && admit_paged_state_bytes(T, pages, n_pages) + extra + list_bytes <= (size_t)kMaxLds;
  if (!in_lds && (!scratch || list_bytes > (size_t)kMaxLds)) return false;
  uint32_t o = 0;
  auto take = [&](size_t bytes) { uint32_t r = o; o += (uint32_t)((bytes + 15) & ~(size_t)15); return r; };
  int maxD = 1;
  for (int k = 0; k < n_pages; ++k) {  // offsets inside LDS or inside the scratch buffer, page after page
    pages[k].off_rv = take((size_t)T * pages[k].D * 8);
    pages[k].off_rc = take((size_t)T * 8);
    pages[k].off_rp = take((size_t)T * 4);
    maxD = pages[k].D > maxD ? pages[k].D : maxD;
  }
  AdmitPagedArgs a{};
  AdmitGangArgs ga{};
  if (gangs) {  // behind every page's state
    ga.rq_stride = (uint32_t)list_bytes;
    ga.off_rq = take(extra);
    ga.off_tag = ga.off_rq + (uint32_t)n_pages * ga.rq_stride;
    ga.gang_off = gangs->off_dev, ga.n_gangs = gangs->n_gangs, ga.gang_out = gangs->out_dev;
    ga.min_members = gangs->min_dev, ga.member_flags = gangs->flags_dev, ga.members_out = gangs->members_dev;
  }
  if (!in_lds) o = 0;
  a.pages = pages_dev, a.n_pages = n_pages, a.rows = rows_dev, a.n = n, a.scratch = (unsigned char*)scratch;
  a.status = status, a.summary = summary, a.T = T, a.on_equal = on_equal ? 1 : 0, a.commit = commit ? 1 : 0;
  a.list_cap = (uint32_t)T;  // a pod can be affected by every throttle
  a.off_list = take((size_t)a.list_cap * 4);
  const size_t lds_bytes = o;
  if ((*hip_err = hipMemcpyAsync(pages_dev, pages, sizeof(AdmitPage) * (size_t)n_pages, hipMemcpyHostToDevice, s)) != hipSuccess) return false;
  if ((*hip_err = hipEventRecord(pages_copied, s)) != hipSuccess) return false;
  const int DT = dt_bucket(maxD);
#define KT_ADMIT_CASE(DT_)                                                                                        \
  if (gangs && gangs->min_dev) {                                                                                 \
    auto kfn = in_lds ? kt_admit_gangs_elastic<DT_, true> : kt_admit_gangs_elastic<DT_, false>;                  \
    (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);     \
    hipLaunchKernelGGL(kfn, dim3(1), dim3(kWave), lds_bytes, s, a, ga);                                          \
  } else if (gangs) {                                                                                            \
    auto kfn = in_lds ? kt_admit_gangs<DT_, true> : kt_admit_gangs<DT_, false>;                                  \
    (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);     \
    hipLaunchKernelGGL(kfn, dim3(1), dim3(kWave), lds_bytes, s, a, ga);                                          \
  } else {                                                                                                       \
    auto kfn = in_lds ? kt_admit<DT_, true> : kt_admit<DT_, false>;                                              \
    (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);     \
    hipLaunchKernelGGL(kfn, dim3(1), dim3(kWave), lds_bytes, s, a);                                              \
  }
  if (DT == 4) KT_ADMIT_CASE(4) else if (DT == 8) KT_ADMIT_CASE(8) else KT_ADMIT_CASE(16)
#undef KT_ADMIT_CASE
  return true;
}

}  // namespace kt
