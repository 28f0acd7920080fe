// kt_kernels_forecast_gangs_elastic.hip — the first instant at which a gang's QUORUM fits (kt_forecast_gangs_elastic_launch), gfx950.
//
// kt_forecast_gangs (kt_kernels_forecast_gangs.hip) answers "when does the WHOLE gang fit": it walks the members throttle by throttle
// (gang_walk), every earlier member reserving, and stops at the first member a throttle stops.  An elastic judge has to count past
// that member, and past it the throttle-major decomposition is wrong: a member that fails on throttle A reserves nowhere, so it does
// not weigh on throttle B either, where a later member then passes — and which members fail depends on the instant.  The judge here
// is therefore MEMBER-major, as kt_admit's walk is: per (gang, instant) the members in order, each against the state R_{t_k} plus
// what the earlier members that SUCCEEDED reserved.
//
//   input   as kt_forecast_gangs: status matrix and summary words of ONE check over the members of all gangs, the partial rows of an
//           aggregate with exact contributor counts, the error bytes of a dry finalize, the stored tables, the instants, the gang
//           offsets; and the rule: min_members [n_gangs], member_flags [n] (nullable).  All read-only.
//   per (gang, instant) pair (one wave, the grid strides over the pairs: a gang's instants spread over the machine)
//           (1) the UNION of the members' affecting throttles, chunk by chunk through the 4 KiB LDS list (gang_affected_chunk), into a
//               compact STATE of one entry per union throttle.  The lane that will own the entry (entry mod 64) builds it: the
//               throttle row; what the four steps read at THIS instant — the threshold the check reads and the throttled bits of
//               CalculateThreshold at t_k against the fresh sums (kt_forecast_gangs' arithmetic with the lane's own loop over its
//               throttle's overrides; a throttle that keeps its stored status reads the stored tables); `used` from the partial row;
//               the running reserved amounts, started from the stored reserved row.
//           (2) the member loop, wave-uniform and in order.  A member whose PreFilter is an Error or whose row is invalid never
//               succeeds.  Otherwise the lanes run over the entries, 64 at a time; a lane whose throttle affects the member (the
//               status-matrix byte) evaluates the four steps for the count and every name the pod requests.  One ballot: the member
//               succeeds iff no lane fails, and then the same lanes add its Reserve to their entries.  A failed member writes nothing.
//   output  per pair, by lane 0: verdicts[g][k], members[g][k] (the successes), blocker[g][k].  first[g] comes from
//           kt_forecast_gangs_elastic_first behind it on the same stream (one wave per gang, a ballot over the verdict row in blocks
//           of 64): it does not depend on the order in which the pairs finish.
//
// Where the state lives: in kElasticLdsBytes of LDS while the union fits (forecast_gangs_elastic_lds_cap entries of 48 + 24 D bytes),
// else in the workgroup's slot of an HBM workspace (T entries: the union cannot be longer) — the same code instantiated for both
// address spaces, as kt_admit and the reprieve kernels do; the launcher sizes the grid so that the workspace stays within
// kElasticWsBudget.  The reprieve kernels count their list before they choose; here LDS is tried first and the pair starts again in
// HBM when the union outgrows it (it writes no output before the walk), so the usual pair scans the members' rows once.  The state
// is laid out field by field, so the 64 lanes of a step touch consecutive words.  An entry is only ever read and written by the
// lane that built it: nothing crosses lanes through the state, in LDS or in HBM.  No lane indexes private memory dynamically.
#include "kt_admit_common.h"

namespace kt {

constexpr int kElasticLdsBytes = kReprieveLdsBytes;     // 20 KiB per wave with the chunk list: eight waves per CU
constexpr size_t kElasticWsBudget = kReprieveWsBudget;  // the HBM workspace of one launch: grid x slot bytes stay below (one slot at least)

__host__ __device__ inline uint32_t elastic_entry_bytes(int D) { return 48u + 24u * (uint32_t)D; }
inline size_t elastic_slot_bytes(int T, int D) { return ((size_t)T * elastic_entry_bytes(D) + 15u) & ~(size_t)15u; }

uint32_t forecast_gangs_elastic_lds_cap(int D, uint32_t limit) {
  const uint32_t cap = (uint32_t)kElasticLdsBytes / elastic_entry_bytes(D);
  return limit != 0 && limit < cap ? limit : cap;
}
// the grid over the (gang, instant) pairs: kPreemptMaxBlocks at the most, and where a union may outgrow LDS no more than the
// workspace budget has slots for
static int elastic_blocks(int T, int D, int64_t pairs, uint32_t lds_cap) {
  int64_t blocks = pairs < kPreemptMaxBlocks ? pairs : kPreemptMaxBlocks;
  if ((uint32_t)T > lds_cap) {
    const int64_t fit = (int64_t)(kElasticWsBudget / elastic_slot_bytes(T, D));
    blocks = std::min(blocks, std::max<int64_t>(fit, 1));
  }
  return (int)std::max<int64_t>(blocks, 1);
}
size_t forecast_gangs_elastic_ws_bytes(int T, int D, int64_t n_gangs, int64_t m, uint32_t lds_cap_limit) {
  const uint32_t lds_cap = forecast_gangs_elastic_lds_cap(D, lds_cap_limit);
  if (n_gangs <= 0 || m <= 0 || (uint32_t)T <= lds_cap) return 0;
  return (size_t)elastic_blocks(T, D, n_gangs * m, lds_cap) * elastic_slot_bytes(T, D);
}

struct ForecastGangElasticArgs {
  AdmitPage pg;                       // pod flags, request rows and the throttle tables of the engine (state offsets unused)
  const int64_t* rows;                // [n] pod table rows: the members of all gangs
  const int64_t* gang_off;            // [n_gangs + 1] queue positions
  int64_t n_gangs, m;                 // gangs, instants
  const int64_t* inst_s;              // [m] strictly ascending
  const int32_t* inst_ns;             // [m]
  const uint8_t* status;              // [n][T]
  const uint64_t* summary;            // [n]
  const unsigned long long* partial;  // [T][partial_stride(D)], exact contributor counts
  const uint8_t* error;               // [T] the reconcile is an error: the stored status stays
  const int64_t* min_members;         // [n_gangs] the quorum
  const uint8_t* member_flags;        // [n] nullable: no member is required
  int64_t* first;                     // [n_gangs] out (kt_forecast_gangs_elastic_first)
  uint8_t* verdicts;                  // [n_gangs][m] out
  int64_t* members;                   // [n_gangs][m] out
  int64_t* blocker;                   // [n_gangs][m] out
  unsigned char* ws;                  // gridDim.x slots of ws_slot bytes (nullptr: T <= lds_cap, no union outgrows LDS)
  size_t ws_slot;
  int32_t T, on_equal;
  uint32_t lds_cap;                   // entries the LDS state holds
};

constexpr uint32_t kEntThHasCount = 0x1u, kEntCountFlag = 0x2u, kEntUsedHasCount = 0x4u, kEntEq3 = 0x8u, kEntResHasCount = 0x10u;

// the state of one pair, field by field, in LDS or in HBM: per entry what the four steps read of its throttle at the pair's instant
// and the running reserved amounts
template <bool IN_LDS>
struct ElasticState {
  typedef typename std::conditional<IN_LDS, KT_LDS int64_t*, int64_t*>::type p64;
  typedef typename std::conditional<IN_LDS, KT_LDS uint32_t*, uint32_t*>::type p32;
  typedef typename std::conditional<IN_LDS, KT_LDS unsigned char*, unsigned char*>::type pbyte;
  p64 th_c, u_c, r_c;  // [cap] the counts: threshold, used, reserved
  p64 tv, uv, rv;      // [D][cap] per resource name: threshold, used, reserved
  p32 tl, bits;        // [cap] throttle row, kEnt*
  p32 th_p, fl_m, pr_m, r_p;  // [cap] per-name masks: the threshold names it, status.throttled, present in used, present in reserved
  uint32_t cap;
  __device__ __forceinline__ ElasticState(pbyte base, uint32_t cap_, int D) : cap(cap_) {
    th_c = (p64)base, u_c = th_c + cap_, r_c = u_c + cap_;
    tv = r_c + cap_, uv = tv + (size_t)D * cap_, rv = uv + (size_t)D * cap_;
    tl = (p32)(rv + (size_t)D * cap_), bits = tl + cap_;
    th_p = bits + cap_, fl_m = th_p + cap_, pr_m = fl_m + cap_, r_p = pr_m + cap_;
  }
};

// Entry e of the state := throttle t as the members meet it at the instant (ts, tn).  The lane's own throttle: every load is the
// lane's, the loop over the overrides too.
template <int DT, class ST>
__device__ __forceinline__ void elastic_entry(const ForecastGangElasticArgs& a, ST& st, uint32_t e, uint32_t t, int64_t ts, int32_t tn) {
  const int D = a.pg.D;
  const bool eq = a.on_equal != 0;
  const ThrTables& tt = a.pg.tt;
  const size_t cap = st.cap;
  const uint32_t tf = tt.flags[t];
  const uint32_t r_p = tt.reserved.present[t];
  const bool r_hc = tt.reserved.has_count[t] != 0;
  uint32_t bits = (admit_eq3(tf, eq) ? kEntEq3 : 0u) | (r_hc ? kEntResHasCount : 0u);
  st.tl[e] = t;
  st.r_p[e] = r_p;
  st.r_c[e] = r_hc ? tt.reserved.count[t] : 0;
#pragma unroll
  for (int d = 0; d < DT; ++d)
    if (d < D) st.rv[(size_t)d * cap + e] = ((r_p >> d) & 1u) ? tt.reserved.v[(size_t)t * D + d] : 0;
  if (preempt_row_stored(tf, a.error[t])) {  // nothing of it depends on the instant: the stored tables
    const AmountTab& th = admit_threshold(tt, tf);
    bits |= (th.has_count[t] != 0 ? kEntThHasCount : 0u) | ((tf & kThrThrottledPod) ? kEntCountFlag : 0u) |
            (tt.used.has_count[t] != 0 ? kEntUsedHasCount : 0u);
    st.th_c[e] = th.count[t], st.u_c[e] = tt.used.count[t];
    st.th_p[e] = th.present[t], st.fl_m[e] = tt.thrl_flag[t] & tt.thrl_has[t], st.pr_m[e] = tt.used.present[t];
#pragma unroll
    for (int d = 0; d < DT; ++d)
      if (d < D) st.tv[(size_t)d * cap + e] = th.v[(size_t)t * D + d], st.uv[(size_t)d * cap + e] = tt.used.v[(size_t)t * D + d];
    st.bits[e] = bits;
    return;
  }
  // ---- a reconciled throttle: CalculateThreshold at (ts, tn) — first active override wins, per name and for the count
  const uint32_t ovr0 = tt.ovr_off[t], ovr1 = tt.ovr_off[t + 1];
  const bool s_hc = tt.spec.has_count[t] != 0, k_hc = tt.calc.has_count[t] != 0;
  const int64_t s_c = tt.spec.count[t], k_c = tt.calc.count[t];
  const uint32_t s_p = tt.spec.present[t], k_p = tt.calc.present[t];
  bool any_err = false, active_found = false, c_hc = false, diff = false;
  int64_t c_c = 0, c_v[DT];
  uint32_t c_p = 0;
#pragma unroll
  for (int d = 0; d < DT; ++d) c_v[d] = 0;
  for (uint32_t o = ovr0; o < ovr1; ++o) {
    if (tt.ovr_flags[o] & kOvrParseError) {  // (the messages of CalculateThreshold: they do not depend on the instant)
      any_err = true;
      continue;
    }
    const int64_t ob_s = tt.ovr_begin_s[o], oe_s = tt.ovr_end_s[o];
    const int32_t ob_ns = tt.ovr_begin_ns[o], oe_ns = tt.ovr_end_ns[o];
    const bool end_zero = oe_s == kZeroTimeS && oe_ns == 0;
    if (!(forecast_le(ob_s, ob_ns, ts, tn) && (end_zero || forecast_le(ts, tn, oe_s, oe_ns)))) continue;
    active_found = true;
    if (!c_hc && tt.ovr_thr.has_count[o] != 0) c_hc = true, c_c = tt.ovr_thr.count[o];
    const uint32_t take = tt.ovr_thr.present[o] & ~c_p;  // the names this override decides
    c_p |= take;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      if (d >= D || !((take >> d) & 1u)) continue;
      c_v[d] = tt.ovr_thr.v[(size_t)o * D + d];
      diff |= c_v[d] != tt.calc.v[(size_t)t * D + d];
    }
  }
  if (!active_found) {  // no active override: spec.threshold; otherwise the merged override REPLACES it
    c_p = s_p, c_hc = s_hc, c_c = s_c;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      if (d >= D) continue;
      c_v[d] = tt.spec.v[(size_t)t * D + d];
      diff |= ((s_p >> d) & 1u) && c_v[d] != tt.calc.v[(size_t)t * D + d];
    }
  }
  // ---- replace the stored calculatedThreshold only if threshold or messages differ by value
  const bool fp_differs = tt.status_msgs_fp[t] != (any_err ? tt.spec_msgs_fp[t] : 0ull);
  const bool same = (c_hc == k_hc) && (!c_hc || c_c == k_c) && c_p == k_p && !diff;
  // ---- the threshold the check reads behind this reconcile: calculatedThreshold once calculatedAt is set, else spec
  const bool reads_calc = (tf & kThrCalcAtNonzero) || !same || fp_differs;
  // ---- `used` of the fresh aggregate, and throttled = calculatedThreshold.IsThrottled(used, true)
  const unsigned long long* prow = a.partial + (size_t)t * partial_stride(D);
  const int64_t pods_total = (int64_t)prow[partial_off_pods(D)];
  bits |= ((reads_calc ? c_hc : s_hc) ? kEntThHasCount : 0u) | ((c_hc && pods_total > 0 && pods_total >= c_c) ? kEntCountFlag : 0u) |
          (pods_total > 0 ? kEntUsedHasCount : 0u);
  st.th_c[e] = reads_calc ? c_c : s_c, st.u_c[e] = pods_total;
  st.th_p[e] = reads_calc ? c_p : s_p;
  uint32_t pr_m = 0u, fl_m = 0u;
#pragma unroll
  for (int d = 0; d < DT; ++d) {
    if (d >= D) continue;
    const int64_t u_v = (int64_t)prow[d];
    // a key is present when some counted pod carried it (as kt_finalize: the contributor count, or a non-zero sum)
    const bool pr = prow[partial_off_presence(D) + d] != 0ull || u_v != 0;
    pr_m |= pr ? 1u << d : 0u;
    fl_m |= (((c_p >> d) & 1u) && pr && u_v >= c_v[d]) ? 1u << d : 0u;
    st.tv[(size_t)d * cap + e] = reads_calc ? c_v[d] : tt.spec.v[(size_t)t * D + d];
    st.uv[(size_t)d * cap + e] = u_v;
  }
  st.pr_m[e] = pr_m, st.fl_m[e] = fl_m, st.bits[e] = bits;
}

// one (gang, instant) pair on a state that holds its union.  false (wave-uniform): the union outgrows the state — nothing was
// written to the outputs, the caller takes the larger state
template <int DT, bool IN_LDS>
__device__ __forceinline__ bool elastic_pair(const ForecastGangElasticArgs& a, ElasticState<IN_LDS> st, lds_u32wp list, int64_t gi, int64_t k,
                                             uint32_t lane) {
  const int T = a.T, D = a.pg.D, DS = a.pg.DS;
  const bool eq = a.on_equal != 0;
  const size_t cap = st.cap;
  const int64_t i0 = a.gang_off[gi], i1 = a.gang_off[gi + 1];
  const int64_t ts = a.inst_s[k];
  const int32_t tn = a.inst_ns[k];
  // ---- (1) the union, entry by entry; entry e belongs to lane e mod 64 from the start
  uint32_t n_ent = 0;  // wave-uniform
  for (int c0 = 0; c0 < T; c0 += kPreemptChunk) {
    bool err_c = false;  // (an Error member is known by its summary word)
    const uint32_t n_c = gang_affected_chunk(a.status, i0, i1, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
    __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
    if (n_ent + n_c > st.cap) return false;  // (before an entry of the chunk is written: e < cap below)
    for (uint32_t e = n_ent + ((lane - n_ent) & (uint32_t)(kWave - 1)); e < n_ent + n_c; e += kWave)
      elastic_entry<DT>(a, st, e, list[e - n_ent], ts, tn);
    n_ent += n_c;
    __syncthreads();  // the next chunk rewrites the list
  }
  // ---- (2) the members in order
  const uint32_t dmask = (1u << D) - 1u;
  int64_t n_ok = 0, n_never = 0, first_fail = -1, first_req_fail = -1;
  bool req_never = false;
  for (int64_t i = i0; i < i1; ++i) {  // (wave-uniform)
    const int64_t p = a.rows[i];
    const uint32_t pf = a.pg.pod_flags[p];
    const bool required = a.member_flags != nullptr && (a.member_flags[i] & 1u) != 0;
    const bool never = a.summary[i] == 2ull || !(pf & kPodValid);
    bool ok = false;
    if (!never) {
      const uint8_t* srow = a.status + i * (int64_t)T;
      const uint32_t present = (pf >> kPresentShift) & dmask;
      bool fail = false;
      for (uint32_t e = lane; e < n_ent; e += kWave) {
        if (srow[st.tl[e]] == 0) continue;  // the throttle does not affect the member: no check, no reservation
        const uint32_t b = st.bits[e], th_p = st.th_p[e], fl_m = st.fl_m[e], pr_m = st.pr_m[e], r_p = st.r_p[e];
        const bool eq3 = (b & kEntEq3) != 0;
        fail |= preempt_fails(1, (b & kEntThHasCount) != 0, st.th_c[e], (b & kEntCountFlag) != 0, (b & kEntUsedHasCount) != 0, st.u_c[e],
                              (b & kEntResHasCount) != 0, st.r_c[e], eq3, eq);
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          if (d >= D) continue;
          const int64_t vp = a.pg.req[p * DS + d];
          // a name the pod does not request passes every step
          if (vp != 0)
            fail |= preempt_fails(vp, (th_p >> d) & 1u, st.tv[(size_t)d * cap + e], (fl_m >> d) & 1u, (pr_m >> d) & 1u, st.uv[(size_t)d * cap + e],
                                  (r_p >> d) & 1u, st.rv[(size_t)d * cap + e], eq3, eq);
        }
      }
      ok = __ballot(fail) == 0ull;
      if (ok)  // Reserve on every throttle that affects it
        for (uint32_t e = lane; e < n_ent; e += kWave) {
          if (srow[st.tl[e]] == 0) continue;
#pragma unroll
          for (int d = 0; d < DT; ++d)
            if (d < D && ((present >> d) & 1u)) st.rv[(size_t)d * cap + e] += a.pg.req[p * DS + d];  // the value of every name it carries ...
          st.r_p[e] |= present;                                                                    // ... the presence of all of them
          st.r_c[e] += 1, st.bits[e] |= kEntResHasCount;
        }
    }
    n_ok += ok ? 1 : 0, n_never += never ? 1 : 0, req_never |= never && required;
    if (!ok && first_fail < 0) first_fail = i;
    if (!ok && required && first_req_fail < 0) first_req_fail = i;
  }
  // ---- the rule
  if (lane == 0) {
    const int64_t quorum = a.min_members[gi];
    const bool err = req_never || (i1 - i0) - n_never < quorum;  // members that never succeed put the rule out of reach
    const bool pass = !err && n_ok >= quorum && first_req_fail < 0;
    a.verdicts[gi * a.m + k] = err ? (uint8_t)2 : pass ? (uint8_t)0 : (uint8_t)1;
    a.members[gi * a.m + k] = n_ok;
    a.blocker[gi * a.m + k] = pass ? -1 : first_req_fail >= 0 ? first_req_fail : first_fail;
  }
  return true;
}

template <int DT>
__global__ __launch_bounds__(kWave) void kt_forecast_gangs_elastic(const ForecastGangElasticArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  __shared__ __attribute__((aligned(16))) unsigned char state[kElasticLdsBytes];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int64_t pairs = a.n_gangs * a.m;
  for (int64_t pi = blockIdx.x; pi < pairs; pi += gridDim.x) {  // (wave-uniform: one pair per wave and turn)
    const int64_t gi = pi / a.m, k = pi - gi * a.m;
    // LDS first: a union that fits — the usual case, whatever T is — is scanned once.  One that outgrows it is found out before its
    // first entry beyond the capacity is written, and before any output is: the pair starts again on the workgroup's slot
    const bool done = elastic_pair<DT, true>(a, ElasticState<true>((KT_LDS unsigned char*)state, a.lds_cap, a.pg.D), list, gi, k, lane);
    __syncthreads();  // the list and the state are rewritten
    if (!done && a.ws)  // (the launcher gives a workspace whenever T > lds_cap; the union holds T entries at the most)
      (void)elastic_pair<DT, false>(a, ElasticState<false>(a.ws + (size_t)blockIdx.x * a.ws_slot, (uint32_t)a.T, a.pg.D), list, gi, k, lane);
    __syncthreads();  // the next pair rewrites the state
  }
}

// first[g] = the first position of verdict row g whose byte is Success, or -1: one wave per gang, the grid strides
__global__ __launch_bounds__(kWave) void kt_forecast_gangs_elastic_first(const uint8_t* verdicts, int64_t n_gangs, int64_t m, int64_t* first) {
  const uint32_t lane = threadIdx.x;
  for (int64_t gi = blockIdx.x; gi < n_gangs; gi += gridDim.x) {
    const uint8_t* ver = verdicts + gi * m;
    int64_t ans = -1;
    for (int64_t q0 = 0; q0 < m; q0 += kWave) {
      const int64_t q = q0 + lane;
      const uint64_t mk = __ballot(q < m && ver[q] == 0);
      if (mk != 0ull) {
        ans = q0 + (__ffsll((long long)mk) - 1);
        break;
      }
    }
    if (lane == 0) first[gi] = ans;
  }
}

void launch_forecast_gangs_elastic(const AdmitPage& pg, int64_t n_gangs, int64_t m, const int64_t* rows_dev, const int64_t* gang_off_dev,
                                   const int64_t* min_dev, const uint8_t* flags_dev, const int64_t* inst_s, const int32_t* inst_ns, int T,
                                   bool on_equal, const uint8_t* status, const uint64_t* summary, const unsigned long long* partial,
                                   const uint8_t* error, int64_t* first, uint8_t* verdicts, int64_t* members, int64_t* blocker, void* ws,
                                   uint32_t lds_cap_limit, hipStream_t s) {
  if (n_gangs <= 0 || m <= 0) return;
  ForecastGangElasticArgs a{};
  a.pg = pg, a.rows = rows_dev, a.gang_off = gang_off_dev, a.n_gangs = n_gangs, a.m = m, a.inst_s = inst_s, a.inst_ns = inst_ns;
  a.status = status, a.summary = summary, a.partial = partial, a.error = error, a.min_members = min_dev, a.member_flags = flags_dev;
  a.first = first, a.verdicts = verdicts, a.members = members, a.blocker = blocker;
  a.T = T, a.on_equal = on_equal ? 1 : 0;
  a.lds_cap = forecast_gangs_elastic_lds_cap(pg.D, lds_cap_limit);
  a.ws = (uint32_t)T > a.lds_cap ? (unsigned char*)ws : nullptr, a.ws_slot = elastic_slot_bytes(T, pg.D);
  const int blocks = elastic_blocks(T, pg.D, n_gangs * m, a.lds_cap);
  const int DT = dt_bucket(pg.D);
  if (DT == 4) hipLaunchKernelGGL(kt_forecast_gangs_elastic<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_forecast_gangs_elastic<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_forecast_gangs_elastic<16>, dim3(blocks), dim3(kWave), 0, s, a);
  const int blocks_first = (int)(n_gangs < kPreemptMaxBlocks ? n_gangs : kPreemptMaxBlocks);
  hipLaunchKernelGGL(kt_forecast_gangs_elastic_first, dim3(blocks_first), dim3(kWave), 0, s, (const uint8_t*)verdicts, n_gangs, m, first);
}

}  // namespace kt
