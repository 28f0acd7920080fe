// kt_kernels_preempt_gangs_elastic.hip — the shortest victim prefix that lets a gang's QUORUM in (kt_preempt_gangs_elastic_launch), gfx950.
//
// kt_preempt_gangs (kt_kernels_preempt_gangs.hip) answers "which victims let the WHOLE gang in" in closed form, throttle by throttle
// over prefix sums.  The elastic rule — at least min_members members succeed, and every required one does — cannot be judged that
// way: a member that fails reserves on no throttle, so which members weigh on a throttle depends on k, and the verdict is not even
// monotone in k (a longer prefix can let a big optional member in, whose reservation then shuts a required one out).  The judge here
// is MEMBER-major, the state-and-member-loop pattern of kt_forecast_gangs_elastic (kt_kernels_forecast_gangs_elastic.hip) with the
// victim prefix where the instant stood: the state is built once per gang as S_0 and MOVED from S_{k-1} to S_k by candidate c_{k-1}.
//
//   input   as kt_preempt_gangs: status matrix and summary words of ONE check over members ++ candidates, the partial rows of an
//           aggregate with exact contributor counts, calc / calc_updated / error of a dry finalize at `now`, the stored tables, the
//           gang offsets; and the rule: min_members [n_gangs], member_flags [n] (nullable).  All read-only.
//   per gang (one wave, the grid strides)
//           (1) the UNION of the members' affecting throttles, chunk by chunk through the 4 KiB LDS list, into a compact STATE of one
//               entry per union throttle, built by the lane that owns it (entry mod 64): the throttle row, whether it keeps its
//               stored status, the threshold the check reads at `now`, the counted pods, per name the `used` value and the exact
//               contributor count (S_0 from the partial row), what the four steps read of them (status.throttled against the
//               calculated threshold, exact presence), and the running reserved amounts.  The row of an Error member is all error
//               bytes: it names no throttle, and is left out of the union (elastic_affected_chunk).
//           (2) the walk over k = 0 .. m_eff, wave-uniform.  For k > 0 the entries whose throttle matches c_{k-1} take the candidate
//               off, if it is counted, and recompute presence and the throttled flags; a stored-status entry never changes.  One
//               ballot tells whether the candidate touched the union: that is its victim bit, and if it did not the verdict of k - 1
//               stands.  Otherwise the judge: the reserved amounts are reset from the stored rows and the members go in order, one
//               ballot per member, Reserve on success only, every member evaluated.  The walk stops at the first k that passes;
//               nothing is bisected and k = m_eff is not probed first.
//           (3) with KT_PREEMPT_REPRIEVE, on the state the walk stands in: j = prefix - 1 .. 0 over the masked positions, c_j is put
//               back on the entries it matches, the gang is judged, and c_j stays back iff it passes — else it is taken off again.
//   output  lane 0: prefix[g], members[g] (the successes in the final state; in S_0 where there is no prefix), blocker[g] (-1 iff the
//           prefix is 0, else the first required member that does not succeed in S_0, else the first member that does not); the
//           victim bytes lane-parallel, position q by lane q mod 64 throughout.
//
// Where the state lives is kt_forecast_gangs_elastic's: kElasticPreemptLdsBytes of LDS while the union fits, else the workgroup's
// slot of an HBM workspace — the same code instantiated for both address spaces; LDS is tried first and the gang starts again in
// HBM when the union outgrows it (no output is written before the walk).  The state is laid out field by field; an entry is only
// ever read and written by the lane that built it.  No lane indexes private memory dynamically; sums are formed in 128 bits
// (preempt_fails).
#include "kt_admit_common.h"

namespace kt {

constexpr int kElasticPreemptLdsBytes = kReprieveLdsBytes;     // 20 KiB per wave with the chunk list: eight waves per CU
constexpr size_t kElasticPreemptWsBudget = kReprieveWsBudget;  // the HBM workspace of one launch: grid x slot bytes stay below (one slot at least)

__host__ __device__ inline uint32_t elastic_preempt_entry_bytes(int D) { return 48u + 28u * (uint32_t)D; }
inline size_t elastic_preempt_slot_bytes(int T, int D) { return ((size_t)T * elastic_preempt_entry_bytes(D) + 15u) & ~(size_t)15u; }

uint32_t preempt_gangs_elastic_lds_cap(int D, uint32_t limit) {
  const uint32_t cap = (uint32_t)kElasticPreemptLdsBytes / elastic_preempt_entry_bytes(D);
  return limit != 0 && limit < cap ? limit : cap;
}
// the grid over the gangs: kPreemptMaxBlocks at the most, and where a union may outgrow LDS no more than the workspace budget has
// slots for
static int elastic_preempt_blocks(int T, int D, int64_t n_gangs, uint32_t lds_cap) {
  int64_t blocks = n_gangs < kPreemptMaxBlocks ? n_gangs : kPreemptMaxBlocks;
  if ((uint32_t)T > lds_cap) {
    const int64_t fit = (int64_t)(kElasticPreemptWsBudget / elastic_preempt_slot_bytes(T, D));
    blocks = std::min(blocks, std::max<int64_t>(fit, 1));
  }
  return (int)std::max<int64_t>(blocks, 1);
}
size_t preempt_gangs_elastic_ws_bytes(int T, int D, int64_t n_gangs, uint32_t lds_cap_limit) {
  const uint32_t lds_cap = preempt_gangs_elastic_lds_cap(D, lds_cap_limit);
  if (n_gangs <= 0 || (uint32_t)T <= lds_cap) return 0;
  return (size_t)elastic_preempt_blocks(T, D, n_gangs, lds_cap) * elastic_preempt_slot_bytes(T, D);
}

struct PreemptGangElasticArgs {
  PreemptArgs p;                // kt_preempt_gangs' arguments: prefix [n_gangs] and victims [n_gangs][m] out
  const int64_t* gang_off;      // [n_gangs + 1] queue positions
  int64_t n_gangs;
  const int64_t* min_members;   // [n_gangs] the quorum
  const uint8_t* member_flags;  // [n] nullable: no member is required
  int64_t* members;             // [n_gangs] out
  int64_t* blocker;             // [n_gangs] out
  unsigned char* ws;            // gridDim.x slots of ws_slot bytes (nullptr: T <= lds_cap, no union outgrows LDS)
  size_t ws_slot;
  uint32_t lds_cap;             // entries the LDS state holds
  int32_t reprieve;
};

constexpr uint32_t kPeThHasCount = 0x1u, kPeCountFlag = 0x2u, kPeUsedHasCount = 0x4u, kPeEq3 = 0x8u, kPeResHasCount = 0x10u, kPeStored = 0x20u;

// the state of one gang, field by field, in LDS or in HBM
template <bool IN_LDS>
struct ElasticPreemptState {
  typedef typename std::conditional<IN_LDS, KT_LDS int64_t*, int64_t*>::type p64;
  typedef typename std::conditional<IN_LDS, KT_LDS uint32_t*, uint32_t*>::type p32;
  typedef typename std::conditional<IN_LDS, KT_LDS unsigned char*, unsigned char*>::type pbyte;
  p64 th_c, pods, r_c;  // [cap] the counts: the threshold the check reads, the counted pods (`used`), reserved
  p64 tv, uv, rv;       // [D][cap] per resource name: threshold, used, reserved
  p32 uc;               // [D][cap] contributors per resource name
  p32 tl, bits;         // [cap] throttle row, kPe*
  p32 th_p, fl_m, pr_m, r_p;  // [cap] per-name masks: the threshold names it, status.throttled, present in used, present in reserved
  uint32_t cap;
  __device__ __forceinline__ ElasticPreemptState(pbyte base, uint32_t cap_, int D) : cap(cap_) {
    th_c = (p64)base, pods = th_c + cap_, r_c = pods + cap_;
    tv = r_c + cap_, uv = tv + (size_t)D * cap_, rv = uv + (size_t)D * cap_;
    uc = (p32)(rv + (size_t)D * cap_);
    tl = uc + (size_t)D * cap_, bits = tl + cap_;
    th_p = bits + cap_, fl_m = th_p + cap_, pr_m = fl_m + cap_, r_p = pr_m + cap_;
  }
};

// One chunk of the union of the rows of queue positions [i0, i1), as gang_affected_chunk forms it, but a byte counts only when it
// names a throttle: the row of a member whose PreFilter is an Error holds the error byte in every column
__device__ __forceinline__ uint32_t elastic_affected_chunk(const uint8_t* status, int64_t i0, int64_t i1, int T, int c0, lds_u32wp list,
                                                           uint32_t list_cap) {
  const uint32_t lane = threadIdx.x % kWave;
  const int b0 = c0 + (int)lane * 16;
  uint32_t nzm = 0;  // bit k: byte k is a verdict in some member's row
  if (b0 < T)
    for (int64_t i = i0; i < i1; ++i) {
      const u32x4 v = *(const u32x4*)(status + i * (int64_t)T + b0);  // the buffer has slack past the last row
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const uint32_t byte = (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu;
        if (b0 + k < T && byte != 0 && byte != 255u) nzm |= 1u << k;
      }
    }
  return admit_append_marked(nzm, b0, list, list_cap, 0u);
}

// what the four steps read of a reconciled entry's `used`: the flags of a fresh reconcile of it, exact presence
template <int DT, class ST>
__device__ __forceinline__ void elastic_preempt_refresh(const PreemptGangElasticArgs& a, ST& st, uint32_t e, uint32_t t) {
  const int D = a.p.pg.D;
  const size_t cap = st.cap;
  const int64_t pods = st.pods[e];
  const uint32_t c_p = a.p.calc.present[t];
  uint32_t bits = st.bits[e] & ~(kPeCountFlag | kPeUsedHasCount);
  bits |= pods > 0 ? kPeUsedHasCount : 0u;
  bits |= (a.p.calc.has_count[t] != 0 && pods > 0 && pods >= a.p.calc.count[t]) ? kPeCountFlag : 0u;
  uint32_t pr_m = 0u, fl_m = 0u;
#pragma unroll
  for (int d = 0; d < DT; ++d) {
    if (d >= D) continue;
    // presence is exact: the name is in `used` while a counted pod carries it
    const bool pr = st.uc[(size_t)d * cap + e] > 0u;
    pr_m |= pr ? 1u << d : 0u;
    fl_m |= (((c_p >> d) & 1u) && pr && st.uv[(size_t)d * cap + e] >= a.p.calc.v[(size_t)t * D + d]) ? 1u << d : 0u;
  }
  st.bits[e] = bits, st.pr_m[e] = pr_m, st.fl_m[e] = fl_m;
}

// Entry e of the state := throttle t in S_0.  The lane's own throttle: every load is the lane's.
template <int DT, class ST>
__device__ __forceinline__ void elastic_preempt_entry(const PreemptGangElasticArgs& a, ST& st, uint32_t e, uint32_t t) {
  const int D = a.p.pg.D;
  const ThrTables& tt = a.p.pg.tt;
  const size_t cap = st.cap;
  const uint32_t tf = tt.flags[t];
  const bool stored = preempt_row_stored(tf, a.p.error[t]);
  const AmountTab& th = preempt_threshold(tt, a.p.calc, tf, a.p.calc_updated[t]);
  uint32_t bits = (admit_eq3(tf, a.p.on_equal != 0) ? kPeEq3 : 0u) | (stored ? kPeStored : 0u) | (th.has_count[t] != 0 ? kPeThHasCount : 0u);
  st.tl[e] = t;
  st.th_c[e] = th.count[t], st.th_p[e] = th.present[t];
#pragma unroll
  for (int d = 0; d < DT; ++d)
    if (d < D) st.tv[(size_t)d * cap + e] = th.v[(size_t)t * D + d];
  if (stored) {  // the stored status, in every S_k
    bits |= ((tf & kThrThrottledPod) ? kPeCountFlag : 0u) | (tt.used.has_count[t] != 0 ? kPeUsedHasCount : 0u);
    st.pods[e] = tt.used.count[t];
    st.fl_m[e] = tt.thrl_flag[t] & tt.thrl_has[t], st.pr_m[e] = tt.used.present[t];
#pragma unroll
    for (int d = 0; d < DT; ++d)
      if (d < D) st.uv[(size_t)d * cap + e] = tt.used.v[(size_t)t * D + d], st.uc[(size_t)d * cap + e] = 0u;
    st.bits[e] = bits;
    return;
  }
  const unsigned long long* prow = a.p.partial + (size_t)t * partial_stride(D);
  st.pods[e] = (int64_t)prow[partial_off_pods(D)];
#pragma unroll
  for (int d = 0; d < DT; ++d)
    if (d < D) st.uv[(size_t)d * cap + e] = (int64_t)prow[d], st.uc[(size_t)d * cap + e] = (uint32_t)prow[partial_off_presence(D) + d];
  st.bits[e] = bits;
  elastic_preempt_refresh<DT>(a, st, e, t);
}

// Candidate at list position q (counted; `cfl` its flags, cv the values of the names it carries) against the state: the entries
// whose throttle matches it take its amounts off (sign = -1) or back on (sign = 1) and recompute what the four steps read; an entry
// that keeps its stored status never changes.  Returns, per lane, whether one of its entries matches the candidate.
template <int DT, class ST>
__device__ __forceinline__ bool elastic_preempt_move(const PreemptGangElasticArgs& a, ST& st, uint32_t n_ent, int64_t q, uint32_t cfl,
                                                     const int64_t (&cv)[DT], int sign, uint32_t lane) {
  const int D = a.p.pg.D;
  const size_t cap = st.cap;
  const uint8_t* crow = a.p.status + (a.p.n + q) * (int64_t)a.p.T;
  bool touched = false;
  for (uint32_t e = lane; e < n_ent; e += kWave) {
    const uint32_t t = st.tl[e];
    if (crow[t] == 0) continue;
    touched = true;
    if (st.bits[e] & kPeStored) continue;
    st.pods[e] += sign;
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      if (d >= D || !(((cfl >> kPresentShift) >> d) & 1u)) continue;
      st.uv[(size_t)d * cap + e] += sign * cv[d];
      st.uc[(size_t)d * cap + e] += (uint32_t)sign;
    }
    elastic_preempt_refresh<DT>(a, st, e, t);
  }
  return touched;
}

// what one walk of the members says (wave-uniform)
struct ElasticWalk {
  int64_t n_ok, first_fail, first_req_fail;
  bool out_of_reach;  // members that never succeed put the rule out of reach: in every state
  bool pass;
};

// The judge: the members of the gang in order against the state as it stands.  The reserved amounts start from the stored rows;
// a member that succeeds reserves on every entry that affects it, one that fails reserves nowhere; every member is evaluated.
template <int DT, class ST>
__device__ __forceinline__ ElasticWalk elastic_preempt_judge(const PreemptGangElasticArgs& a, ST& st, uint32_t n_ent, int64_t gi, int64_t i0,
                                                             int64_t i1, uint32_t lane) {
  const int T = a.p.T, D = a.p.pg.D, DS = a.p.pg.DS;
  const bool eq = a.p.on_equal != 0;
  const ThrTables& tt = a.p.pg.tt;
  const size_t cap = st.cap;
  for (uint32_t e = lane; e < n_ent; e += kWave) {
    const uint32_t t = st.tl[e];
    const bool r_hc = tt.reserved.has_count[t] != 0;
    const uint32_t r_p = tt.reserved.present[t];
    st.r_c[e] = r_hc ? tt.reserved.count[t] : 0, st.r_p[e] = r_p;
    st.bits[e] = (st.bits[e] & ~kPeResHasCount) | (r_hc ? kPeResHasCount : 0u);
#pragma unroll
    for (int d = 0; d < DT; ++d)
      if (d < D) st.rv[(size_t)d * cap + e] = ((r_p >> d) & 1u) ? tt.reserved.v[(size_t)t * D + d] : 0;
  }
  const uint32_t dmask = (1u << D) - 1u;
  ElasticWalk w;
  w.n_ok = 0, w.first_fail = -1, w.first_req_fail = -1;
  int64_t n_never = 0;
  bool req_never = false;
  for (int64_t i = i0; i < i1; ++i) {  // (wave-uniform)
    const int64_t p = a.p.rows[i];
    const uint32_t pf = a.p.pg.pod_flags[p];
    const bool required = a.member_flags != nullptr && (a.member_flags[i] & 1u) != 0;
    const bool never = a.p.summary[i] == 2ull || !(pf & kPodValid);  // an Error or invalid member never succeeds
    bool ok = false;
    if (!never) {
      const uint8_t* srow = a.p.status + i * (int64_t)T;
      const uint32_t present = (pf >> kPresentShift) & dmask;
      bool fail = false;
      for (uint32_t e = lane; e < n_ent; e += kWave) {
        if (srow[st.tl[e]] == 0) continue;  // the throttle does not affect the member: no check, no reservation
        const uint32_t b = st.bits[e], th_p = st.th_p[e], fl_m = st.fl_m[e], pr_m = st.pr_m[e], r_p = st.r_p[e];
        const bool eq3 = (b & kPeEq3) != 0;
        fail |= preempt_fails(1, (b & kPeThHasCount) != 0, st.th_c[e], (b & kPeCountFlag) != 0, (b & kPeUsedHasCount) != 0, st.pods[e],
                              (b & kPeResHasCount) != 0, st.r_c[e], eq3, eq);
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          if (d >= D) continue;
          const int64_t vp = a.p.pg.req[p * DS + d];
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
            if (d < D && ((present >> d) & 1u)) st.rv[(size_t)d * cap + e] += a.p.pg.req[p * DS + d];  // the value of every name it carries ...
          st.r_p[e] |= present;                                                                      // ... the presence of all of them
          st.r_c[e] += 1, st.bits[e] |= kPeResHasCount;
        }
    }
    w.n_ok += ok ? 1 : 0, n_never += never ? 1 : 0, req_never |= never && required;
    if (!ok && w.first_fail < 0) w.first_fail = i;
    if (!ok && required && w.first_req_fail < 0) w.first_req_fail = i;
  }
  const int64_t quorum = a.min_members[gi];
  w.out_of_reach = req_never || (i1 - i0) - n_never < quorum;
  w.pass = !w.out_of_reach && w.n_ok >= quorum && w.first_req_fail < 0;
  return w;
}

// one gang on a state that holds its union.  false (wave-uniform): the union outgrows the state — nothing was written to the
// outputs, the caller takes the larger state
template <int DT, bool IN_LDS>
__device__ __forceinline__ bool elastic_preempt_gang(const PreemptGangElasticArgs& a, ElasticPreemptState<IN_LDS> st, lds_u32wp list, int64_t gi,
                                                     int64_t m_eff, uint32_t lane) {
  const int T = a.p.T, D = a.p.pg.D, DS = a.p.pg.DS;
  const int64_t i0 = a.gang_off[gi], i1 = a.gang_off[gi + 1];
  const int64_t m = a.p.m, n = a.p.n;
  // ---- (1) the union, entry by entry; entry e belongs to lane e mod 64 from the start
  uint32_t n_ent = 0;  // wave-uniform
  for (int c0 = 0; c0 < T; c0 += kPreemptChunk) {
    const uint32_t n_c = elastic_affected_chunk(a.p.status, i0, i1, T, c0, list, (uint32_t)kPreemptChunk);
    __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
    if (n_ent + n_c > st.cap) return false;  // (before an entry of the chunk is written: e < cap below)
    for (uint32_t e = n_ent + ((lane - n_ent) & (uint32_t)(kWave - 1)); e < n_ent + n_c; e += kWave)
      elastic_preempt_entry<DT>(a, st, e, list[e - n_ent]);
    n_ent += n_c;
    __syncthreads();  // the next chunk rewrites the list
  }
  uint8_t* vic = a.p.victims + gi * m;
  for (int64_t q = lane; q < m; q += kWave) vic[q] = 0;
  int64_t cv[DT];
#pragma unroll
  for (int d = 0; d < DT; ++d) cv[d] = 0;
  // the candidate at list position q, wave-uniform: its flags, and the values of the names it carries
  auto candidate = [&](int64_t q) -> uint32_t {
    const int64_t c = a.p.rows[n + q];
    const uint32_t cfl = a.p.pg.pod_flags[c];
#pragma unroll
    for (int d = 0; d < DT; ++d)
      if (d < D && (((cfl >> kPresentShift) >> d) & 1u)) cv[d] = a.p.pg.req[c * DS + d];
    return cfl;
  };
  // ---- (2) the walk: `k` is the state the entries stand in, `q` the list position whose candidate moves them next.  One judge for
  //      the walk and for the reprieve behind it: the loop chooses the move, judges, and draws the consequences
  int64_t prefix = -1, members = 0, blocker = -1;
  int64_t k = 0;       // the walk: S_k is the state
  bool back = false;   // the reprieve runs
  int64_t q0 = 0;      // the reprieve: the block of 64 positions being walked back
  uint64_t mk = 0ull;  // ... its masked positions not yet tried
  int64_t j = -1;      // ... the position put back tentatively
  uint64_t vbits = 0ull;  // the walk: victim bits of the block of 64 positions k - 1 lies in; the reprieve: the bits cleared in block q0
  for (;;) {
    if (!back && k > 0) {  // S_{k-1} -> S_k
      const int64_t q = k - 1;
      if ((q & (kWave - 1)) == 0) vbits = 0ull;
      const uint32_t cfl = candidate(q);
      bool touched = false;
      if ((cfl & (kCounted | kPodFinished)) == kCounted) touched = elastic_preempt_move<DT>(a, st, n_ent, q, cfl, cv, -1, lane);
      const bool any = __ballot(touched) != 0ull;
      vbits |= any ? 1ull << (q & (kWave - 1)) : 0ull;
      const bool last = k >= m_eff;
      if (!any) {  // the verdict of k - 1 stands: it did not pass
        if (((q & (kWave - 1)) == kWave - 1 || last) && ((vbits >> lane) & 1ull)) vic[(q & ~(int64_t)(kWave - 1)) + lane] = 1;
        if (last) break;
        ++k;
        continue;
      }
    }
    const ElasticWalk w = elastic_preempt_judge<DT>(a, st, n_ent, gi, i0, i1, lane);
    if (!back) {
      if (k == 0) {
        members = w.n_ok;
        blocker = w.first_req_fail >= 0 ? w.first_req_fail : w.first_fail;
      }
      const bool block_end = k > 0 && (((k - 1) & (kWave - 1)) == kWave - 1 || w.pass || k >= m_eff);
      if (block_end && ((vbits >> lane) & 1ull)) vic[((k - 1) & ~(int64_t)(kWave - 1)) + lane] = 1;
      if (w.pass) {
        prefix = k, members = w.n_ok;
        if (k == 0) blocker = -1;
        if (!a.reprieve || k == 0) break;
        back = true, q0 = ((k - 1) / kWave) * kWave + kWave, mk = 0ull, vbits = 0ull;  // (the first block is taken below)
      } else {
        if (w.out_of_reach || k >= m_eff) break;  // no state passes
        ++k;
        continue;
      }
    } else {
      if (w.pass) vbits |= 1ull << (j - q0), members = w.n_ok;  // c_j stays back
      else (void)elastic_preempt_move<DT>(a, st, n_ent, j, candidate(j), cv, -1, lane);
    }
    // ---- (3) the reprieve: the next masked position below, c_{prefix-1} first
    while (mk == 0ull) {
      if ((vbits >> lane) & 1ull) vic[q0 + lane] = 0;  // the positions of the block that stay back
      vbits = 0ull;
      q0 -= kWave;
      if (q0 < 0) break;
      const int64_t q = q0 + lane;
      mk = __ballot(q < prefix && vic[q] != 0);  // (written by this lane: position q is lane q mod 64's throughout)
    }
    if (q0 < 0) break;
    const int b = 63 - __clzll((long long)mk);
    mk &= ~(1ull << b);
    j = q0 + b;
    (void)elastic_preempt_move<DT>(a, st, n_ent, j, candidate(j), cv, 1, lane);  // (masked: counted, and it touches the union)
  }
  if (prefix < 0)  // no prefix: the bits the walk left are no victims
    for (int64_t q = lane; q < m; q += kWave) vic[q] = 0;
  if (lane == 0) a.p.prefix[gi] = prefix, a.members[gi] = members, a.blocker[gi] = blocker;
  return true;
}

template <int DT>
__global__ __launch_bounds__(kWave) void kt_preempt_gangs_elastic(const PreemptGangElasticArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  __shared__ __attribute__((aligned(16))) unsigned char state[kElasticPreemptLdsBytes];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int64_t m_eff = preempt_m_eff(a.p, lane);  // from the candidates' summary words and flags
  for (int64_t gi = blockIdx.x; gi < a.n_gangs; gi += gridDim.x) {  // (wave-uniform: one gang per wave and turn)
    // LDS first: a union that fits — the usual case, whatever T is — is scanned once.  One that outgrows it is found out before its
    // first entry beyond the capacity is written, and before any output is: the gang starts again on the workgroup's slot
    const bool done =
        elastic_preempt_gang<DT, true>(a, ElasticPreemptState<true>((KT_LDS unsigned char*)state, a.lds_cap, a.p.pg.D), list, gi, m_eff, lane);
    __syncthreads();  // the list and the state are rewritten
    if (!done && a.ws)  // (the launcher gives a workspace whenever T > lds_cap; the union holds T entries at the most)
      (void)elastic_preempt_gang<DT, false>(a, ElasticPreemptState<false>(a.ws + (size_t)blockIdx.x * a.ws_slot, (uint32_t)a.p.T, a.p.pg.D), list, gi,
                                            m_eff, lane);
    __syncthreads();  // the next gang rewrites the state
  }
}

void launch_preempt_gangs_elastic(const AdmitPage& pg, int64_t n, int64_t m, const int64_t* rows_dev, int64_t n_gangs, const int64_t* gang_off_dev,
                                  const int64_t* min_dev, const uint8_t* flags_dev, int T, bool on_equal, bool reprieve, const uint8_t* status,
                                  const uint64_t* summary, const unsigned long long* partial, const AmountTab& calc, const uint8_t* calc_updated,
                                  const uint8_t* error, int64_t* prefix, uint8_t* victims, int64_t* members, int64_t* blocker, void* ws,
                                  uint32_t lds_cap_limit, hipStream_t s) {
  if (n_gangs <= 0) return;
  PreemptGangElasticArgs a{};
  a.p.pg = pg, a.p.rows = rows_dev, a.p.n = n, a.p.m = m, a.p.status = status, a.p.summary = summary, a.p.partial = partial, a.p.calc = calc;
  a.p.calc_updated = calc_updated, a.p.error = error, a.p.prefix = prefix, a.p.victims = victims, a.p.T = T, a.p.on_equal = on_equal ? 1 : 0;
  a.gang_off = gang_off_dev, a.n_gangs = n_gangs, a.min_members = min_dev, a.member_flags = flags_dev, a.members = members, a.blocker = blocker;
  a.reprieve = reprieve ? 1 : 0;
  a.lds_cap = preempt_gangs_elastic_lds_cap(pg.D, lds_cap_limit);
  a.ws = (uint32_t)T > a.lds_cap ? (unsigned char*)ws : nullptr, a.ws_slot = elastic_preempt_slot_bytes(T, pg.D);
  const int blocks = elastic_preempt_blocks(T, pg.D, n_gangs, a.lds_cap);
  const int DT = dt_bucket(pg.D);
  if (DT == 4) hipLaunchKernelGGL(kt_preempt_gangs_elastic<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_preempt_gangs_elastic<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_preempt_gangs_elastic<16>, dim3(blocks), dim3(kWave), 0, s, a);
}

}  // namespace kt
