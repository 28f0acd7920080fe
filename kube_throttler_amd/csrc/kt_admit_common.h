// kt_admit_common.h — what the admission kernels (kt_kernels_admit.hip: kt_admit, kt_admit_gangs) and the headroom kernel
// (kt_kernels_headroom.hip: kt_headroom) share, gfx950: the affected-throttle list of a status-matrix row, the page descriptor
// by value, the effective threshold and step 3's isThrottledOnEqual of a throttle, the 128-bit comparison; and what the preemption
// kernels (kt_kernels_preempt.hip: kt_preempt, kt_kernels_reprieve.hip: kt_preempt_reprieve, kt_kernels_preempt_gangs.hip:
// kt_preempt_gangs) share: the four steps for one amount against `used` as it stands in some state, the wave scan, the chunk and
// grid sizes; and what kt_preempt and kt_preempt_gangs share on top: their arguments, the list cut, which rows keep their stored
// status and which threshold a check reads behind the reconcile, the pieces of the k >= 1 block body (a lane's candidate, the
// scans with their carries, `used` with a prefix gone against one amount) and the derivation of prefix and victim mask from the
// verdict bits; what kt_preempt_gangs and kt_preempt_gangs_reprieve share: the members of a gang in order on one throttle against one
// state of `used` (gang_walk); and what the two reprieve kernels (kt_preempt_reprieve, kt_kernels_preempt_gangs_reprieve.hip:
// kt_preempt_gangs_reprieve) share: arguments, the list's state in LDS or HBM with its sizes, the list (counted, then gathered) and
// the walk over the masked positions, generic in who is judged; and what the two forecast kernels (kt_kernels_forecast.hip,
// kt_kernels_forecast_paged.hip) share on top of the four steps: the comparison of two instants.  And what kt_headroom and
// kt_headroom_forecast (kt_kernels_headroom_forecast.hip) share: the closed form of one amount against a run of identical pods.  The page descriptors themselves
// (AdmitPage, PreemptPage) are host-visible: kt_launch.h.
#pragma once
#include <algorithm>
#include <type_traits>

#include "kt_index_device.h"

namespace kt {

// the sums of used + reserved (+ the pod) are formed in 128 bits: an all-reduced `used` may come close to int64's end
__device__ __forceinline__ bool admit_cmp(__int128 a, int64_t b, bool eq) { return eq ? a >= (__int128)b : a > (__int128)b; }

// The marked bytes (bit k of nzm: byte b0 + k) of every lane go behind n_aff in the list (ballot/mbcnt append; entries beyond
// list_cap are counted, not written); returns the wave-uniform new count
__device__ __forceinline__ uint32_t admit_append_marked(uint32_t nzm, int b0, lds_u32wp list, uint32_t list_cap, uint32_t n_aff) {
  while (__ballot(nzm != 0) != 0ull) {
    const bool has = nzm != 0;
    const uint32_t k = (uint32_t)__ffs((int)nzm) - 1u;
    nzm &= nzm - 1u;
    const uint64_t mk = __ballot(has);
    const uint32_t pos = n_aff + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
    if (has && pos < list_cap) list[pos] = (uint32_t)b0 + k;
    n_aff += (uint32_t)__popcll(mk);
  }
  return n_aff;
}

// One chunk (kWave x 16 bytes from byte c0) of a pod's status-matrix row: its nonzero bytes are appended to the
// affected-throttle list behind n_aff (16 bytes per lane, ballot/mbcnt append; entries beyond list_cap are counted, not
// written); returns the wave-uniform new count, *err |= the chunk holds an error byte (per lane: ballot it)
__device__ __forceinline__ uint32_t admit_affected_chunk(const uint8_t* row, int T, int c0, lds_u32wp list, uint32_t list_cap, uint32_t n_aff,
                                                         bool* err) {
  const uint32_t lane = threadIdx.x % kWave;
  const int b0 = c0 + (int)lane * 16;
  u32x4 v = {0u, 0u, 0u, 0u};
  if (b0 < T) v = *(const u32x4*)(row + b0);  // the buffer has slack past the last row
  uint32_t nzm = 0;                            // bit k: byte k is nonzero
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t byte = (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu;
    if (b0 + k < T && byte != 0) nzm |= 1u << k;
    *err |= (b0 + k < T) && byte == 255u;
  }
  return admit_append_marked(nzm, b0, list, list_cap, n_aff);
}

// The gang form: one chunk of the UNION of the rows of queue positions [i0, i1) — a byte counts when it is nonzero in some
// member's row; *err |= some member's row holds an error byte in the chunk (per lane: ballot it)
__device__ __forceinline__ uint32_t gang_affected_chunk(const uint8_t* status, int64_t i0, int64_t i1, int T, int c0, lds_u32wp list,
                                                        uint32_t list_cap, uint32_t n_aff, bool* err) {
  const uint32_t lane = threadIdx.x % kWave;
  const int b0 = c0 + (int)lane * 16;
  uint32_t nzm = 0;  // bit k: byte k is nonzero in some member's row
  if (b0 < T)
    for (int64_t i = i0; i < i1; ++i) {
      const u32x4 v = *(const u32x4*)(status + i * (int64_t)T + b0);  // the buffer has slack past the last row
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const uint32_t byte = (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu;
        if (b0 + k < T && byte != 0) nzm |= 1u << k;
        *err |= (b0 + k < T) && byte == 255u;
      }
    }
  return admit_append_marked(nzm, b0, list, list_cap, n_aff);
}

// (1) of a pod: the nonzero bytes of its status-matrix row -> the affected-throttle list, chunk after chunk; returns the
// wave-uniform count, *err = the row holds an error byte
__device__ __forceinline__ uint32_t admit_affected(const uint8_t* row, int T, lds_u32wp list, uint32_t list_cap, bool* err_out) {
  uint32_t n_aff = 0;  // wave-uniform
  bool err = false;
  for (int c0 = 0; c0 < T; c0 += kWave * 16) n_aff = admit_affected_chunk(row, T, c0, list, list_cap, n_aff, &err);
  *err_out = err;
  return n_aff;
}

// a page descriptor by value: read through the constant address space (nothing writes the descriptors while the kernel
// runs), so the wave-uniform fields come in with scalar loads into SGPRs
__device__ __forceinline__ AdmitPage admit_page(const AdmitPage* pages, int k) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ((const __attribute__((address_space(4))) AdmitPage*)pages)[k];
#else
  return pages[k];
#endif
}

// a PreemptPage descriptor by value in the same way (kt_kernels_preempt_paged.hip, kt_kernels_forecast_paged.hip)
__device__ __forceinline__ PreemptPage preempt_page(const PreemptPage* pages, int k) {
#if defined(__HIP_DEVICE_COMPILE__)
  return ((const __attribute__((address_space(4))) PreemptPage*)pages)[k];
#else
  return pages[k];
#endif
}

// threshold := status.calculatedThreshold if calculatedAt != zero else spec.threshold (throttle_types.go:129-132)
__device__ __forceinline__ const AmountTab& admit_threshold(const ThrTables& tt, uint32_t tf) { return (tf & kThrCalcAtNonzero) ? tt.calc : tt.spec; }
// isThrottledOnEqual of step 3: always for a Throttle, the caller's for a ClusterThrottle (throttle_types.go:143 vs
// clusterthrottle_types.go:45)
__device__ __forceinline__ bool admit_eq3(uint32_t tf, bool eq) { return (tf & kThrCluster) ? eq : true; }

constexpr int kPreemptChunk = kWave * 16;  // matrix bytes per chunk = entries the chunk list holds
constexpr int kPreemptMaxBlocks = 2048;    // 256 CUs x 8 one-wave workgroups; more preemptors than that: the grid strides
constexpr uint32_t kCounted = kPodValid | kPodSchedMatch | kPodScheduled;  // ... and not kPodFinished (throttle_controller.go:217-219)

// One amount of one throttle for the preemptor (a resource name it requests with vp != 0, or the pod count with vp = 1)
// against `used` as it stands in some S_k: does one of the four CheckThrottledFor steps stop the pod
__device__ __forceinline__ bool preempt_fails(int64_t vp, bool th_has, int64_t tv, bool flagged, bool u_pres, int64_t uv, bool r_has, int64_t rv,
                                              bool eq3, bool eq) {
  if (flagged) return true;   // step 2: status.throttled of the fresh reconcile
  if (!th_has) return false;  // the threshold does not name the amount
  if (vp > tv) return true;   // step 1
  const __int128 s = (__int128)(u_pres ? uv : 0) + (r_has ? rv : 0);
  if ((u_pres || r_has) && admit_cmp(s, tv, eq3)) return true;  // step 3
  return admit_cmp(s + vp, tv, eq);                             // step 4
}

// ---- what kt_headroom and kt_headroom_forecast share: the closed form of one amount ----------------------------------------------
// One amount of one throttle as a run of identical pods meets it: a resource name (v = the pod's request) or the pod count
// (v = 1).  Copy j (0-based) is checked against used + reserved + j * va, where va is what Reserve adds per admitted copy
// (admit_reserve: the request when the pod's presence bit is set), and from copy 1 on the amount is present in `reserved`
// because the pod brought it in.
struct HeadroomTerm {
  int64_t v, va, tv, uv, rv;
  bool th_has;    // the threshold names the amount
  bool present0;  // the amount is present in used or reserved before copy 0
  bool brings;    // an admitted copy makes it present in reserved
  bool flagged;   // step 2: status.throttled says so
  bool eq3, eq;   // isThrottledOnEqual of step 3 and of step 4
};
// the four CheckThrottledFor steps (throttle_types.go:128-153) of copy j: does it pass all of them
__device__ __forceinline__ bool headroom_passes(const HeadroomTerm& m, uint32_t j) {
  if (m.flagged) return false;  // step 2
  if (!m.th_has) return true;
  if (m.v > m.tv) return false;  // step 1
  const __int128 s = (__int128)m.uv + m.rv + (__int128)j * m.va;
  if ((m.present0 || (j > 0 && m.brings)) && admit_cmp(s, m.tv, m.eq3)) return false;  // step 3
  return !admit_cmp(s + m.v, m.tv, m.eq);                                                // step 4
}
// the largest h in [0, cap] with h * v <= room (v > 0, room >= 0).  cap * v is compared first, in 128 bits; below that the
// quotient is < cap <= 2^31 and is found by bisection: 31 multiplications, exact for every 128-bit room, no division
__device__ __forceinline__ uint32_t headroom_fit(__int128 room, int64_t v, uint32_t cap) {
  if ((__int128)cap * v <= room) return cap;
  uint32_t lo = 0, hi = cap;  // lo * v <= room < hi * v
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if ((__int128)mid * v <= room) lo = mid;
    else hi = mid;
  }
  return lo;
}
// the leading copies that pass.  Copy 0 is decided as it stands (its presence rule differs).  With va > 0 (then va == v) the
// sums grow: step 4 of copy j implies step 3 of copy j, so the copies that pass are those with
// used + reserved + (j + 1) v < tv (on_equal) or <= tv (not): floor((tv - used - reserved - on_equal) / v) of them.  With
// va <= 0 the sums do not grow: copies 1.. all fare as copy 1 does, or better.
__device__ __forceinline__ uint32_t headroom_of_term(const HeadroomTerm& m, uint32_t cap) {
  if (!headroom_passes(m, 0u)) return 0u;
  if (!m.th_has || m.va <= 0) return headroom_passes(m, 1u) ? cap : 1u;
  return headroom_fit((__int128)m.tv - m.uv - m.rv - (m.eq ? 1 : 0), m.v, cap);
}

// instant a <= instant b, (seconds, nanoseconds) each: the forecast kernels' override windows are inclusive at both ends
__device__ __forceinline__ bool forecast_le(int64_t as, int32_t an, int64_t bs, int32_t bn) { return as != bs ? as < bs : an <= bn; }

template <class V>
__device__ __forceinline__ V wave_inclusive_scan(V x, uint32_t lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const V y = __shfl_up(x, o);
    if (lane >= (uint32_t)o) x += y;
  }
  return x;
}

// ---- what kt_preempt and kt_preempt_gangs share --------------------------------------------------------------------------------
struct PreemptArgs {
  AdmitPage pg;                       // pod flags, request rows and the throttle tables of the engine (state offsets unused)
  const int64_t* rows;                // [n + m] pod table rows: the preemptors (the gangs' members), then the candidates
  int64_t n, m;
  const uint8_t* status;              // [n + m][T]
  const uint64_t* summary;            // [n + m]
  const unsigned long long* partial;  // [T][partial_stride(D)], exact contributor counts
  AmountTab calc;                     // the dry finalize's status.calculatedThreshold at `now`
  const uint8_t* calc_updated;        // [T] it replaces the stored one (calculatedAt := now)
  const uint8_t* error;               // [T] the reconcile is an error: the stored status stays
  int64_t* prefix;                    // [n] out ([n_gangs] for the gang form)
  uint8_t* victims;                   // [n][m] out (and the kernel's per-position verdict bits while it runs)
  int32_t T, on_equal;
};

// m_eff: the list ends before the first candidate whose PreFilter is an error or whose row is invalid (wave-uniform)
__device__ __forceinline__ int64_t preempt_m_eff(const PreemptArgs& a, uint32_t lane) {
  for (int64_t q0 = 0; q0 < a.m; q0 += kWave) {
    const int64_t q = q0 + lane;
    bool bad = false;
    if (q < a.m) bad = a.summary[a.n + q] == 2ull || !(a.pg.pod_flags[a.rows[a.n + q]] & kPodValid);
    const uint64_t mk = __ballot(bad);
    if (mk != 0ull) return q0 + (__ffsll((long long)mk) - 1);
  }
  return a.m;
}

// a throttle whose reconcile is an error keeps its stored status: nothing of it depends on k
__device__ __forceinline__ bool preempt_row_stored(uint32_t tf, uint8_t error_byte) {
  return error_byte != 0 || (tf & (kThrValid | kThrResponsible)) != (kThrValid | kThrResponsible);
}
// the threshold the check reads behind the reconcile: calculatedThreshold once calculatedAt is set, else spec
__device__ __forceinline__ const AmountTab& preempt_threshold(const ThrTables& tt, const AmountTab& calc, uint32_t tf, uint8_t calc_updated) {
  return ((tf & kThrCalcAtNonzero) || calc_updated) ? calc : tt.spec;
}

// the lane's candidate in a block of kWave positions, seen from throttle t: contrib = it is counted and t matches it
struct PreemptCand {
  int64_t c;
  uint32_t fl;
  bool in, contrib;
};
__device__ __forceinline__ PreemptCand preempt_cand(const PreemptArgs& a, uint32_t t, int64_t q, int64_t m_eff) {
  PreemptCand L;
  L.in = q < m_eff;
  L.c = L.in ? a.rows[a.n + q] : 0;
  L.fl = L.in ? a.pg.pod_flags[L.c] : 0u;
  const uint8_t sb = L.in ? a.status[(a.n + q) * (int64_t)a.T + t] : (uint8_t)0;
  L.contrib = L.in && (L.fl & (kCounted | kPodFinished)) == kCounted && sb != 0;
  return L;
}
// the counted pods of t among the candidates up to and including the lane's (the carry: those of the earlier blocks)
__device__ __forceinline__ int64_t preempt_scan_pods(const PreemptCand& L, uint32_t lane, int64_t& car) {
  const int64_t pre = car + (int64_t)wave_inclusive_scan<uint32_t>(L.contrib ? 1u : 0u, lane);
  car = __shfl(pre, kWave - 1);
  return pre;
}
// ... and of name d their value and how many of them carry it
__device__ __forceinline__ void preempt_scan_name(const PreemptArgs& a, const PreemptCand& L, int d, uint32_t lane, int64_t& car_v, uint32_t& car_c,
                                                  int64_t* pre_v, uint32_t* pre_c) {
  const bool has = L.contrib && (((L.fl >> kPresentShift) >> d) & 1u);
  const int64_t v = has ? a.pg.req[L.c * a.pg.DS + d] : 0;
  *pre_v = car_v + wave_inclusive_scan<int64_t>(v, lane);
  *pre_c = car_c + wave_inclusive_scan<uint32_t>(has ? 1u : 0u, lane);
  car_v = __shfl(*pre_v, kWave - 1), car_c = (uint32_t)__shfl((int)*pre_c, kWave - 1);
}
// `used` of a reconciled throttle with u_c counted pods left: the pod count against it (the fresh reconcile's throttled flag is
// IsThrottled(used, true) against the calculated threshold)
__device__ __forceinline__ bool preempt_count_fails(bool th_hc, int64_t th_c, bool c_hc, int64_t c_c, int64_t u_c, bool r_hc, int64_t r_c, bool eq3,
                                                    bool eq) {
  const bool u_hc = u_c > 0;
  return preempt_fails(1, th_hc, th_c, c_hc && u_hc && u_c >= c_c, u_hc, u_c, r_hc, r_c, eq3, eq);
}
// ... and a name the pod requests with vp: u_v its value in `used`, u_n how many remaining counted pods carry it (presence is
// exact: the name stays in `used` only while one does)
__device__ __forceinline__ bool preempt_name_fails(int64_t vp, bool th_has, int64_t tv, bool c_has, int64_t cv, int64_t u_v, int64_t u_n, bool r_has,
                                                   int64_t rv, bool eq3, bool eq) {
  const bool u_pr = u_n > 0;
  return preempt_fails(vp, th_has, tv, c_has && u_pr && u_v >= cv, u_pr, u_v, r_has, rv, eq3, eq);
}

// The verdict bits of a row of the victim buffer (bit 1: some pair fails at k = position + 1; bit 0: the candidate is counted and
// matched) -> the prefix (0 when nothing fails in S_0, else the first position whose fail bit is clear + 1, else -1; -1 at once
// when !ok) and the victim bytes in place: j < prefix && bit 0
__device__ __forceinline__ int64_t preempt_answer(uint8_t* vic, int64_t m, int64_t m_eff, bool ok, bool fail0, uint32_t lane) {
  int64_t ans = -1;
  if (ok) {
    if (!fail0) ans = 0;
    else
      for (int64_t q0 = 0; q0 < m_eff; q0 += kWave) {
        const int64_t q = q0 + lane;
        const uint64_t mk = __ballot(q < m_eff && !(vic[q] & 2u));
        if (mk != 0ull) {
          ans = q0 + __ffsll((long long)mk);  // the first passing position + 1 = the prefix length
          break;
        }
      }
  }
  for (int64_t q = lane; q < m; q += kWave) vic[q] = (q < ans && (vic[q] & 1u)) ? (uint8_t)1 : (uint8_t)0;
  return ans;
}

// ---- what kt_preempt_gangs and kt_preempt_gangs_reprieve share -----------------------------------------------------------------
// `used` of one throttle as a lane (or the whole wave) sees it in some state: what the four steps read of it
template <int DT>
struct GangUsed {
  bool c_flag, u_hc;     // the pod count: status.throttled, presence
  int64_t u_c;
  uint32_t flag_m, pr_m;  // per name: status.throttled, presence
  int64_t u_v[DT];
};

// the throttle as the members meet it: threshold, step 3's on-equal, the stored reserved row
template <int DT>
struct GangThr {
  bool th_hc, r_hc, eq3, eq;
  int64_t th_c, r_c;
  uint32_t th_p, r_p;
  int64_t tv[DT], rv[DT];
};

// The members [i0, i1) in order on throttle t against one state of `used`: the first queue position whose member t affects and
// stops (i1: none), every earlier member having reserved.  `a` is PreemptArgs or ReprieveArgs (page, rows, status matrix, T).
// kt_preempt_gangs calls it with a wave-uniform throttle (everything but `u` is uniform), the gang reprieve with the lane's own.
template <int DT, class ARGS>
__device__ __forceinline__ int64_t gang_walk(const ARGS& a, uint32_t t, int64_t i0, int64_t i1, const GangThr<DT>& g, const GangUsed<DT>& u) {
  const int D = a.pg.D, DS = a.pg.DS;
  int64_t rv[DT], rc = g.r_hc ? g.r_c : 0;
  uint32_t rp = g.r_p;
  bool rhc = g.r_hc;
#pragma unroll
  for (int d = 0; d < DT; ++d) rv[d] = ((g.r_p >> d) & 1u) ? g.rv[d] : 0;
  int64_t first = i1;
  for (int64_t i = i0; i < i1; ++i) {
    if (a.status[i * (int64_t)a.T + t] == 0) continue;  // t does not affect the member: no check, no reservation
    const int64_t p = a.rows[i];
    const uint32_t present = a.pg.pod_flags[p] >> kPresentShift;
    bool f = preempt_fails(1, g.th_hc, g.th_c, u.c_flag, u.u_hc, u.u_c, rhc, rc, g.eq3, g.eq);
#pragma unroll
    for (int d = 0; d < DT; ++d) {
      if (d >= D) continue;
      const int64_t vp = a.pg.req[p * DS + d];
      // a name the pod does not request passes every step
      if (vp != 0) f |= preempt_fails(vp, (g.th_p >> d) & 1u, g.tv[d], (u.flag_m >> d) & 1u, (u.pr_m >> d) & 1u, u.u_v[d], (rp >> d) & 1u, rv[d], g.eq3, g.eq);
      if ((present >> d) & 1u) rv[d] += vp;  // Reserve: the value of every name it carries ...
    }
    rp |= present & ((1u << D) - 1u);  // ... the presence of all of them, zero-valued ones included
    rc += 1, rhc = true;
    if (f && first == i1) first = i;
  }
  return first;
}

// ---- what kt_preempt_reprieve and kt_preempt_gangs_reprieve share --------------------------------------------------------------
constexpr int kReprieveLdsBytes = 16 * 1024;         // the list's state in LDS: 20 KiB per wave with the chunk list, 8 waves per CU
constexpr size_t kReprieveWsBudget = 64ull << 20;    // the HBM workspace of one launch: grid x slot bytes stay below (one slot at least)

__host__ __device__ inline uint32_t reprieve_entry_bytes(int D) { return 12u + 12u * (uint32_t)D; }
inline size_t reprieve_slot_bytes(int T, int D) { return ((size_t)T * reprieve_entry_bytes(D) + 15u) & ~(size_t)15u; }
// the grid over n preemptors (gangs): kPreemptMaxBlocks at the most, and where a list may outgrow LDS no more than the workspace
// budget has slots for
inline int reprieve_blocks(int T, int D, int64_t n, uint32_t lds_cap) {
  int64_t blocks = n < kPreemptMaxBlocks ? n : kPreemptMaxBlocks;
  if ((uint32_t)T > lds_cap) {  // a list may outgrow LDS: every workgroup owns a slot
    const int64_t fit = (int64_t)(kReprieveWsBudget / reprieve_slot_bytes(T, D));
    blocks = std::min(blocks, std::max<int64_t>(fit, 1));
  }
  return (int)std::max<int64_t>(blocks, 1);
}

struct ReprieveArgs {
  AdmitPage pg;                       // pod flags, request rows and the throttle tables of the engine (state offsets unused)
  const int64_t* rows;                // [n + m] pod table rows: the preemptors (the gangs' members), then the candidates
  int64_t n, m;
  const uint8_t* status;              // [n + m][T]
  const unsigned long long* partial;  // [T][partial_stride(D)], exact contributor counts
  AmountTab calc;                     // the dry finalize's status.calculatedThreshold at `now`
  const uint8_t* calc_updated;        // [T]
  const uint8_t* error;               // [T]
  const int64_t* prefix;              // [n] ([n_gangs]) as the prefix kernel left it
  uint8_t* victims;                   // [n][m] ([n_gangs][m]) in: the prefix mask, out: the reprieved set
  unsigned char* ws;                  // gridDim.x slots of ws_slot bytes (nullptr: T <= lds_cap, no list outgrows LDS)
  size_t ws_slot;
  int32_t T, on_equal;
  uint32_t lds_cap;                   // entries the LDS state holds
};

// the list's state, field by field, in LDS or in HBM
template <bool IN_LDS>
struct ReprieveState {
  typedef typename std::conditional<IN_LDS, KT_LDS int64_t*, int64_t*>::type p64;
  typedef typename std::conditional<IN_LDS, KT_LDS uint32_t*, uint32_t*>::type p32;
  typedef typename std::conditional<IN_LDS, KT_LDS unsigned char*, unsigned char*>::type pbyte;
  p64 pods;  // [cap] counted pods
  p64 uv;    // [D][cap] `used` value per resource name
  p32 uc;    // [D][cap] contributors per resource name
  p32 tl;    // [cap] throttle row
  uint32_t cap;
  __device__ __forceinline__ ReprieveState(pbyte base, uint32_t cap_, int D) : cap(cap_) {
    pods = (p64)base;
    uv = (p64)(base + (size_t)8 * cap_);
    uc = (p32)(base + (size_t)8 * cap_ * (1 + D));
    tl = uc + (size_t)D * cap_;
  }
};

// a throttle whose reconcile is an error (or that nobody reconciles) keeps its stored status: nothing of it depends on V
__device__ __forceinline__ bool reprieve_stored(const ReprieveArgs& a, uint32_t t) { return preempt_row_stored(a.pg.tt.flags[t], a.error[t]); }

// The affecting throttles that are reconciled — chunk(c0, list, &err) appends one chunk of the matrix row (of the union of the
// members' rows) to the chunk list: counted (ST = void) or gathered into the state with the aggregate's totals; returns the
// wave-uniform list length
template <int DT, bool GATHER, class ST, class CHUNK>
__device__ __forceinline__ uint32_t reprieve_list(const ReprieveArgs& a, const CHUNK& chunk, lds_u32wp list, ST* st, uint32_t lane) {
  const int T = a.T, D = a.pg.D;
  const int stride = partial_stride(D);
  uint32_t n_list = 0;
  for (int c0 = 0; c0 < T; c0 += kPreemptChunk) {
    bool err_c = false;  // (prefix > 0: the row holds no error byte)
    const uint32_t n_c = chunk(c0, list, &err_c);
    __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
    for (uint32_t a0 = 0; a0 < n_c; a0 += kWave) {
      const uint32_t ai = a0 + lane;
      const uint32_t t = ai < n_c ? list[ai] : 0u;
      const bool keep = ai < n_c && !reprieve_stored(a, t);
      const uint64_t mk = __ballot(keep);
      if constexpr (GATHER) {
        const uint32_t e = n_list + __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0u));
        if (keep && e < st->cap) {
          const unsigned long long* prow = a.partial + (size_t)t * stride;
          st->tl[e] = t;
          st->pods[e] = (int64_t)prow[partial_off_pods(D)];
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            if (d >= D) continue;
            st->uv[(size_t)d * st->cap + e] = (int64_t)prow[d];
            st->uc[(size_t)d * st->cap + e] = (uint32_t)prow[partial_off_presence(D) + d];
          }
        }
      }
      n_list += (uint32_t)__popcll(mk);
    }
    __syncthreads();  // the next chunk rewrites the chunk list
  }
  return n_list;
}

// The walk over the masked positions below k of one row of the victim buffer, on a gathered list.  `track`: the names whose state
// is kept (wave-uniform); judge.step<JUDGE, SIGN>(st, n_list, crow, cfl, cv, lane) is one candidate against the list — JUDGE: does
// some entry whose throttle matches it stop whoever is judged with the candidate back (per lane: balloted here), nothing is
// written; otherwise the candidate's amounts are added to (SIGN = 1) or taken off (SIGN = -1) the state of every such entry.
template <int DT, class ST, class JUDGE>
__device__ __forceinline__ void reprieve_walk_list(const ReprieveArgs& a, ST& st, uint32_t n_list, uint8_t* vic, int64_t k, uint32_t track,
                                                   const JUDGE& judge, uint32_t lane) {
  const int T = a.T, D = a.pg.D, DS = a.pg.DS;
  const int64_t n = a.n;
  int64_t cv[DT];
#pragma unroll
  for (int d = 0; d < DT; ++d) cv[d] = 0;
  // the masked positions of one block of 64 candidates: their rows and flags come in with one load each
  auto block = [&](int64_t q0, int64_t& c, uint32_t& fl) -> uint64_t {
    const int64_t q = q0 + lane;
    const bool in = q < k;
    const bool masked = in && vic[q] != 0;
    c = masked ? a.rows[n + q] : 0;
    fl = masked ? a.pg.pod_flags[c] : 0u;
    return __ballot(masked);
  };
  auto candidate = [&](int b, int64_t c, uint32_t fl, uint32_t& cfl) -> int64_t {
    const int64_t cb = __shfl(c, b);
    cfl = (uint32_t)__shfl((int)fl, b);
#pragma unroll
    for (int d = 0; d < DT; ++d)
      if (d < D && ((track >> d) & 1u) && (((cfl >> kPresentShift) >> d) & 1u)) cv[d] = a.pg.req[cb * DS + d];
    return cb;
  };
  // S_k: the totals minus every masked victim
  for (int64_t q0 = 0; q0 < k; q0 += kWave) {
    int64_t c;
    uint32_t fl, cfl;
    uint64_t mk = block(q0, c, fl);
    while (mk != 0ull) {
      const int b = __ffsll((long long)mk) - 1;
      mk &= mk - 1ull;
      candidate(b, c, fl, cfl);
      (void)judge.template step<false, -1>(st, n_list, a.status + (n + q0 + b) * (int64_t)T, cfl, cv, lane);
    }
  }
  // the walk: c_{k-1} first
  for (int64_t q0 = ((k - 1) / kWave) * kWave; q0 >= 0; q0 -= kWave) {
    int64_t c;
    uint32_t fl, cfl;
    uint64_t mk = block(q0, c, fl);
    while (mk != 0ull) {
      const int b = 63 - __clzll((long long)mk);
      mk &= ~(1ull << b);
      candidate(b, c, fl, cfl);
      const uint8_t* crow = a.status + (n + q0 + b) * (int64_t)T;
      const bool fail = judge.template step<true, 1>(st, n_list, crow, cfl, cv, lane);
      if (__ballot(fail) != 0ull) continue;  // c_j stays a victim
      (void)judge.template step<false, 1>(st, n_list, crow, cfl, cv, lane);
      if (lane == 0) vic[q0 + b] = 0;
    }
  }
}

}  // namespace kt
