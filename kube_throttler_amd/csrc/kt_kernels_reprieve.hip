// kt_kernels_reprieve.hip — the reprieve pass behind the victim prefix (kt_preempt_reprieve_launch), gfx950.
//
// kt_preempt left, per preemptor p, the prefix length k and the mask M of the counted candidates below k that a throttle
// affecting p matches.  The pass is kube-scheduler's selectVictimsOnNode, second half: start from "all of M removed" and put the
// victims back one by one, c_{k-1} first, keeping each back as long as PreFilter(p) is still Success against a fresh reconcile
// at `now`.  The definition is the walk itself, step by step: nothing is assumed about the signs of requests.
//
//   input   everything kt_preempt reads (status matrix and summary of ONE check over preemptors ++ candidates, pod flags and
//           request rows, the partial rows with exact contributor counts, the dry finalize's threshold with its calc_updated /
//           error bytes, the stored tables), prefix[] and victims[][] as kt_preempt left them.
//   per preemptor (one wave, the grid strides; prefix <= 0 costs the one load of prefix[i])
//           (1) the affecting throttles, chunk by chunk through the 4 KiB LDS list (admit_affected_chunk).  A throttle that
//               keeps its stored status (reconcile error, not valid / responsible) is dropped: it passed — prefix > 0 says so —
//               and nothing of it depends on the victim set.  The rest form the LIST; an entry carries its throttle row and its
//               mutable state: counted pods, and per resource name the preemptor requests the `used` value and the exact
//               contributor count.  The initial state is S_k: the aggregate's totals minus every masked victim the throttle
//               matches.
//           (2) the walk, wave-uniform in j = k-1 .. 0 over the masked positions (64 mask bytes, rows and flags per load; the
//               set bits are visited through a ballot).  Lanes are list entries, a list longer than 64 takes several entries per
//               lane.  An entry whose throttle matches c_j (status[(n + j) * T + t] != 0) adds the candidate's amounts to its
//               state and re-judges its (throttle, amount) pairs with preempt_fails; entries the candidate does not match keep
//               passing (invariant: the current state passes).  A ballot decides: on a pass the matched entries commit and
//               lane 0 clears vic[j], on a fail nothing is written.
//   output  victims[i][j] = 1 iff c_j is still a victim at the end.  prefix[] is not written.
//
// Where the state lives: in kReprieveLdsBytes of LDS while the list fits (reprieve_lds_cap entries at 12 + 12 D bytes each),
// else in the preemptor's workgroup slot of an HBM workspace of the engine (T entries: the list cannot be longer) — the same
// code, instantiated for both address spaces as kt_admit does.  The launcher sizes the grid so that the workspace stays within
// kReprieveWsBudget bytes (one slot at the least).  The list is counted first and gathered second (the row is read twice, T bytes
// each time) so that the choice is made before anything is written.
//
// Deviation from a plain per-entry record: the state is laid out field by field ([cap] pods, [D][cap] values, [D][cap]
// contributor counts, [cap] throttle rows), so that the 64 lanes of a step touch consecutive words of LDS / HBM, and it is
// updated in place by a second pass over the matched entries after the ballot — a lane may own several entries, and holding
// their new values across the ballot would need a private array.  No lane indexes private memory dynamically: 0 bytes of scratch.
#include <type_traits>

#include "kt_admit_common.h"

namespace kt {

constexpr int kReprieveLdsBytes = 16 * 1024;         // the list's state in LDS: 20 KiB per wave with the chunk list, 8 waves per CU
constexpr size_t kReprieveWsBudget = 64ull << 20;    // the HBM workspace of one launch: grid x slot bytes stay below (one slot at least)

__host__ __device__ inline uint32_t reprieve_entry_bytes(int D) { return 12u + 12u * (uint32_t)D; }
static inline size_t reprieve_slot_bytes(int T, int D) { return ((size_t)T * reprieve_entry_bytes(D) + 15u) & ~(size_t)15u; }
uint32_t reprieve_lds_cap(int D, uint32_t limit) {
  const uint32_t cap = (uint32_t)kReprieveLdsBytes / reprieve_entry_bytes(D);
  return limit != 0 && limit < cap ? limit : cap;
}
static inline int reprieve_blocks(int T, int D, int64_t n, uint32_t lds_cap) {
  int64_t blocks = n < kPreemptMaxBlocks ? n : kPreemptMaxBlocks;
  if ((uint32_t)T > lds_cap) {  // a list may outgrow LDS: every workgroup owns a slot
    const int64_t fit = (int64_t)(kReprieveWsBudget / reprieve_slot_bytes(T, D));
    blocks = std::min(blocks, std::max<int64_t>(fit, 1));
  }
  return (int)std::max<int64_t>(blocks, 1);
}
size_t reprieve_ws_bytes(int T, int D, int64_t n, uint32_t lds_cap_limit) {
  const uint32_t lds_cap = reprieve_lds_cap(D, lds_cap_limit);
  if (n <= 0 || (uint32_t)T <= lds_cap) return 0;
  return (size_t)reprieve_blocks(T, D, n, lds_cap) * reprieve_slot_bytes(T, D);
}

struct ReprieveArgs {
  AdmitPage pg;                       // pod flags, request rows and the throttle tables of the engine (state offsets unused)
  const int64_t* rows;                // [n + m] pod table rows: the preemptors, then the candidates
  int64_t n, m;
  const uint8_t* status;              // [n + m][T]
  const unsigned long long* partial;  // [T][partial_stride(D)], exact contributor counts
  AmountTab calc;                     // the dry finalize's status.calculatedThreshold at `now`
  const uint8_t* calc_updated;        // [T]
  const uint8_t* error;               // [T]
  const int64_t* prefix;              // [n] as kt_preempt left it
  uint8_t* victims;                   // [n][m] in: the prefix mask, out: the reprieved set
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
__device__ __forceinline__ bool reprieve_stored(const ReprieveArgs& a, uint32_t t) {
  return a.error[t] != 0 || (a.pg.tt.flags[t] & (kThrValid | kThrResponsible)) != (kThrValid | kThrResponsible);
}

// the preemptor's affecting throttles that are reconciled: counted (ST = nullptr_t) or gathered into the state with the
// aggregate's totals; returns the wave-uniform list length
template <int DT, bool GATHER, class ST>
__device__ __forceinline__ uint32_t reprieve_list(const ReprieveArgs& a, const uint8_t* row, lds_u32wp list, ST* st, uint32_t lane) {
  const int T = a.T, D = a.pg.D;
  const int stride = partial_stride(D);
  uint32_t n_list = 0;
  for (int c0 = 0; c0 < T; c0 += kPreemptChunk) {
    bool err_c = false;  // (prefix > 0: the row holds no error byte)
    const uint32_t n_c = admit_affected_chunk(row, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
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

// one candidate against the list.  JUDGE: would some (throttle, amount) pair stop the preemptor with the candidate back
// (per lane: ballot it), nothing is written.  Otherwise the candidate's amounts are added (SIGN = 1) to or taken off
// (SIGN = -1) the state of every entry whose throttle matches it.
template <int DT, bool JUDGE, int SIGN, class ST>
__device__ __forceinline__ bool reprieve_step(const ReprieveArgs& a, ST& st, uint32_t n_list, const uint8_t* crow, uint32_t cfl,
                                              const int64_t (&vp)[DT], const int64_t (&cv)[DT], uint32_t lane) {
  const int D = a.pg.D;
  const bool eq = a.on_equal != 0;
  const ThrTables& tt = a.pg.tt;
  bool fail = false;
  for (uint32_t e = lane; e < n_list; e += kWave) {
    const uint32_t t = st.tl[e];
    if (crow[t] == 0) continue;
    const int64_t pods = st.pods[e] + SIGN;
    if constexpr (JUDGE) {
      const uint32_t tf = tt.flags[t];
      // the threshold the check reads behind the reconcile: calculatedThreshold once calculatedAt is set, else spec
      const AmountTab& th = ((tf & kThrCalcAtNonzero) || a.calc_updated[t]) ? a.calc : tt.spec;
      const bool eq3 = admit_eq3(tf, eq);
      const uint32_t th_p = th.present[t], c_p = a.calc.present[t], r_p = tt.reserved.present[t];
      const bool u_hc = pods > 0;
      fail |= preempt_fails(1, th.has_count[t] != 0, th.count[t], a.calc.has_count[t] != 0 && u_hc && pods >= a.calc.count[t], u_hc, pods,
                            tt.reserved.has_count[t] != 0, tt.reserved.count[t], eq3, eq);
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        if (d >= D || vp[d] == 0) continue;  // (wave-uniform)
        // a name that neither threshold names passes every step
        if (!(((th_p | c_p) >> d) & 1u)) continue;
        const bool has = ((cfl >> kPresentShift) >> d) & 1u;
        const int64_t u_v = st.uv[(size_t)d * st.cap + e] + (has ? cv[d] : 0);
        // presence is exact: the name is in `used` while a counted pod carries it
        const bool u_pr = st.uc[(size_t)d * st.cap + e] + (has ? 1u : 0u) > 0u;
        const bool c_pd = (c_p >> d) & 1u;
        fail |= preempt_fails(vp[d], (th_p >> d) & 1u, th.v[(size_t)t * D + d], c_pd && u_pr && u_v >= a.calc.v[(size_t)t * D + d], u_pr, u_v,
                              (r_p >> d) & 1u, tt.reserved.v[(size_t)t * D + d], eq3, eq);
      }
    } else {
      st.pods[e] = pods;
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        if (d >= D || vp[d] == 0) continue;  // (wave-uniform: only the names the preemptor requests are ever judged)
        if (!(((cfl >> kPresentShift) >> d) & 1u)) continue;
        st.uv[(size_t)d * st.cap + e] += SIGN * cv[d];
        st.uc[(size_t)d * st.cap + e] += (uint32_t)SIGN;
      }
    }
  }
  return fail;
}

template <int DT, bool IN_LDS>
__device__ __forceinline__ void reprieve_walk(const ReprieveArgs& a, ReprieveState<IN_LDS> st, lds_u32wp list, int64_t i, int64_t k,
                                              uint32_t lane) {
  const int T = a.T, D = a.pg.D, DS = a.pg.DS;
  const int64_t n = a.n;
  const int64_t p = a.rows[i];
  uint8_t* vic = a.victims + i * a.m;
  int64_t vp[DT], cv[DT];
#pragma unroll
  for (int d = 0; d < DT; ++d) vp[d] = d < D ? a.pg.req[p * DS + d] : 0, cv[d] = 0;
  const uint32_t n_list = reprieve_list<DT, true>(a, a.status + i * T, list, &st, lane);
  __syncthreads();  // an entry is owned by lane (entry mod 64) from here on; another lane wrote it
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
      if (d < D && vp[d] != 0 && (((cfl >> kPresentShift) >> d) & 1u)) cv[d] = a.pg.req[cb * DS + d];
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
      (void)reprieve_step<DT, false, -1>(a, st, n_list, a.status + (n + q0 + b) * (int64_t)T, cfl, vp, cv, lane);
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
      const bool fail = reprieve_step<DT, true, 1>(a, st, n_list, crow, cfl, vp, cv, lane);
      if (__ballot(fail) != 0ull) continue;  // c_j stays a victim
      (void)reprieve_step<DT, false, 1>(a, st, n_list, crow, cfl, vp, cv, lane);
      if (lane == 0) vic[q0 + b] = 0;
    }
  }
}

template <int DT>
__global__ __launch_bounds__(kWave) void kt_preempt_reprieve(const ReprieveArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  __shared__ __attribute__((aligned(16))) unsigned char state[kReprieveLdsBytes];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {  // (wave-uniform: one preemptor per wave and turn)
    const int64_t k = a.prefix[i];
    if (k <= 0) continue;
    const uint32_t n_list = reprieve_list<DT, false, void>(a, a.status + i * a.T, list, nullptr, lane);
    if (n_list <= a.lds_cap)
      reprieve_walk<DT, true>(a, ReprieveState<true>((KT_LDS unsigned char*)state, a.lds_cap, a.pg.D), list, i, k, lane);
    else if (a.ws)  // (the launcher gives a workspace whenever T > lds_cap; n_list <= T)
      reprieve_walk<DT, false>(a, ReprieveState<false>(a.ws + (size_t)blockIdx.x * a.ws_slot, (uint32_t)a.T, a.pg.D), list, i, k, lane);
    __syncthreads();  // the next preemptor rewrites the state
  }
}

void launch_preempt_reprieve(const AdmitPage& pg, int64_t n, int64_t m, const int64_t* rows_dev, int T, bool on_equal, const uint8_t* status,
                             const unsigned long long* partial, const AmountTab& calc, const uint8_t* calc_updated, const uint8_t* error,
                             const int64_t* prefix, uint8_t* victims, void* ws, uint32_t lds_cap_limit, hipStream_t s) {
  if (n <= 0 || m <= 0) return;
  ReprieveArgs a{};
  a.pg = pg, a.rows = rows_dev, a.n = n, a.m = m, a.status = status, a.partial = partial, a.calc = calc;
  a.calc_updated = calc_updated, a.error = error, a.prefix = prefix, a.victims = victims, a.T = T, a.on_equal = on_equal ? 1 : 0;
  a.lds_cap = reprieve_lds_cap(pg.D, lds_cap_limit);
  a.ws = (uint32_t)T > a.lds_cap ? (unsigned char*)ws : nullptr, a.ws_slot = reprieve_slot_bytes(T, pg.D);
  const int blocks = reprieve_blocks(T, pg.D, n, a.lds_cap);
  const int DT = dt_bucket(pg.D);
  if (DT == 4) hipLaunchKernelGGL(kt_preempt_reprieve<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_preempt_reprieve<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_preempt_reprieve<16>, dim3(blocks), dim3(kWave), 0, s, a);
}

}  // namespace kt
