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
#include "kt_admit_common.h"

namespace kt {

// (the state's layout and sizes, ReprieveArgs, the list and the walk are kt_admit_common.h's: the gang form shares them)
uint32_t reprieve_lds_cap(int D, uint32_t limit) {
  const uint32_t cap = (uint32_t)kReprieveLdsBytes / reprieve_entry_bytes(D);
  return limit != 0 && limit < cap ? limit : cap;
}
size_t reprieve_ws_bytes(int T, int D, int64_t n, uint32_t lds_cap_limit) {
  const uint32_t lds_cap = reprieve_lds_cap(D, lds_cap_limit);
  if (n <= 0 || (uint32_t)T <= lds_cap) return 0;
  return (size_t)reprieve_blocks(T, D, n, lds_cap) * reprieve_slot_bytes(T, D);
}

// one candidate against the list, for ONE preemptor with requests vp.  JUDGE: would some (throttle, amount) pair stop the
// preemptor with the candidate back (per lane: ballot it), nothing is written.  Otherwise the candidate's amounts are added
// (SIGN = 1) to or taken off (SIGN = -1) the state of every entry whose throttle matches it.
template <int DT>
struct ReprievePod {
  const ReprieveArgs& a;
  int64_t vp[DT];
  template <bool JUDGE, int SIGN, class ST>
  __device__ __forceinline__ bool step(ST& st, uint32_t n_list, const uint8_t* crow, uint32_t cfl, const int64_t (&cv)[DT], uint32_t lane) const {
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
};

template <int DT, bool IN_LDS>
__device__ __forceinline__ void reprieve_walk(const ReprieveArgs& a, ReprieveState<IN_LDS> st, lds_u32wp list, int64_t i, int64_t k,
                                              uint32_t lane) {
  const int D = a.pg.D, DS = a.pg.DS;
  const int64_t p = a.rows[i];
  ReprievePod<DT> pod{a, {}};
  uint32_t track = 0;  // the names the preemptor requests
#pragma unroll
  for (int d = 0; d < DT; ++d) {
    pod.vp[d] = d < D ? a.pg.req[p * DS + d] : 0;
    track |= pod.vp[d] != 0 ? 1u << d : 0u;
  }
  const uint8_t* row = a.status + i * a.T;
  const auto chunk = [&](int c0, lds_u32wp l, bool* err) { return admit_affected_chunk(row, a.T, c0, l, (uint32_t)kPreemptChunk, 0u, err); };
  const uint32_t n_list = reprieve_list<DT, true>(a, chunk, list, &st, lane);
  __syncthreads();  // an entry is owned by lane (entry mod 64) from here on; another lane wrote it
  reprieve_walk_list<DT>(a, st, n_list, a.victims + i * a.m, k, track, pod, lane);
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
    const uint8_t* row = a.status + i * a.T;
    const auto chunk = [&](int c0, lds_u32wp l, bool* err) { return admit_affected_chunk(row, a.T, c0, l, (uint32_t)kPreemptChunk, 0u, err); };
    const uint32_t n_list = reprieve_list<DT, false, void>(a, chunk, list, nullptr, lane);
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
