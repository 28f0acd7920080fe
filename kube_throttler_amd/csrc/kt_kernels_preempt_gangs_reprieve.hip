// kt_kernels_preempt_gangs_reprieve.hip — the reprieve pass behind a gang's victim prefix (kt_preempt_gangs_reprieve_launch), gfx950.
//
// kt_preempt_gangs left, per gang g, the prefix length k and the mask M of the counted candidates below k that a throttle affecting
// some member matches.  The pass is kt_preempt_reprieve's (kt_kernels_reprieve.hip) with kt_preempt_gangs' judge in the place of
// the single pod's: start from "all of M removed" and put the victims back one by one, c_{k-1} first, keeping each back as long as
// an in-order admission of the gang — PreFilter, and on Success Reserve on every throttle that affects the member — still admits
// every member against a fresh reconcile at `now`.  The definition is the walk itself: nothing is assumed about the signs of
// requests.  The members' own reprieved sets do not compose into this answer: every admitted member reserves against the
// throttles the later members meet.
//
//   input   everything kt_preempt_gangs reads, prefix[] and victims[][] as it left them.
//   per gang (one wave, the grid strides; prefix <= 0 costs the one load of prefix[g])
//           (1) the UNION of the members' affecting throttles, chunk by chunk through the 4 KiB LDS list (gang_affected_chunk),
//               without those that keep their stored status: the LIST, counted first and gathered second (reprieve_list).  An
//               entry carries its throttle row, its counted pods and, per resource name SOME member requests with a non-zero
//               value (a wave-uniform mask), the `used` value and the exact contributor count.  Initial state: S_k.
//           (2) the walk (reprieve_walk_list), wave-uniform in j = k-1 .. 0 over the masked positions.  Lanes are list entries.  An
//               entry whose throttle matches c_j forms its tentative `used` — pods + 1, the values and contributor counts of the
//               names c_j carries — recomputes from it what the four steps read (status.throttled of the count and per name
//               against the calculated threshold, exact presence) and walks the members in order on its throttle under the
//               reserved prefix (gang_walk, with the lane's own throttle row: the member loop is uniform, a lane skips the
//               members its throttle does not affect, in the judge and in the reserved prefix).  Entries the candidate does not
//               match keep passing (invariant: the current state passes).  One ballot decides: on a pass the matched entries
//               commit in a second pass and lane 0 clears vic[j], on a fail nothing is written.
//   output  victims[g][j] = 1 iff c_j is still a victim at the end.  prefix[] and blocker[] are not written.
//
// Where the state lives, and how the grid is sized, is kt_preempt_reprieve's: kReprieveLdsBytes of LDS while the list fits, else
// the workgroup's slot of the engine's reprieve workspace.  No lane indexes private memory dynamically.
#include "kt_admit_common.h"

namespace kt {

struct GangReprieveArgs {
  const int64_t* gang_off;  // [n_gangs + 1] queue positions
  int64_t n_gangs;
};

// one candidate against the list, for the members [i0, i1) of one gang; `track`: the names some member requests
template <int DT>
struct ReprieveGang {
  const ReprieveArgs& a;
  int64_t i0, i1;
  uint32_t track;
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
        const AmountTab& th = preempt_threshold(tt, a.calc, tf, a.calc_updated[t]);
        GangThr<DT> g;
        g.eq = eq, g.eq3 = admit_eq3(tf, eq);
        g.th_hc = th.has_count[t] != 0, g.r_hc = tt.reserved.has_count[t] != 0;
        g.th_c = th.count[t], g.r_c = tt.reserved.count[t];
        g.th_p = th.present[t], g.r_p = tt.reserved.present[t];
        const uint32_t c_p = a.calc.present[t];
        // the tentative `used` with the candidate back, and the flags of a fresh reconcile of it
        GangUsed<DT> u;
        u.u_c = pods, u.u_hc = pods > 0, u.c_flag = a.calc.has_count[t] != 0 && u.u_hc && pods >= a.calc.count[t];
        u.flag_m = u.pr_m = 0u;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          g.tv[d] = g.rv[d] = u.u_v[d] = 0;
          if (d >= D) continue;
          g.rv[d] = tt.reserved.v[(size_t)t * D + d];  // (every name: Reserve adds to it whoever reads it)
          // a name no member requests, or that neither threshold names, passes every step of every member
          if (!(((track & (g.th_p | c_p)) >> d) & 1u)) continue;
          g.tv[d] = th.v[(size_t)t * D + d];
          const bool has = ((cfl >> kPresentShift) >> d) & 1u;
          u.u_v[d] = st.uv[(size_t)d * st.cap + e] + (has ? cv[d] : 0);
          // presence is exact: the name is in `used` while a counted pod carries it
          const bool u_pr = st.uc[(size_t)d * st.cap + e] + (has ? 1u : 0u) > 0u;
          u.pr_m |= u_pr ? 1u << d : 0u;
          u.flag_m |= (((c_p >> d) & 1u) && u_pr && u.u_v[d] >= a.calc.v[(size_t)t * D + d]) ? 1u << d : 0u;
        }
        // (a name the thresholds do not name: th_p's bit and flag_m's are clear, preempt_fails passes it whatever tv and u_v hold)
        fail |= gang_walk<DT>(a, t, i0, i1, g, u) < i1;
      } else {
        st.pods[e] = pods;
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          if (d >= D || !((track >> d) & 1u)) continue;  // (wave-uniform: only the names some member requests are ever judged)
          if (!(((cfl >> kPresentShift) >> d) & 1u)) continue;
          st.uv[(size_t)d * st.cap + e] += SIGN * cv[d];
          st.uc[(size_t)d * st.cap + e] += (uint32_t)SIGN;
        }
      }
    }
    return fail;
  }
};

// the names some member of the gang requests with a non-zero value (wave-uniform)
template <int DT>
__device__ __forceinline__ uint32_t gang_tracked_names(const ReprieveArgs& a, int64_t i0, int64_t i1, uint32_t lane) {
  const int D = a.pg.D, DS = a.pg.DS;
  uint32_t mine = 0;
  for (int64_t j = i0 + lane; j < i1; j += kWave) {
    const int64_t p = a.rows[j];
#pragma unroll
    for (int d = 0; d < DT; ++d)
      if (d < D && a.pg.req[p * DS + d] != 0) mine |= 1u << d;
  }
  uint32_t track = 0;
#pragma unroll
  for (int d = 0; d < DT; ++d)
    if (__ballot((mine >> d) & 1u) != 0ull) track |= 1u << d;
  return track;
}

template <int DT, bool IN_LDS, class CHUNK>
__device__ __forceinline__ void gang_reprieve_walk(const ReprieveArgs& a, ReprieveState<IN_LDS> st, const CHUNK& chunk, lds_u32wp list, int64_t gi,
                                                   int64_t i0, int64_t i1, int64_t k, uint32_t lane) {
  const ReprieveGang<DT> gang{a, i0, i1, gang_tracked_names<DT>(a, i0, i1, lane)};
  const uint32_t n_list = reprieve_list<DT, true>(a, chunk, list, &st, lane);
  __syncthreads();  // an entry is owned by lane (entry mod 64) from here on; another lane wrote it
  reprieve_walk_list<DT>(a, st, n_list, a.victims + gi * a.m, k, gang.track, gang, lane);
}

template <int DT>
__global__ __launch_bounds__(kWave) void kt_preempt_gangs_reprieve(const ReprieveArgs a, const GangReprieveArgs ga) {
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
    const uint32_t n_list = reprieve_list<DT, false, void>(a, chunk, list, nullptr, lane);
    if (n_list <= a.lds_cap)
      gang_reprieve_walk<DT, true>(a, ReprieveState<true>((KT_LDS unsigned char*)state, a.lds_cap, a.pg.D), chunk, list, gi, i0, i1, k, lane);
    else if (a.ws)  // (the launcher gives a workspace whenever T > lds_cap; n_list <= T)
      gang_reprieve_walk<DT, false>(a, ReprieveState<false>(a.ws + (size_t)blockIdx.x * a.ws_slot, (uint32_t)a.T, a.pg.D), chunk, list, gi, i0, i1, k,
                                    lane);
    __syncthreads();  // the next gang rewrites the state
  }
}

void launch_preempt_gangs_reprieve(const AdmitPage& pg, int64_t n, int64_t m, const int64_t* rows_dev, int64_t n_gangs, const int64_t* gang_off_dev,
                                   int T, bool on_equal, const uint8_t* status, const unsigned long long* partial, const AmountTab& calc,
                                   const uint8_t* calc_updated, const uint8_t* error, const int64_t* prefix, uint8_t* victims, void* ws,
                                   uint32_t lds_cap_limit, hipStream_t s) {
  if (n_gangs <= 0 || m <= 0) return;
  ReprieveArgs a{};
  a.pg = pg, a.rows = rows_dev, a.n = n, a.m = m, a.status = status, a.partial = partial, a.calc = calc;
  a.calc_updated = calc_updated, a.error = error, a.prefix = prefix, a.victims = victims, a.T = T, a.on_equal = on_equal ? 1 : 0;
  a.lds_cap = reprieve_lds_cap(pg.D, lds_cap_limit);
  a.ws = (uint32_t)T > a.lds_cap ? (unsigned char*)ws : nullptr, a.ws_slot = reprieve_slot_bytes(T, pg.D);
  const GangReprieveArgs ga{gang_off_dev, n_gangs};
  const int blocks = reprieve_blocks(T, pg.D, n_gangs, a.lds_cap);
  const int DT = dt_bucket(pg.D);
  if (DT == 4) hipLaunchKernelGGL(kt_preempt_gangs_reprieve<4>, dim3(blocks), dim3(kWave), 0, s, a, ga);
  else if (DT == 8) hipLaunchKernelGGL(kt_preempt_gangs_reprieve<8>, dim3(blocks), dim3(kWave), 0, s, a, ga);
  else hipLaunchKernelGGL(kt_preempt_gangs_reprieve<16>, dim3(blocks), dim3(kWave), 0, s, a, ga);
}

}  // namespace kt
