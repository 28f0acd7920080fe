// kt_kernels_headroom_forecast.hip — how many copies of a pod the throttles admit at each of a list of instants
// (kt_headroom_forecast_launch), gfx950.
//
// kt_forecast (kt_kernels_forecast.hip) with kt_headroom's closed form (headroom_of_term, kt_admit_common.h) in the place of the
// verdict.  For pod p and the caller's ascending instants t_0 .. t_{m-1}, state R_k is the cluster as the engine holds it, every
// valid and responsible throttle reconciled at t_k; copies[p][k] is headroom(p, cap) with R_k as the stored status: the leading
// Success verdicts of a dry kt_admit over [p] * cap.  `used` does not depend on k, the threshold does not depend on the pod, every
// affecting throttle reserves every admitted copy and inside a throttle the pod count and every requested name are independent:
// the answer at k is the minimum over (affecting throttle, amount) of a closed form, and every k is judged in parallel, lane =
// instant position.
//
//   input   that of kt_forecast (status matrix and summary words of ONE check, the partial rows of an aggregate with exact
//           contributor counts, the error bytes of a dry finalize, the stored tables, the instants), plus cap and want.  Read-only.
//   per pod (one wave, the grid strides) the affecting throttles chunk by chunk through a 4 KiB LDS list; per throttle the
//           instants 64 at a time: the lane computes the calculated threshold at its instant, `replace`, the threshold the check
//           reads and `throttled` from the fresh sums exactly as kt_forecast does, fills a HeadroomTerm for the pod count and for
//           every needed name and reduces headroom_of_term into h at once.  A throttle that keeps its stored status (reconcile
//           error, not valid or not responsible) is judged once, wave-uniform, from the stored tables as kt_headroom reads them:
//           its h holds at every instant.
//   running answer: the lexicographic minimum of (h, throttle row), packed as kt_headroom packs it.  The chunk list is NOT in
//           row order (admit_append_marked fills it round by round), so the row is a key of the comparison.  With more than 64
//           instants a lane owns several positions: the running pair of each lives in the lane's own cell of the copies buffer
//           (one 64-bit word per position, as kt_forecast keeps ver[q]), written only where a throttle lowers it.
//   output  copies[i][k] = min(cap, h); limiting[i][k] = the row where h < cap, else -1; first[i] = the first position with
//           copies >= want (ballot over the blocks in order), or -1.  An error row or an invalid pod row: 0, -1 and -1.
#include "kt_admit_common.h"

namespace kt {

struct HeadroomForecastArgs {
  AdmitPage pg;                       // pod flags, request rows and the throttle tables of the engine (state offsets unused)
  const int64_t* rows;                // [n] pod table rows
  int64_t n, m;                       // pods, instants
  const int64_t* inst_s;              // [m] strictly ascending
  const int32_t* inst_ns;             // [m]
  const uint8_t* status;              // [n][T]
  const uint64_t* summary;            // [n]
  const unsigned long long* partial;  // [T][partial_stride(D)], exact contributor counts
  const uint8_t* error;               // [T] the reconcile is an error: the stored status stays
  int64_t* first;                     // [n] out
  int64_t* copies;                    // [n][m] out (and the running (h, row) pair of every position while the kernel runs)
  int32_t* limiting;                  // [n][m] out
  int32_t T, on_equal;
  uint32_t cap, want;                 // 1 <= want <= cap <= 2^31 - 1
};

__device__ __forceinline__ uint32_t hf_min(uint32_t a, uint32_t b) { return b < a ? b : a; }
__device__ __forceinline__ unsigned long long hf_min(unsigned long long a, unsigned long long b) { return b < a ? b : a; }

template <int DT>
__global__ __launch_bounds__(kWave) void kt_headroom_forecast(const HeadroomForecastArgs a) {
  __shared__ uint32_t chunk_list[kPreemptChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  const uint32_t lane = threadIdx.x;
  const int T = a.T, D = a.pg.D, DS = a.pg.DS;
  const bool eq = a.on_equal != 0;
  const uint32_t cap = a.cap, want = a.want;
  const ThrTables& tt = a.pg.tt;
  const int stride = partial_stride(D);
  const int64_t n = a.n, m = a.m;
  const unsigned long long none = (unsigned long long)cap << 32 | 0xFFFFFFFFull;  // (cap, no row)
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {  // (wave-uniform: one pod per wave and turn)
    const int64_t p = a.rows[i];
    unsigned long long* run = (unsigned long long*)(a.copies + i * m);  // the lane's own cells: positions lane, lane + 64, ...
    int32_t* lim = a.limiting + i * m;
    for (int64_t q = lane; q < m; q += kWave) run[q] = none;
    const uint8_t* row = a.status + i * T;
    const uint32_t pfl = a.pg.pod_flags[p];
    const uint32_t brings = pfl >> kPresentShift;
    bool err = a.summary[i] == 2ull || !(pfl & kPodValid);
    unsigned long long kept = none;  // the minimum over the throttles that keep their stored status: it holds at every instant
    for (int c0 = 0; c0 < T && !err; c0 += kPreemptChunk) {
      bool err_c = false;
      const uint32_t n_c = admit_affected_chunk(row, T, c0, list, (uint32_t)kPreemptChunk, 0u, &err_c);
      err = __ballot(err_c) != 0ull;
      __syncthreads();  // (one wave: the list's entries are read by other lanes than wrote them)
      for (uint32_t ai = 0; ai < n_c && !err; ++ai) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)list[ai]);
        const uint32_t tf = tt.flags[t];
        const bool stored = a.error[t] != 0 || (tf & (kThrValid | kThrResponsible)) != (kThrValid | kThrResponsible);
        const bool eq3 = admit_eq3(tf, eq);
        const bool r_hc = tt.reserved.has_count[t] != 0;
        const int64_t r_c = r_hc ? tt.reserved.count[t] : 0;  // a reserved amount whose presence bit is clear reads as 0
        const uint32_t r_p = tt.reserved.present[t];
        HeadroomTerm hm;
        hm.eq3 = eq3, hm.eq = eq;
        if (stored) {  // nothing of it depends on the instant: the stored tables as headroom_count / headroom_name read them
          const AmountTab& th = admit_threshold(tt, tf);
          const uint32_t th_p = th.present[t], u_p = tt.used.present[t], flg = tt.thrl_flag[t] & tt.thrl_has[t];
          const bool u_hc = tt.used.has_count[t] != 0;
          hm.v = 1, hm.va = 1, hm.tv = th.count[t], hm.uv = u_hc ? tt.used.count[t] : 0, hm.rv = r_c;
          hm.th_has = th.has_count[t] != 0, hm.present0 = u_hc || r_hc, hm.brings = true, hm.flagged = (tf & kThrThrottledPod) != 0;
          uint32_t h = headroom_of_term(hm, cap);
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            if (d >= D) continue;
            const int64_t vpd = a.pg.req[p * DS + d];
            if (vpd == 0) continue;  // steps 1-4 of a name the pod does not request
            hm.brings = (brings >> d) & 1u;
            hm.v = vpd, hm.va = hm.brings ? vpd : 0;
            hm.th_has = (th_p >> d) & 1u;
            hm.tv = th.v[(size_t)t * D + d];
            hm.uv = ((u_p >> d) & 1u) ? tt.used.v[(size_t)t * D + d] : 0;
            hm.rv = ((r_p >> d) & 1u) ? tt.reserved.v[(size_t)t * D + d] : 0;
            hm.present0 = ((u_p | r_p) >> d) & 1u;
            hm.flagged = (flg >> d) & 1u;
            h = hf_min(h, headroom_of_term(hm, h));
          }
          kept = hf_min(kept, (unsigned long long)h << 32 | t);
          continue;
        }
        // ---- the throttle's own state: one batch of wave-uniform loads
        const uint32_t ovr0 = tt.ovr_off[t], ovr1 = tt.ovr_off[t + 1];
        const uint64_t status_fp = tt.status_msgs_fp[t], spec_fp = tt.spec_msgs_fp[t];
        const bool s_hc = tt.spec.has_count[t] != 0, k_hc = tt.calc.has_count[t] != 0;
        const int64_t s_c = tt.spec.count[t], k_c = tt.calc.count[t];
        const uint32_t s_p = tt.spec.present[t], k_p = tt.calc.present[t];
        const unsigned long long* prow = a.partial + (size_t)t * stride;
        const int64_t pods_total = (int64_t)prow[partial_off_pods(D)];
        const bool u_hc = pods_total > 0;
        // the names some threshold of this throttle can name, and whether an override has a parse error (the messages of
        // CalculateThreshold: they do not depend on the instant)
        uint32_t names = s_p | k_p;
        bool any_err = false;
        for (uint32_t o = ovr0; o < ovr1; ++o) {
          if (tt.ovr_flags[o] & kOvrParseError) any_err = true;
          else names |= tt.ovr_thr.present[o];
        }
        const bool fp_differs = status_fp != (any_err ? spec_fp : 0ull);
        int64_t vp[DT], sv[DT], kv[DT], rv[DT], tot_v[DT];
        bool need[DT], u_pr[DT];
        bool spec_diff = false;  // spec.threshold against the stored calculatedThreshold, by value, over the names spec has
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          need[d] = u_pr[d] = false, vp[d] = sv[d] = kv[d] = rv[d] = tot_v[d] = 0;
          if (d >= D) continue;
          sv[d] = tt.spec.v[(size_t)t * D + d], kv[d] = tt.calc.v[(size_t)t * D + d];
          spec_diff |= ((s_p >> d) & 1u) && sv[d] != kv[d];
          vp[d] = a.pg.req[p * DS + d];
          // a name the pod does not request passes every step, and so does one that no threshold names
          need[d] = vp[d] != 0 && ((names >> d) & 1u);
          if (!need[d]) continue;
          rv[d] = ((r_p >> d) & 1u) ? tt.reserved.v[(size_t)t * D + d] : 0;
          // a key is present when some counted pod carried it (as kt_finalize: the contributor count, or a non-zero sum)
          const int64_t tot = (int64_t)prow[d];
          u_pr[d] = prow[partial_off_presence(D) + d] != 0ull || tot != 0;
          tot_v[d] = u_pr[d] ? tot : 0;
        }
        for (int64_t q0 = 0; q0 < m; q0 += kWave) {
          const int64_t q = q0 + lane;
          const bool in = q < m;
          const int64_t ts = a.inst_s[in ? q : m - 1];
          const int32_t tn = a.inst_ns[in ? q : m - 1];
          // ---- CalculateThreshold(t): first active override wins, per name and for the count
          bool active_found = false, c_hc = false, diff = false;
          int64_t c_c = 0, c_v[DT];
          uint32_t c_p = 0;
#pragma unroll
          for (int d = 0; d < DT; ++d) c_v[d] = 0;
          for (uint32_t o = ovr0; o < ovr1; ++o) {
            // one batch of loads per override (wave-uniform)
            const uint8_t of = tt.ovr_flags[o];
            const int64_t ob_s = tt.ovr_begin_s[o], oe_s = tt.ovr_end_s[o];
            const int32_t ob_ns = tt.ovr_begin_ns[o], oe_ns = tt.ovr_end_ns[o];
            const bool o_hc = tt.ovr_thr.has_count[o] != 0;
            const int64_t o_c = tt.ovr_thr.count[o];
            const uint32_t op = tt.ovr_thr.present[o];
            if (of & kOvrParseError) continue;
            const bool end_zero = oe_s == kZeroTimeS && oe_ns == 0;
            const bool active = forecast_le(ob_s, ob_ns, ts, tn) && (end_zero || forecast_le(ts, tn, oe_s, oe_ns));
            if (__ballot(active) == 0ull) continue;
            active_found |= active;
            if (active && !c_hc && o_hc) c_hc = true, c_c = o_c;
            const uint32_t take = active ? op & ~c_p : 0u;  // the names this override decides at this lane's instant
            c_p |= take;
#pragma unroll
            for (int d = 0; d < DT; ++d) {
              if (d >= D || !((op >> d) & 1u)) continue;  // (wave-uniform)
              const int64_t o_v = tt.ovr_thr.v[(size_t)o * D + d];
              if ((take >> d) & 1u) {
                diff |= o_v != kv[d];
                c_v[d] = o_v;
              }
            }
          }
          if (!active_found) {  // no active override: spec.threshold; otherwise the merged override REPLACES it
            c_p = s_p, c_hc = s_hc, c_c = s_c, diff = spec_diff;
#pragma unroll
            for (int d = 0; d < DT; ++d) c_v[d] = sv[d];
          }
          // ---- replace the stored calculatedThreshold only if threshold or messages differ by value (where they do not, the
          //      stored one equals the computed one by value: the lane goes on with its own)
          const bool same = (c_hc == k_hc) && (!c_hc || c_c == k_c) && c_p == k_p && !diff;
          const bool replace = !same || fp_differs;
          // ---- the threshold the check reads behind this reconcile: calculatedThreshold once calculatedAt is set, else spec
          const bool reads_calc = (tf & kThrCalcAtNonzero) || replace;
          const uint32_t th_p = reads_calc ? c_p : s_p;
          // ---- throttled = calculatedThreshold.IsThrottled(used, true), then the closed form of the four steps: the pod count ...
          hm.v = 1, hm.va = 1, hm.tv = reads_calc ? c_c : s_c, hm.uv = u_hc ? pods_total : 0, hm.rv = r_c;
          hm.th_has = reads_calc ? c_hc : s_hc, hm.present0 = u_hc || r_hc, hm.brings = true;
          hm.flagged = c_hc && u_hc && pods_total >= c_c;
          uint32_t h = headroom_of_term(hm, cap);
          // ... and every needed name, reduced into the minimum at once: the minimum so far is the term's cap (min(h, term) is the
          // same number, and headroom_fit bisects below h only)
#pragma unroll
          for (int d = 0; d < DT; ++d) {
            if (!need[d]) continue;  // (wave-uniform)
            hm.brings = (brings >> d) & 1u;
            hm.v = vp[d], hm.va = hm.brings ? vp[d] : 0;
            hm.th_has = (th_p >> d) & 1u;
            hm.tv = reads_calc ? c_v[d] : sv[d];
            hm.uv = tot_v[d], hm.rv = rv[d];
            hm.present0 = u_pr[d] || ((r_p >> d) & 1u);
            hm.flagged = ((c_p >> d) & 1u) && u_pr[d] && tot_v[d] >= c_v[d];
            h = hf_min(h, headroom_of_term(hm, h));
          }
          // (cap, any row) lowers no answer: only a throttle that stops a copy below cap touches the lane's cell
          if (in && h < cap) run[q] = hf_min(run[q], (unsigned long long)h << 32 | t);
        }
      }
      __syncthreads();  // the next chunk rewrites the list
    }
    int64_t ans = -1;
    for (int64_t q0 = 0; q0 < m; q0 += kWave) {
      const int64_t q = q0 + lane;
      const bool in = q < m;
      const unsigned long long best = in ? hf_min(run[q], kept) : none;
      const uint32_t h = err ? 0u : (uint32_t)(best >> 32);
      if (in) {
        a.copies[i * m + q] = (int64_t)h;
        lim[q] = (err || h >= cap) ? -1 : (int32_t)(uint32_t)best;
      }
      const uint64_t mk = __ballot(in && !err && h >= want);
      if (mk != 0ull && ans < 0) ans = q0 + (__ffsll((long long)mk) - 1);  // the first position with `want` copies
    }
    if (lane == 0) a.first[i] = ans;
  }
}

void launch_headroom_forecast(const AdmitPage& pg, int64_t n, int64_t m, const int64_t* rows_dev, const int64_t* inst_s, const int32_t* inst_ns,
                              int T, bool on_equal, uint32_t cap, uint32_t want, const uint8_t* status, const uint64_t* summary,
                              const unsigned long long* partial, const uint8_t* error, int64_t* first, int64_t* copies, int32_t* limiting,
                              hipStream_t s) {
  if (n <= 0 || m <= 0) return;
  HeadroomForecastArgs a{};
  a.pg = pg, a.rows = rows_dev, a.n = n, a.m = m, a.inst_s = inst_s, a.inst_ns = inst_ns, a.status = status, a.summary = summary;
  a.partial = partial, a.error = error, a.first = first, a.copies = copies, a.limiting = limiting, a.T = T, a.on_equal = on_equal ? 1 : 0;
  a.cap = cap, a.want = want;
  const int blocks = (int)(n < kPreemptMaxBlocks ? n : kPreemptMaxBlocks);
  const int DT = dt_bucket(pg.D);
  if (DT == 4) hipLaunchKernelGGL(kt_headroom_forecast<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_headroom_forecast<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_headroom_forecast<16>, dim3(blocks), dim3(kWave), 0, s, a);
}

}  // namespace kt
