// kt_kernels_headroom.hip — how many copies of a pod the throttles still admit (kt_headroom_launch), gfx950.
//
// headroom(pod, cap) is the number of leading Success verdicts kt_admit (kt_kernels_admit.hip) returns for the queue
// [pod] * cap as a dry run: PreFilter (plugin.go:148-215) and, on Success, Reserve (plugin.go:217-239 ->
// reservedResourceAmounts.addPod, reserved_resource_amounts.go:66-77), copy after copy, until the first copy that is not
// admitted.  Every affecting throttle reserves every admitted copy, so the answer is the minimum over the affecting
// throttles t of h_t, the copies t alone lets through, and inside a throttle the pod count and every requested resource name
// are independent: h_t is the minimum over them of a closed form (headroom_of_term, kt_admit_common.h).  Nothing is walked in sequence and
// nothing is mutable, so — unlike kt_admit, which is ONE wave — the pods are independent: one wave per pod, the grid strides.
//
//   input   status matrix [n][T] and summary words [n] of a preceding kt_check launch over the same rows (which throttles
//           affect which pod; error rows = 255 / summary 2), the page descriptors of kt_admit (AdmitPage: thresholds, used,
//           status.throttled, reserved tables, pod requests), all read-only
//   per pod lane = (affected throttle, dimension) in the DT bucket of the widest page: h of the lane's resource name over
//           every page (the name part is the minimum over the pages), h of the pod count once, on page 0;
//           min over the DT lanes of a throttle, then the lexicographic (h, throttle row) minimum over the pod's throttles
//   output  copies[i] = min(cap, min_t h_t); limiting[i] = the lowest throttle row with h_t == copies[i] when copies[i] < cap —
//           the lowest row whose status is not `not-throttled` in the row PreFilter returns for the first copy that is not
//           admitted (a throttle with h_t > copies[i] still passes that copy) — else -1.  An error row (selector / namespace
//           error, plugin.go:154-168) or an invalid pod row: 0 and -1.  A pod no throttle affects: cap and -1.
//
// The affected throttles are consumed CHUNK BY CHUNK (kWave x 16 bytes of the matrix row at a time, admit_affected_chunk)
// through a list of one chunk's entries in LDS, not collected for the whole row as kt_admit does: no second pass (Reserve,
// rollback) needs the list here, and a fixed 4 KiB of LDS per wave keeps the occupancy and puts no limit on the throttle rows.
#include "kt_admit_common.h"

namespace kt {

struct HeadroomArgs {
  const AdmitPage* pages;  // [n_pages] in device memory (the descriptors kt_admit reads)
  int32_t n_pages;
  const int64_t* rows;  // nullable: position -> pod table row (the same rows in every page)
  int64_t n;
  const uint8_t* status;    // [n][T] page 0's matrix
  const uint64_t* summary;  // [n] page 0's summary words (2: PreFilter is an error)
  int64_t* copies;          // [n] out
  int32_t* limiting;        // [n] out
  int32_t T, on_equal;
  uint32_t cap;  // 1 .. 2^31 - 1
};

// A reserved amount whose presence bit (has_count) is clear reads as 0 below, whatever the table holds: that is the state kt_admit
// starts from (admit_load_state stores 0 for such an entry, and admit_count_bits / admit_name_bits then read the state unmasked).
// resourceCounts.pod of throttle t (the same in every page: evaluated on page 0)
__device__ __forceinline__ uint32_t headroom_count(const ThrTables& tt, uint32_t t, bool eq, uint32_t cap) {
  const uint32_t tf = tt.flags[t];
  const AmountTab& th = admit_threshold(tt, tf);
  const bool u_hc = tt.used.has_count[t] != 0, r_hc = tt.reserved.has_count[t] != 0;
  HeadroomTerm m;
  m.v = 1, m.va = 1, m.tv = th.count[t];
  m.uv = u_hc ? tt.used.count[t] : 0, m.rv = r_hc ? tt.reserved.count[t] : 0;
  m.th_has = th.has_count[t] != 0, m.present0 = u_hc || r_hc, m.brings = true;
  m.flagged = (tf & kThrThrottledPod) != 0;
  m.eq3 = admit_eq3(tf, eq), m.eq = eq;
  return headroom_of_term(m, cap);
}

// dimension d of one page's names for pod row p on throttle t
__device__ __forceinline__ uint32_t headroom_name(const AdmitPage& pg, int64_t p, uint32_t t, uint32_t d, bool eq, uint32_t cap) {
  const ThrTables& tt = pg.tt;
  const int D = pg.D;
  if ((int)d >= D) return cap;
  const int64_t v = pg.req[p * pg.DS + d];
  if (v == 0) return cap;  // steps 1-4 of a name the pod does not request
  const uint32_t tf = tt.flags[t];
  const AmountTab& th = admit_threshold(tt, tf);
  const uint32_t u_p = tt.used.present[t], r_p = tt.reserved.present[t];
  HeadroomTerm m;
  m.brings = ((pg.pod_flags[p] >> kPresentShift) >> d) & 1u;
  m.v = v, m.va = m.brings ? v : 0;
  m.th_has = (th.present[t] >> d) & 1u;
  m.tv = m.th_has ? th.v[(size_t)t * D + d] : 0;
  m.uv = ((u_p >> d) & 1u) ? tt.used.v[(size_t)t * D + d] : 0;
  m.rv = ((r_p >> d) & 1u) ? tt.reserved.v[(size_t)t * D + d] : 0;
  m.present0 = ((u_p | r_p) >> d) & 1u;
  m.flagged = ((tt.thrl_flag[t] & tt.thrl_has[t]) >> d) & 1u;
  m.eq3 = admit_eq3(tf, eq), m.eq = eq;
  return headroom_of_term(m, cap);
}

constexpr int kHeadroomChunk = kWave * 16;  // matrix bytes per chunk = entries the chunk list holds
constexpr int kHeadroomMaxBlocks = 2048;    // 256 CUs x 8 one-wave workgroups; more pods than that: the grid strides

template <class U>
__device__ __forceinline__ U umin(U a, U b) { return b < a ? b : a; }

template <int DT>
__global__ __launch_bounds__(kWave) void kt_headroom(const HeadroomArgs a) {
  __shared__ uint32_t chunk_list[kHeadroomChunk];
  lds_u32wp list = (lds_u32wp)chunk_list;
  constexpr int MPW = kWave / DT;
  const uint32_t lane = threadIdx.x, d = lane % DT, ml = lane / DT;
  const int T = a.T, n_pages = a.n_pages;
  const bool eq = a.on_equal != 0;
  const uint32_t cap = a.cap;
  for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {  // (wave-uniform: one pod per wave and turn)
    const int64_t p = a.rows ? a.rows[i] : i;
    const uint8_t* row = a.status + i * T;
    bool err = a.summary[i] == 2ull || !(admit_page(a.pages, 0).pod_flags[p] & kPodValid);
    unsigned long long best = (unsigned long long)cap << 32 | 0xFFFFFFFFull;  // (h, throttle row), lexicographic minimum
    for (int c0 = 0; c0 < T && !err; c0 += kHeadroomChunk) {
      bool err_c = false;
      const uint32_t n_c = admit_affected_chunk(row, T, c0, list, (uint32_t)kHeadroomChunk, 0u, &err_c);
      err = __ballot(err_c) != 0ull;
      for (uint32_t base = 0; base < n_c && !err; base += MPW) {
        const uint32_t j = base + ml;
        const bool vv = j < n_c;
        const uint32_t t = list[vv ? j : 0u];
        uint32_t h = cap;
        for (int k = 0; k < n_pages; ++k) {
          const AdmitPage pg = admit_page(a.pages, k);
          if (!vv) continue;
          if (k == 0 && d == 0) h = umin(h, headroom_count(pg.tt, t, eq, cap));
          h = umin(h, headroom_name(pg, p, t, d, eq, cap));
        }
#pragma unroll
        for (int o = DT / 2; o >= 1; o >>= 1) h = umin(h, (uint32_t)__shfl_xor((int)h, o));
        if (vv && d == 0) best = umin(best, (unsigned long long)h << 32 | t);
      }
    }
#pragma unroll
    for (int o = kWave / 2; o >= 1; o >>= 1) best = umin(best, __shfl_xor(best, o));
    if (lane == 0) {
      const uint32_t h = (uint32_t)(best >> 32);
      a.copies[i] = err ? 0 : (int64_t)h;
      a.limiting[i] = (err || h >= cap) ? -1 : (int32_t)(uint32_t)best;
    }
  }
}

// pages: the descriptors as launch_admit lays them out (the state offsets are not used); copied to pages_dev, pages_copied
// recorded behind the copy, as there.  false: *hip_err says why
bool launch_headroom(const AdmitPage* pages, int n_pages, AdmitPage* pages_dev, hipEvent_t pages_copied, int64_t n, const int64_t* rows_dev, int T,
                     bool on_equal, uint32_t cap, const uint8_t* status, const uint64_t* summary, int64_t* copies, int32_t* limiting,
                     hipStream_t s, hipError_t* hip_err) {
  *hip_err = hipSuccess;
  int maxD = 1;
  for (int k = 0; k < n_pages; ++k) maxD = pages[k].D > maxD ? pages[k].D : maxD;
  HeadroomArgs a{};
  a.pages = pages_dev, a.n_pages = n_pages, a.rows = rows_dev, a.n = n, a.status = status, a.summary = summary;
  a.copies = copies, a.limiting = limiting, a.T = T, a.on_equal = on_equal ? 1 : 0, a.cap = cap;
  if ((*hip_err = hipMemcpyAsync(pages_dev, pages, sizeof(AdmitPage) * (size_t)n_pages, hipMemcpyHostToDevice, s)) != hipSuccess) return false;
  if ((*hip_err = hipEventRecord(pages_copied, s)) != hipSuccess) return false;
  const int blocks = (int)(n < kHeadroomMaxBlocks ? n : kHeadroomMaxBlocks);
  const int DT = dt_bucket(maxD);
  if (DT == 4) hipLaunchKernelGGL(kt_headroom<4>, dim3(blocks), dim3(kWave), 0, s, a);
  else if (DT == 8) hipLaunchKernelGGL(kt_headroom<8>, dim3(blocks), dim3(kWave), 0, s, a);
  else hipLaunchKernelGGL(kt_headroom<16>, dim3(blocks), dim3(kWave), 0, s, a);
  return true;
}

}  // namespace kt
