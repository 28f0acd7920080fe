// kt_admit_common.h — what the admission kernels (kt_kernels_admit.hip: kt_admit, kt_admit_gangs) and the headroom kernel
// (kt_kernels_headroom.hip: kt_headroom) share, gfx950: the affected-throttle list of a status-matrix row, the page descriptor
// by value, the effective threshold and step 3's isThrottledOnEqual of a throttle, the 128-bit comparison; and what the preemption
// kernels (kt_kernels_preempt.hip: kt_preempt, kt_kernels_reprieve.hip: kt_preempt_reprieve) share: the four steps for one amount
// against `used` as it stands in some state, the wave scan, the chunk and grid sizes.  The page descriptor itself (AdmitPage) is
// host-visible: kt_launch.h.
#pragma once
#include "kt_index_device.h"

namespace kt {

// the sums of used + reserved (+ the pod) are formed in 128 bits: an all-reduced `used` may come close to int64's end
__device__ __forceinline__ bool admit_cmp(__int128 a, int64_t b, bool eq) { return eq ? a >= (__int128)b : a > (__int128)b; }

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

template <class V>
__device__ __forceinline__ V wave_inclusive_scan(V x, uint32_t lane) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const V y = __shfl_up(x, o);
    if (lane >= (uint32_t)o) x += y;
  }
  return x;
}

}  // namespace kt
