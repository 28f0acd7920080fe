// kt_launch.h — host-callable launchers of the HIP kernels (implemented in kt_kernels*.hip).
#pragma once
#include "kt_device.h"

namespace kt {

// Staged pod batch in device memory (row-major, as in kt_snapshot).
struct PodBatchDev {
  int64_t n;
  const int64_t* rows;  // nullable => row0 + i
  int64_t row0;
  const uint32_t* ns;
  const uint32_t* flags;
  const uint32_t* label_off;  // [n+1], relative to label_base
  const uint32_t* label_key;
  const uint32_t* label_pair;
  uint32_t label_base;        // value of label_off[0] in the host batch (arrays are copied from there)
  const uint32_t* ctr_off;    // [n+1]
  const uint8_t* ctr_init;
  const uint32_t* ctr_present;
  const int64_t* ctr_req;     // [n_ctr][D]
  uint32_t ctr_base;
  const uint32_t* ovh_present;
  const int64_t* ovh;         // [n][D]
};

struct IndexTables;  // kt_index.h

void launch_ingest_pods(const PodTable& pods, const PodBatchDev& b, hipStream_t s);
// dense list of the countable pod rows among [0, n) (out_n: device counter, zeroed by the caller)
void launch_compact_countable(const PodTable& pods, int64_t n, int64_t* out_rows, unsigned long long* out_n, hipStream_t s);
// pod rows of [0, n) ordered by namespace (all of them, or the countable ones); cursor: n_keys device words of scratch,
// n_keys = namespace capacity; out_n: device counter receiving the number of listed rows
void launch_order_rows_by_ns(const PodTable& pods, int64_t n, bool countable_only, uint32_t n_keys, unsigned long long* cursor,
                             int64_t* out_rows, unsigned long long* out_n, hipStream_t s);
// contiguous record ranges of a namespace-ordered list for the G workgroups of a scan, ends moved to namespace boundaries
// (host code, kt_kernels.hip: plan_wg_ranges): range[0 .. G], range[G + 1] = the largest range; no range holds more than
// wg_range_cap(n, G) records.  ns_end = a host copy of the cursor words launch_order_rows_by_ns leaves behind (end of every
// namespace's records); range: G + 2 host words
uint32_t wg_range_cap(int64_t n, int G);
void plan_wg_ranges(const unsigned long long* ns_end, uint32_t n_keys, int64_t n, int G, uint32_t* range);
// scan-ordered copies of meta / atom row (/ request row when v_req is given) of the listed rows
struct PackPlan;  // kt_index.h
// pk + v_pk (nullable): also the packed request words of every listed pod
// pos (nullable, one int32 per pod row, -1 = not listed): pos[row] = the record's position in the view
void launch_build_scan_view(const PodTable& pods, int64_t n, const int64_t* rows, uint64_t* v_meta, uint16_t* v_latom,
                            int64_t* v_req, hipStream_t s, const PackPlan* pk = nullptr, uint64_t* v_pk = nullptr, int32_t* pos = nullptr);
// a pod event batch applied to the scan views in place (kt_kernels.hip: kt_patch_scan_views)
struct ViewPatch;  // kt_index.h
void launch_patch_scan_views(const PodTable& pods, int64_t n, const int64_t* rows, int64_t row0, const ViewPatch& v, hipStream_t s);
// exact per-dimension sums of |request| over the valid rows of [0, n): out[2d] low-half sum, out[2d+1] high-half sum (32 words)
void launch_sum_abs_requests(const PodTable& pods, int64_t n, unsigned long long* out, hipStream_t s);
void launch_delete_pods(const PodTable& pods, int64_t n, const int64_t* rows_dev, hipStream_t s);
// small pod event batches (n <= kFeedSmallMax) as ONE launch: ingest + translate + view patch / delete + view patch
constexpr int64_t kFeedSmallMax = 256;
struct IndexDev;
void launch_feed_small(const PodTable& pods, const PodBatchDev& b, const IndexDev& ix, unsigned long long* n_overflow, bool do_translate,
                       const ViewPatch* v, unsigned long long* host_overflow, const void* stage_src, void* stage_dst, uint32_t stage_bytes,
                       unsigned long long* host_seq, unsigned long long seq, hipStream_t s);
// n <= kFeedFewMax pods, whose batch fits kFeedFewSlotMax bytes: one wave per pod (kt_feed_few); b_off holds BYTE OFFSETS into the slot
constexpr int64_t kFeedFewMax = 4;
constexpr uint32_t kFeedFewSlotMax = 32 * 1024;
void launch_feed_few(const PodTable& pods, const PodBatchDev& b_off, bool has_rows, const IndexDev& ix, unsigned long long* n_overflow, bool do_translate,
                     const ViewPatch* v, unsigned long long* host_overflow, const void* slot, uint32_t slot_bytes, unsigned long long* host_seq,
                     unsigned long long seq, hipStream_t s);
void launch_unfeed_small(const PodTable& pods, int64_t n, const int64_t* rows, const ViewPatch* v, unsigned long long* host_seq,
                         unsigned long long seq, hipStream_t s);
void launch_gather_pod_requests(const PodTable& pods, int64_t n, const int64_t* rows_dev, int64_t* out_v,
                                uint32_t* out_present, hipStream_t s);

void launch_aggregate_dense(const PodTable& pods, int64_t n_rows, const SelProgram& sp, bool keys,
                            unsigned long long* partial, hipStream_t s, int limb = 0);
// recs (nullable): also build the CheckRec<rec_DT> of every throttle for isThrottledOnEqual = rec_eq
// consume: the kernel leaves the partial rows zeroed behind
void launch_finalize(const ThrTables& tt, const SelProgram& sp, int D, unsigned long long* partial, bool consume,
                     int64_t now_s, int32_t now_ns, bool apply, const ReconcileOut& out, void* recs, int rec_DT, bool rec_eq,
                     const ReqBound& vmax, hipStream_t s, const uint8_t* row_mask = nullptr, unsigned long long* partial_hi = nullptr);
// partial_hi (nullable): wide sums — partial = sums of the requests' low 32-bit limbs, partial_hi = sums of their high parts
// row_mask (nullable, device, T bytes): rows with 0 are not reconciled — they keep and report their stored status
void launch_prepare_check(const ThrTables& tt, int T, int D, int DT, bool on_equal, void* recs, const ReqBound& vmax, hipStream_t s);
void launch_check_dense(const PodTable& pods, int64_t n, const int64_t* rows_dev, const SelProgram& sp, bool keys,
                        const void* recs, uint64_t* summary, uint8_t* status, hipStream_t s);

// sequential admission of a pod queue with reservation (kt_kernels_admit.hip) over n_pages >= 1 pages (a page = an engine
// of <= 16 resource names; kt_admit_launch is one page): one descriptor per page, the offsets are filled in by the launcher,
// which also copies the descriptors to pages_dev (n_pages entries of device memory) and records pages_copied behind that
// copy: `pages` must stay unmodified until the event has completed.  The mutable state (reserved amounts of all throttles
// of every page) lives in LDS while admit_paged_state_bytes + the list fit, else in `scratch` (admit_paged_state_bytes
// bytes).  false: the list does not fit LDS, or (*hip_err != hipSuccess) the copy of the descriptors failed
struct AdmitPage {
  const uint32_t* pod_flags;  // the page's pod flags (presence bits of ITS names)
  const int64_t* req;         // [pods][DS]
  ThrTables tt;
  int32_t D, DS;
  uint32_t off_rv, off_rc, off_rp;
};
size_t admit_state_bytes(int T, int D);  // one page
size_t admit_paged_state_bytes(int T, const AdmitPage* pages, int n_pages);
// gangs (kt_admit_gangs_launch): the queue positions [off_dev[g], off_dev[g + 1]) are admitted all or nothing, out_dev[g] = 1
// admitted / 0 rolled back; the gang form keeps admit_gang_extra_bytes more state (LDS, or scratch behind the pages' state)
// elastic gangs (kt_admit_gangs_elastic_launch, min_dev set): gang g is kept iff at least min_dev[g] members succeeded and none whose
// flags_dev byte has bit 0 failed; members_dev[g] = the members that stay reserved, 0 rolled back.  The same extra state
struct AdmitGangs {
  const int64_t* off_dev;  // [n_gangs + 1] in device memory
  int64_t n_gangs;
  uint8_t* out_dev;        // [n_gangs]
  const int64_t* min_dev = nullptr;    // [n_gangs] nullable: all or nothing
  const uint8_t* flags_dev = nullptr;  // [n] nullable: no member is required
  int64_t* members_dev = nullptr;      // [n_gangs] with min_dev
};
size_t admit_gang_extra_bytes(int T, int n_pages);
bool launch_admit(AdmitPage* pages, int n_pages, AdmitPage* pages_dev, hipEvent_t pages_copied, int64_t n, const int64_t* rows_dev, int T,
                  bool on_equal, bool commit, uint8_t* status, uint64_t* summary, void* scratch, bool force_global, hipStream_t s,
                  hipError_t* hip_err, const AdmitGangs* gangs = nullptr);
// how many copies of each pod the throttles still admit (kt_kernels_headroom.hip): one wave per pod over the same page descriptors
// (the state offsets are not used: nothing is mutable), copied and guarded by pages_copied as launch_admit does.  status / summary:
// page 0's check of the same rows; copies [n], limiting [n] out; cap in [1, 2^31 - 1].  false: *hip_err says why
bool launch_headroom(const AdmitPage* pages, int n_pages, AdmitPage* pages_dev, hipEvent_t pages_copied, int64_t n, const int64_t* rows_dev, int T,
                     bool on_equal, uint32_t cap, const uint8_t* status, const uint64_t* summary, int64_t* copies, int32_t* limiting,
                     hipStream_t s, hipError_t* hip_err);
// how many copies of each gang [gang_off[g], gang_off[g + 1]) the throttles still admit (kt_kernels_headroom_gangs.hip): one wave
// per gang, lane = a candidate number of copies.  status / summary: ONE check over the members of all gangs; the stored tables of
// the one page; copies [n_gangs], limiting [n_gangs], blocker [n_gangs] out; cap in [1, 2^31 - 1]
void launch_headroom_gangs(const AdmitPage& pg, int64_t n_gangs, const int64_t* rows_dev, const int64_t* gang_off_dev, int T, bool on_equal,
                           uint32_t cap, const uint8_t* status, const uint64_t* summary, int64_t* copies, int32_t* limiting, int64_t* blocker,
                           hipStream_t s);
// ... over n_pages >= 1 pages (kt_kernels_headroom_gangs_paged.hip): the descriptors of launch_headroom, copied to pages_dev and
// guarded by pages_copied as there; status / summary: ONE check of page 0 over rows_dev [n], the members of all gangs; copies
// [n_gangs], limiting [n_gangs] and blocker [n_gangs] out, on page 0.  false: the copy failed (*hip_err)
bool launch_headroom_gangs_paged(const AdmitPage* pages, int n_pages, AdmitPage* pages_dev, hipEvent_t pages_copied, int64_t n_gangs,
                                 const int64_t* rows_dev, const int64_t* gang_off_dev, int T, bool on_equal, uint32_t cap, const uint8_t* status,
                                 const uint64_t* summary, int64_t* copies, int32_t* limiting, int64_t* blocker, hipStream_t s,
                                 hipError_t* hip_err);
// the shortest victim prefix per preemptor (kt_kernels_preempt.hip): one wave per preemptor.  rows_dev [n + m]: the preemptors,
// then the candidates; status / summary: ONE check over those rows; partial: aggregate rows with exact per-name contributor counts;
// calc / calc_updated / error: a dry finalize at `now`; prefix [n] and victims [n][m] out
void launch_preempt(const AdmitPage& pg, int64_t n, int64_t m, const int64_t* rows_dev, int T, bool on_equal, const uint8_t* status,
                    const uint64_t* summary, const unsigned long long* partial, const AmountTab& calc, const uint8_t* calc_updated,
                    const uint8_t* error, int64_t* prefix, uint8_t* victims, hipStream_t s);
// the gang form (kt_kernels_preempt_gangs.hip): one wave per gang, the same inputs over members ++ candidates (n members in all);
// gang g is the queue positions [gang_off_dev[g], gang_off_dev[g + 1]) of rows_dev (device memory).  prefix [n_gangs], victims
// [n_gangs][m] and blocker [n_gangs] (the first member that is not Success in S_0, a queue position; -1 with prefix 0) out
void launch_preempt_gangs(const AdmitPage& pg, int64_t n, int64_t m, const int64_t* rows_dev, int64_t n_gangs, const int64_t* gang_off_dev, int T,
                          bool on_equal, const uint8_t* status, const uint64_t* summary, const unsigned long long* partial, const AmountTab& calc,
                          const uint8_t* calc_updated, const uint8_t* error, int64_t* prefix, uint8_t* victims, int64_t* blocker, hipStream_t s);
// the reprieve pass behind it (kt_kernels_reprieve.hip): one wave per preemptor walks its masked victims back, last first, and
// rewrites victims [n][m] in place; prefix is read.  The list of a preemptor's reconciled affecting throttles lives in LDS up to
// reprieve_lds_cap(D, limit) entries (limit: a test hook that lowers the capacity, 0 = none), beyond that in `ws`:
// reprieve_ws_bytes bytes of device memory (0: no list can outgrow LDS, ws may be null)
uint32_t reprieve_lds_cap(int D, uint32_t limit);
size_t reprieve_ws_bytes(int T, int D, int64_t n, uint32_t lds_cap_limit);
void launch_preempt_reprieve(const AdmitPage& pg, int64_t n, int64_t m, const int64_t* rows_dev, int T, bool on_equal, const uint8_t* status,
                             const unsigned long long* partial, const AmountTab& calc, const uint8_t* calc_updated, const uint8_t* error,
                             const int64_t* prefix, uint8_t* victims, void* ws, uint32_t lds_cap_limit, hipStream_t s);
// the reprieve pass behind the gang form (kt_kernels_preempt_gangs_reprieve.hip): one wave per gang walks its masked victims back,
// last first, judging the members in order, and rewrites victims [n_gangs][m] in place; prefix [n_gangs] is read.  LDS capacity
// and workspace as for launch_preempt_reprieve, sized with n_gangs in the place of n
void launch_preempt_gangs_reprieve(const AdmitPage& pg, int64_t n, int64_t m, const int64_t* rows_dev, int64_t n_gangs, const int64_t* gang_off_dev,
                                   int T, bool on_equal, const uint8_t* status, const unsigned long long* partial, const AmountTab& calc,
                                   const uint8_t* calc_updated, const uint8_t* error, const int64_t* prefix, uint8_t* victims, void* ws,
                                   uint32_t lds_cap_limit, hipStream_t s);
// the shortest victim prefix that lets a gang's QUORUM in (kt_kernels_preempt_gangs_elastic.hip): one wave per gang, the members
// walked in order in every S_k, a failed member reserving nowhere.  launch_preempt_gangs' inputs plus min_dev [n_gangs] and flags_dev
// [n] (nullable: no member is required; bit 0 = required); `reprieve`: the masked victims are walked back in the same kernel.
// prefix, members (the successes in the final state) and blocker [n_gangs] and victims [n_gangs][m] out.  A gang's union of
// affecting throttles lives in LDS up to preempt_gangs_elastic_lds_cap(D, limit) entries (limit: a test hook that lowers the
// capacity, 0 = none), beyond that in `ws`: preempt_gangs_elastic_ws_bytes bytes of device memory (0: no union can outgrow LDS, ws
// may be null)
uint32_t preempt_gangs_elastic_lds_cap(int D, uint32_t limit);
size_t preempt_gangs_elastic_ws_bytes(int T, int D, int64_t n_gangs, uint32_t lds_cap_limit);
void launch_preempt_gangs_elastic(const AdmitPage& pg, int64_t n, int64_t m, const int64_t* rows_dev, int64_t n_gangs, const int64_t* gang_off_dev,
                                  const int64_t* min_dev, const uint8_t* flags_dev, int T, bool on_equal, bool reprieve, const uint8_t* status,
                                  const uint64_t* summary, const unsigned long long* partial, const AmountTab& calc, const uint8_t* calc_updated,
                                  const uint8_t* error, int64_t* prefix, uint8_t* victims, int64_t* members, int64_t* blocker, void* ws,
                                  uint32_t lds_cap_limit, hipStream_t s);
// the victim prefix and its reprieve pass over n_pages >= 1 pages (kt_kernels_preempt_paged.hip).  One descriptor per page: the
// page as kt_admit reads it (the state offsets are unused), and of that page's own dense aggregate and dry finalize at `now` the
// partial rows with exact contributor counts, the calculated threshold and the calc_updated / error bytes.  launch_preempt_paged
// copies the descriptors to pages_dev and records pages_copied behind the copy (`pages` stays unmodified until the event has
// completed), then launches kt_preempt_paged: rows_dev [n + m], status / summary: ONE check of page 0 over those rows; prefix [n]
// and victims [n][m] out, on page 0.  false: the copy failed (*hip_err).  launch_preempt_reprieve_paged, behind it on the same
// stream, reads the same device descriptors; its list state is sized with the sum of the pages' D in D's place
// (reprieve_paged_ws_bytes bytes of workspace, 0: no list can outgrow LDS)
struct PreemptPage {
  AdmitPage pg;
  const unsigned long long* partial;  // [T][partial_stride(pg.D)]
  AmountTab calc;
  const uint8_t* calc_updated;        // [T]
  const uint8_t* error;               // [T]
};
bool launch_preempt_paged(const PreemptPage* pages, int n_pages, PreemptPage* pages_dev, hipEvent_t pages_copied, int64_t n, int64_t m,
                          const int64_t* rows_dev, int T, bool on_equal, const uint8_t* status, const uint64_t* summary, int64_t* prefix,
                          uint8_t* victims, hipStream_t s, hipError_t* hip_err);
size_t reprieve_paged_ws_bytes(int T, const PreemptPage* pages, int n_pages, int64_t n, uint32_t lds_cap_limit);
void launch_preempt_reprieve_paged(const PreemptPage* pages, int n_pages, const PreemptPage* pages_dev, int64_t n, int64_t m, const int64_t* rows_dev,
                                   int T, bool on_equal, const uint8_t* status, const int64_t* prefix, uint8_t* victims, void* ws,
                                   uint32_t lds_cap_limit, hipStream_t s);
// the gang forms over the same descriptors (kt_kernels_preempt_gangs_paged.hip): one wave per gang.  rows_dev [n + m]: the members of
// all gangs, then the candidates; gang g is the queue positions [gang_off_dev[g], gang_off_dev[g + 1]) (device memory); status /
// summary: ONE check of page 0 over those rows.  launch_preempt_gangs_paged copies the descriptors and records pages_copied as
// launch_preempt_paged does; prefix [n_gangs], victims [n_gangs][m] and blocker [n_gangs] out, on page 0.  false: the copy failed
// (*hip_err).  launch_preempt_gangs_reprieve_paged, behind it on the same stream, reads the same device descriptors; LDS capacity
// and workspace as for launch_preempt_reprieve_paged, sized with n_gangs in the place of n
bool launch_preempt_gangs_paged(const PreemptPage* pages, int n_pages, PreemptPage* pages_dev, hipEvent_t pages_copied, int64_t n, int64_t m,
                                const int64_t* rows_dev, int64_t n_gangs, const int64_t* gang_off_dev, int T, bool on_equal, const uint8_t* status,
                                const uint64_t* summary, int64_t* prefix, uint8_t* victims, int64_t* blocker, hipStream_t s, hipError_t* hip_err);
void launch_preempt_gangs_reprieve_paged(const PreemptPage* pages, int n_pages, const PreemptPage* pages_dev, int64_t n, int64_t m,
                                         const int64_t* rows_dev, int64_t n_gangs, const int64_t* gang_off_dev, int T, bool on_equal,
                                         const uint8_t* status, const int64_t* prefix, uint8_t* victims, void* ws, uint32_t lds_cap_limit,
                                         hipStream_t s);
// the first instant at which a pod passes (kt_kernels_forecast.hip): one wave per pod, lane = instant position.  rows_dev [n];
// inst_s / inst_ns [m] in device memory, strictly ascending; status / summary: ONE check over those rows; partial: aggregate rows
// with exact per-name contributor counts; error: the error bytes of a dry finalize; first [n] and verdicts [n][m] out
void launch_forecast(const AdmitPage& pg, int64_t n, int64_t m, const int64_t* rows_dev, const int64_t* inst_s, const int32_t* inst_ns, int T,
                     bool on_equal, const uint8_t* status, const uint64_t* summary, const unsigned long long* partial, const uint8_t* error,
                     int64_t* first, uint8_t* verdicts, hipStream_t s);
// how many copies of a pod the throttles admit at each instant (kt_kernels_headroom_forecast.hip): launch_forecast's inputs plus cap
// and want (1 <= want <= cap <= 2^31 - 1); first [n], copies [n][m] and limiting [n][m] out
void launch_headroom_forecast(const AdmitPage& pg, int64_t n, int64_t m, const int64_t* rows_dev, const int64_t* inst_s, const int32_t* inst_ns,
                              int T, bool on_equal, uint32_t cap, uint32_t want, const uint8_t* status, const uint64_t* summary,
                              const unsigned long long* partial, const uint8_t* error, int64_t* first, int64_t* copies, int32_t* limiting,
                              hipStream_t s);
// ... over n_pages >= 1 pages (kt_kernels_forecast_paged.hip): the descriptors of launch_preempt_paged (every page's own dense
// aggregate and the error bytes of its dry finalize; calc / calc_updated are not read), copied to pages_dev and guarded by
// pages_copied as there; status / summary: ONE check of page 0 over rows_dev [n]; first [n] and verdicts [n][m] out, on page 0.
// false: the copy failed (*hip_err)
bool launch_forecast_paged(const PreemptPage* pages, int n_pages, PreemptPage* pages_dev, hipEvent_t pages_copied, int64_t n, int64_t m,
                           const int64_t* rows_dev, const int64_t* inst_s, const int32_t* inst_ns, int T, bool on_equal, const uint8_t* status,
                           const uint64_t* summary, int64_t* first, uint8_t* verdicts, hipStream_t s, hipError_t* hip_err);
// the first instant at which a whole gang is admitted (kt_kernels_forecast_gangs.hip): one wave per gang, lane = instant position.
// rows_dev [n]: the members of all gangs; gang g is the queue positions [gang_off_dev[g], gang_off_dev[g + 1]) (device memory);
// instants, status / summary, partial and error as for launch_forecast; first [n_gangs], verdicts [n_gangs][m] and blocker
// [n_gangs][m] out
void launch_forecast_gangs(const AdmitPage& pg, int64_t n_gangs, int64_t m, const int64_t* rows_dev, const int64_t* gang_off_dev,
                           const int64_t* inst_s, const int32_t* inst_ns, int T, bool on_equal, const uint8_t* status, const uint64_t* summary,
                           const unsigned long long* partial, const uint8_t* error, int64_t* first, uint8_t* verdicts, int64_t* blocker,
                           hipStream_t s);
// the first instant at which a gang's QUORUM fits (kt_kernels_forecast_gangs_elastic.hip): one wave per (gang, instant) pair, the
// members walked in order, a failed member reserving nowhere.  launch_forecast_gangs' inputs plus min_dev [n_gangs] and flags_dev [n]
// (nullable: no member is required; bit 0 = required); first [n_gangs] (by a small launch behind the kernel, on the same stream),
// verdicts, members and blocker [n_gangs][m] out.  A pair's union of affecting throttles lives in LDS up to
// forecast_gangs_elastic_lds_cap(D, limit) entries (limit: a test hook that lowers the capacity, 0 = none), beyond that in `ws`:
// forecast_gangs_elastic_ws_bytes bytes of device memory (0: no union can outgrow LDS, ws may be null)
uint32_t forecast_gangs_elastic_lds_cap(int D, uint32_t limit);
size_t forecast_gangs_elastic_ws_bytes(int T, int D, int64_t n_gangs, int64_t m, uint32_t lds_cap_limit);
void launch_forecast_gangs_elastic(const AdmitPage& pg, int64_t n_gangs, int64_t m, const int64_t* rows_dev, const int64_t* gang_off_dev,
                                   const int64_t* min_dev, const uint8_t* flags_dev, const int64_t* inst_s, const int32_t* inst_ns, int T,
                                   bool on_equal, const uint8_t* status, const uint64_t* summary, const unsigned long long* partial,
                                   const uint8_t* error, int64_t* first, uint8_t* verdicts, int64_t* members, int64_t* blocker, void* ws,
                                   uint32_t lds_cap_limit, hipStream_t s);
// how many copies of a whole gang the throttles admit at each instant (kt_kernels_headroom_forecast_gangs.hip): one wave per gang,
// lane = instant position, every lane searches the copies of its own instant.  launch_forecast_gangs' inputs plus cap and want
// (1 <= want <= cap <= 2^31 - 1); first [n_gangs], copies [n_gangs][m], limiting [n_gangs][m] and blocker [n_gangs][m] out
void launch_headroom_forecast_gangs(const AdmitPage& pg, int64_t n_gangs, int64_t m, const int64_t* rows_dev, const int64_t* gang_off_dev,
                                    const int64_t* inst_s, const int32_t* inst_ns, int T, bool on_equal, uint32_t cap, uint32_t want,
                                    const uint8_t* status, const uint64_t* summary, const unsigned long long* partial, const uint8_t* error,
                                    int64_t* first, int64_t* copies, int32_t* limiting, int64_t* blocker, hipStream_t s);
// ... over n_pages >= 1 pages (kt_kernels_forecast_gangs_paged.hip): the descriptors of launch_forecast_paged, copied to pages_dev and
// guarded by pages_copied as there; status / summary: ONE check of page 0 over rows_dev [n], the members of all gangs; first
// [n_gangs], verdicts [n_gangs][m] and blocker [n_gangs][m] out, on page 0.  false: the copy failed (*hip_err)
bool launch_forecast_gangs_paged(const PreemptPage* pages, int n_pages, PreemptPage* pages_dev, hipEvent_t pages_copied, int64_t n_gangs, int64_t m,
                                 const int64_t* rows_dev, const int64_t* gang_off_dev, const int64_t* inst_s, const int32_t* inst_ns, int T,
                                 bool on_equal, const uint8_t* status, const uint64_t* summary, int64_t* first, uint8_t* verdicts, int64_t* blocker,
                                 hipStream_t s, hipError_t* hip_err);
// how many copies of a pod the throttles admit at each instant over n_pages >= 1 pages (kt_kernels_headroom_forecast_paged.hip):
// launch_forecast_paged's inputs plus cap and want (1 <= want <= cap <= 2^31 - 1); first [n], copies [n][m] and limiting [n][m]
// out, on page 0.  false: the copy failed (*hip_err)
bool launch_headroom_forecast_paged(const PreemptPage* pages, int n_pages, PreemptPage* pages_dev, hipEvent_t pages_copied, int64_t n, int64_t m,
                                    const int64_t* rows_dev, const int64_t* inst_s, const int32_t* inst_ns, int T, bool on_equal, uint32_t cap,
                                    uint32_t want, const uint8_t* status, const uint64_t* summary, int64_t* first, int64_t* copies,
                                    int32_t* limiting, hipStream_t s, hipError_t* hip_err);
// how many copies of a whole gang the throttles admit at each instant over n_pages >= 1 pages
// (kt_kernels_headroom_forecast_gangs_paged.hip): launch_forecast_gangs_paged's inputs plus cap and want (1 <= want <= cap <=
// 2^31 - 1); first [n_gangs], copies [n_gangs][m], limiting [n_gangs][m] and blocker [n_gangs][m] out, on page 0.  false: the copy
// failed (*hip_err)
bool launch_headroom_forecast_gangs_paged(const PreemptPage* pages, int n_pages, PreemptPage* pages_dev, hipEvent_t pages_copied, int64_t n_gangs,
                                          int64_t m, const int64_t* rows_dev, const int64_t* gang_off_dev, const int64_t* inst_s,
                                          const int32_t* inst_ns, int T, bool on_equal, uint32_t cap, uint32_t want, const uint8_t* status,
                                          const uint64_t* summary, int64_t* first, int64_t* copies, int32_t* limiting, int64_t* blocker,
                                          hipStream_t s, hipError_t* hip_err);

inline int dt_bucket(int D) { return D <= 4 ? 4 : D <= 8 ? 8 : 16; }
inline int dt_bucket_ix(int D) { return D <= 8 ? 8 : 16; }  // indexed kernels: two instantiations
inline int lt_bucket(int L) { return L <= 8 ? 8 : 16; }

}  // namespace kt
