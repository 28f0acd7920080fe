// kt_host.hpp — C++ mirror of kube-throttler's scheduler plugin on top of the engine's C-ABI.
//
// The reference's host side is Go (pkg/scheduler_plugin/plugin.go); Go is not available in this build
// image, so the layer above include/kt_engine.h is written in C++ with the SAME names, argument meaning
// and error behaviour for the hot path:
//     PluginName, NewPlugin(args), KubeThrottler::Name / PreFilter / Reserve / Unreserve
// plus the informer-side feed (OnPodAdd/..., what the event handlers of
// pkg/controllers/throttle_controller.go:400-536 push) and ReconcileAll (the aggregation part of
// [Cluster]ThrottleController.reconcile for every responsible throttle).
//
// Everything string-shaped lives here: label/namespace/resource interning, resource.Quantity and RFC3339
// parsing, LabelSelectorAsSelector validation, reason-string formatting.  The engine only sees ids and
// exact integers.
#pragma once
#include <cstdint>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/kt_engine.h"

namespace kth {

// ---- k8s.io/apimachinery pkg/api/resource.Quantity, exact (restated) ---------------
// value = nano * 1e-9 ; finer input is rounded away from zero at parse time.
// Format is the suffix family the text was written in; it only steers String() (quantity.go CanonicalizeBytes) and
// is inherited by a sum from the addend that first made it non-zero (Quantity.Add).
enum class Format : uint8_t { DecimalSI = 0, BinarySI = 1, DecimalExponent = 2 };
struct Quantity {
  __int128 nano = 0;
  Format format = Format::DecimalSI;
};
bool ParseQuantity(const std::string& text, Quantity* out, std::string* err);
// Quantity.String(): the canonical text the API server persists (status write-back).  BinarySI
// falls back to DecimalSI for |value| < 1024 and for non-integers; mantissa without trailing zeros, exponent a
// multiple of 3 (DecimalSI / DecimalExponent) or a power of 1024 (BinarySI).
std::string FormatQuantity(const Quantity& q);
// Quantity.Add's format rule: a zero receiver takes the addend's format.
inline void AddQuantity(Quantity* q, const Quantity& y) {
  if (q->nano == 0) q->format = y.format;
  q->nano += y.nano;
}
// value / 10^scale as an exact integer; false when not representable (or beyond int64).
bool ScaledValue(const Quantity& q, int scale, int64_t* out);
std::string FormatDecimalSI(const Quantity& q);

// k8s.io/apimachinery validation.IsQualifiedName / IsValidLabelValue (restated): what makes
// LabelSelectorAsSelector fail on a key or a value.
bool ValidLabelKey(const std::string& key);
bool ValidLabelValue(const std::string& value);

// Go time.Parse(time.RFC3339, text) -> (unix seconds, nanoseconds).
bool ParseRFC3339(const std::string& text, int64_t* sec, int32_t* nsec, std::string* err);

// ---- object model (core/v1 Pod / Namespace, schedule/v1alpha1 Throttle / ClusterThrottle) ---------------
using Labels = std::map<std::string, std::string>;
using ResourceList = std::map<std::string, std::string>;  // resource name -> Quantity text

struct Container {
  ResourceList requests;
};
struct Pod {
  std::string ns, name;
  Labels labels;
  std::string schedulerName, nodeName, phase;
  std::vector<Container> containers, initContainers;
  bool hasOverhead = false;
  ResourceList overhead;
  std::string Key() const { return ns + "/" + name; }
};
struct Namespace {
  std::string name;
  Labels labels;
};
struct LabelSelectorRequirement {
  std::string key, op;  // In | NotIn | Exists | DoesNotExist
  std::vector<std::string> values;
};
struct LabelSelector {
  Labels matchLabels;
  std::vector<LabelSelectorRequirement> matchExpressions;
};
struct SelectorTerm {
  LabelSelector podSelector;
  LabelSelector namespaceSelector;  // ClusterThrottle only
};
struct ResourceAmount {
  bool hasCounts = false;  // resourceCounts != nil
  int64_t pod = 0;
  ResourceList requests;
};
struct TemporaryThresholdOverride {
  std::string begin, end;
  ResourceAmount threshold;
};
struct Throttle {
  bool cluster = false;  // kind ClusterThrottle
  std::string ns, name, throttlerName;
  ResourceAmount threshold;
  std::vector<TemporaryThresholdOverride> overrides;
  std::vector<SelectorTerm> selectorTerms;
  // types.NamespacedName.String(): a ClusterThrottle renders as "/name" (plugin.go:289-295)
  std::string Key() const { return (cluster ? std::string() : ns) + "/" + name; }
};

// status written back by ReconcileAll (what UpdateStatus would persist)
struct ThrottleStatus {
  bool usedHasCounts = false;
  int64_t usedPod = 0;
  std::map<std::string, Quantity> used;
  std::map<std::string, bool> throttledRequests;
  bool throttledPod = false;
  bool calculatedThresholdUpdated = false;
  std::vector<std::string> messages;
  bool error = false;
  // ThrottleSpecBase.NextOverrideHappensIn as an instant: when the controller must reconcile this throttle again
  bool hasNextOverride = false;
  int64_t nextOverrideSec = 0;
  int32_t nextOverrideNsec = 0;
  // !apiequality.Semantic.DeepEqual(thr.Status, *newStatus) (throttle_controller.go:157): UpdateStatus is only called
  // when this is set; otherwise the reference logs "No need to update status"
  bool needsUpdate = false;
  // status.used.resourceRequests as the API server would persist it (Quantity.String())
  std::map<std::string, std::string> UsedStrings() const;
};
// apiequality.Semantic.DeepEqual on the parts of ThrottleStatus a reconcile can change besides calculatedThreshold
// (used, throttled): quantities compare by value (Cmp == 0), nil and empty maps are equal, resourceCounts nil != &{0}.
bool StatusSemanticEqual(const ThrottleStatus& a, const ThrottleStatus& b);

// framework.Code values used by the plugin
enum Code { Success = 0, Error = 1, UnschedulableAndUnresolvable = 3 };
// what PreFilter hands to fh.EventRecorder().Eventf (plugin.go:190-202)
struct Event {
  std::string type, reason, message;
};
struct Status {
  Code code = Success;
  std::vector<std::string> reasons;
  std::vector<Event> events;
  bool IsSuccess() const { return code == Success; }
};

// AdmitGangs: what PreFilter / Reserve answered per pod (in the order of the flattened gangs), and per gang 1 admitted /
// 0 rolled back (every member un-reserved)
struct GangAdmission {
  std::vector<Status> status;
  std::vector<uint8_t> admitted;
};

// AdmitElasticGangs: a gang that starts once its quorum of members fits (PodGroup.minMember / minAvailable) — the members by
// Key(), how many of them must succeed (1 .. size), and per member whether it is required (a launcher, a head node)
struct ElasticGang {
  std::vector<std::string> members;
  int64_t min_members = 0;
  std::vector<uint8_t> required;  // per member, 1: the gang is rolled back when this one fails; empty: none
};
// ... what PreFilter / Reserve answered per pod (in the order of the flattened gangs), and per gang the members that stay reserved
// (0: rolled back, every member un-reserved).  A member is in iff its gang's count is above 0 and its own status is Success
struct ElasticGangAdmission {
  std::vector<Status> status;
  std::vector<int64_t> members;
};

// Headroom: how many further pods of a pod's shape the throttles still admit, and the throttle that stops the next one
struct HeadroomResult {
  int64_t copies = 0;     // in [0, cap]
  std::string limiting;   // Throttle::Key() of the lowest-row throttle that blocks copy number `copies`; empty: none (all cap fit,
                          // or the pod's PreFilter is an Error)
  std::string error;      // not empty: the call failed (unknown pod, engine error) and copies is 0
};

// HeadroomGang: how many further replicas of a whole gang the throttles still admit, and who stops the next one
struct GangHeadroomResult {
  HeadroomResult headroom;  // copies / limiting / error as for Headroom, for the gang as a whole (limiting is empty too when the
                            // blocker's PreFilter is an Error)
  std::string blocker;      // Pod::Key() of the first member of replica number `copies` that is not admitted; empty: all cap fit
};

// Preempt: the pods that would have to go before a blocked pod passes PreFilter
struct PreemptResult {
  bool none = false;                 // no prefix of the candidates lets the pod through (victims is empty)
  std::vector<std::string> victims;  // Pod::Key() of the candidates to delete, in the caller's order; empty and !none: the pod
                                     // already passes against a fresh reconcile
  std::string error;                 // not empty: the call failed (unknown pod, a paged mirror, engine error)
};

// PreemptGang: the pods that would have to go before a whole gang is admitted, and the member that stops it as things stand
struct GangPreemptResult {
  PreemptResult preempt;  // none / victims / error as for Preempt, for the gang as a whole
  std::string blocker;    // Pod::Key() of the first member that is not admitted with nothing deleted; empty: the gang already passes
};

// PreemptElasticGang: the pods that would have to go before a gang's QUORUM is in (ElasticGang's rule), who stops it as things
// stand and how many members are in once the victims are gone
struct ElasticGangPreemptResult {
  PreemptResult preempt;  // none / victims / error as for Preempt, for the gang under its rule (none also where members that never
                          // succeed put the rule out of reach)
  std::string blocker;    // Pod::Key() of the first required member that does not succeed with nothing deleted, else of the first
                          // member that does not; empty: the rule is met as things stand
  int64_t members = 0;    // the members that succeed once the victims are gone; with nothing deleted where `none` is set
};

// RetryAfter: the first instant at which a blocked pod passes PreFilter, among `now` and the override boundaries up to the horizon
struct RetryAfterResult {
  bool has = false;              // some instant of the window lets the pod through: `instant` is the first
  int64_t instantSec = 0;        // the instant (Unix seconds, nanoseconds); == now: the pod passes against a fresh reconcile
  int32_t instantNsec = 0;
  std::string instant;           // ... as RFC3339 (UTC, with nanoseconds where they are not zero)
  // the instants that were judged — now, then every override boundary in (now, now + horizon] — and the KT_VERDICT_* of each
  std::vector<std::pair<int64_t, int32_t>> instants;
  std::vector<uint8_t> verdicts_at;
  std::string error;             // not empty: the call failed (unknown pod, a paged mirror, engine error)
};

// RetryAfterGang: the first instant at which a whole gang is admitted, and the member that stops it at each judged instant
struct GangRetryAfterResult {
  RetryAfterResult retry;                // has / instant / instants / verdicts_at / error as for RetryAfter, for the gang as a whole
  std::vector<std::string> blockers_at;  // per judged instant the Pod::Key() of the first member that is not admitted; empty: the gang passes
};

// RetryAfterElasticGang: the first instant at which a gang's QUORUM fits (ElasticGang's rule), who stops it and how many members
// succeed at each judged instant
struct ElasticGangRetryAfterResult {
  RetryAfterResult retry;                // has / instant / instants / verdicts_at / error as for RetryAfter, for the gang under its rule;
                                         // KT_VERDICT_ERROR at every instant: members that never succeed put the rule out of reach
  std::vector<std::string> blockers_at;  // per judged instant the Pod::Key() of the first required member that does not succeed, else
                                         // of the first member that does not; empty: the rule is met
  std::vector<int64_t> members_at;       // per judged instant the members that succeed, whether or not the rule is met
};

// ScaleAfter: the first instant at which `want` further pods of a pod's shape fit, and how many fit at each judged instant
struct ScaleAfterResult {
  bool found = false;            // some instant of the window admits `want` copies: `instant` is the first
  int64_t instantSec = 0;        // the instant (Unix seconds, nanoseconds); == now: they fit against a fresh reconcile
  int32_t instantNsec = 0;
  std::string instant;           // ... as RFC3339 (UTC, with nanoseconds where they are not zero)
  // the instants that were judged — now, then every override boundary in (now, now + horizon] — and per instant the copies
  // admitted (in [0, want]) and the Throttle::Key() of the lowest-row throttle that stops the next one (empty: all `want` fit, or
  // the pod's PreFilter is an Error)
  std::vector<std::pair<int64_t, int32_t>> instants;
  std::vector<int64_t> copies_at;
  std::vector<std::string> limiting_at;
  std::string error;             // not empty: the call failed (unknown pod, want < 1, a paged mirror, engine error)
};

// ScaleAfterGang: the first instant at which `want` further replicas of a whole gang fit, how many fit at each judged instant and
// which member stops the next one
struct GangScaleAfterResult {
  ScaleAfterResult scale;                // found / instant / instants / copies_at / limiting_at / error as for ScaleAfter, for the gang as
                                         // a whole (limiting is empty too where the blocker's PreFilter is an Error)
  std::vector<std::string> blockers_at;  // per judged instant the Pod::Key() of the first member of replica number copies_at that is
                                         // not admitted; empty: all `want` fit
};

// KubeThrottlerPluginArgs (pkg/scheduler_plugin/plugin_args.go:33-40) + engine sizing
struct PluginArgs {
  std::string name;                 // throttler name (required)
  std::string targetSchedulerName;  // required
  int64_t podCapacity = 1 << 16;
  int32_t throttleCapacity = 1024;
  int32_t namespaceCapacity = 256;
  int32_t maxLabels = KT_MAX_LABELS;
  // resource name -> decimal scale of its fixed-point dimension (e.g. {"cpu",-3}); names not listed are
  // assigned on first sight at scale 0 ("cpu" at -3)
  std::map<std::string, int> resourceScales;
};

extern const char* const PluginName;  // "kube-throttler" (plugin.go:45)

class KubeThrottler {
 public:
  ~KubeThrottler();
  const char* Name() const { return PluginName; }

  // ---- informer feed
  bool OnNamespaceAdd(const Namespace& ns, std::string* err);
  bool OnNamespaceDelete(const std::string& name, std::string* err);
  bool OnPodAdd(const Pod& pod, std::string* err);  // Add; also what the engine has to see of an Update
  // Update handler (throttle_controller.go:451-507, clusterthrottle_controller.go:483-539): when the pod counts in
  // (before or after) and its set of affected throttles changes, its reservation moves with it — removed from the
  // throttles it left, ADDED to the ones it joined (reserved_resource_amounts.go:92-111), until their next reconcile
  // counts it in `used` and un-reserves it.  Then the new object is fed to the engine like OnPodAdd.
  bool OnPodUpdate(const Pod& old_pod, const Pod& new_pod, std::string* err);
  // Delete handler: a scheduled pod that counts in is un-reserved first (throttle_controller.go:508-517)
  bool OnPodDelete(const std::string& key, std::string* err);
  bool OnThrottleAdd(const Throttle& thr, std::string* err);  // also Update; the stored status restarts empty until ReconcileAll
  bool OnThrottleDelete(const std::string& key, bool cluster, std::string* err);

  // ---- plugin.go:148-215
  Status PreFilter(const Pod& pod);
  // ---- plugin.go:217-257 (reservation bookkeeping stays host-side; totals go to the engine)
  Status Reserve(const Pod& pod);
  void Unreserve(const Pod& pod);

  // ---- one scheduling pass over a queue of pending pods (by Key(), fed through OnPodAdd) in order: PreFilter and,
  // on Success, Reserve — ONE engine launch (kt_paged_admit) instead of 2 x n calls; same reserved bookkeeping
  std::vector<Status> AdmitQueue(const std::vector<std::string>& pod_keys);
  // the same pass over GANGS, each admitted all or nothing: per member PreFilter and, on Success, Reserve; a gang with a member
  // that did not succeed gets Unreserve for every member before the next gang — one engine launch per segment
  // (kt_paged_admit_gangs).  Only members of admitted gangs are in the reservation map afterwards (Unreserve works pod by pod)
  GangAdmission AdmitGangs(const std::vector<std::vector<std::string>>& gangs);
  // the same pass over ELASTIC gangs: a gang stays once at least min_members members succeeded and every required one did — the
  // members that succeeded keep their reservation, the others never reserved; otherwise every member gets Unreserve.  One engine
  // launch per segment (kt_paged_admit_gangs_elastic), the segments of AdmitGangs.  Only members that stay are in the reservation
  // map afterwards.  An empty gang is admitted with 0 members; min_members outside [1, size] or a `required` of the wrong length
  // is an Error on every status
  ElasticGangAdmission AdmitElasticGangs(const std::vector<ElasticGang>& gangs);

  // ---- how many replicas fit: the number of pods of pod_key's shape (same namespace, labels and requests) that PreFilter +
  // Reserve would admit one after the other right now, at most cap (1 .. KT_HEADROOM_MAX_CAP), and the throttle that stops the
  // next one — ONE engine call (kt_paged_headroom over the mirror's pages) instead of a dry-run queue of cap pods.  Nothing is
  // reserved.  The copies are FURTHER pods: a pod whose own amount is already part of the reserved totals (Reserve was called for
  // it) is answered as the totals stand, its reservation counts against the copies like anybody else's.
  HeadroomResult Headroom(const std::string& pod_key, int64_t cap);
  // ---- how many replicas of a whole job fit: the number of further gangs of the members' shapes that AdmitGangs would admit one
  // after the other right now, at most cap — each admitted member reserves against the throttles the later members and the later
  // replicas meet, so this is NOT the minimum of the members' own Headroom answers.  ONE engine call (kt_headroom_gangs_launch +
  // kt_headroom_gangs_fetch) instead of a dry-run queue of cap x members pods.  Nothing is reserved; the reserved totals are read
  // as they stand.  A member named twice, an unknown key, an empty gang and a mirror on several pages answer an error.
  GangHeadroomResult HeadroomGang(const std::vector<std::string>& member_keys, int64_t cap);

  // ---- who has to go: the shortest prefix of `candidate_keys` (the caller's order, typically ascending priority) whose deletion,
  // followed by a reconcile of every throttle at `now` (RFC3339), lets pod_key through PreFilter — ONE engine call
  // (kt_preempt_launch + kt_preempt_fetch) instead of delete + ReconcileAll + PreFilter per victim tried.  The victims are the
  // candidates of that prefix that count in a throttle affecting the pod; the others of the prefix may stay.  A dry run: no pod is
  // deleted, no status and no reservation changes.  A mirror that runs on pages (more than KT_MAX_DIMS resource names) answers an
  // error: the engine has no paged form of the query.
  // `reprieve` (kt_preempt_reprieve_launch, still one engine call): the victims of that prefix are then put back one by one, the last
  // of the list first, and each stays back as long as the pod still passes — the second half of the scheduler's selectVictimsOnNode.
  // The names that remain are a minimal set: with non-negative requests no single one of them can stay.
  PreemptResult Preempt(const std::string& pod_key, const std::vector<std::string>& candidate_keys, const std::string& now_rfc3339,
                        bool reprieve = false);
  // ---- who has to go for a whole job: the shortest prefix of `candidate_keys` whose deletion, followed by a reconcile of every
  // throttle at `now`, lets AdmitGangs({member_keys}) admit the gang — each admitted member reserves against the throttles the later
  // members meet, so this is NOT the longest of the members' own prefixes.  ONE engine call (kt_preempt_gangs_launch +
  // kt_preempt_gangs_fetch) instead of delete + ReconcileAll + AdmitGangs per prefix.  A dry run: nothing is deleted, reserved or
  // stored, and the reserved totals are read as they stand.  A member named twice, a member among the candidates and a mirror on
  // several pages answer an error.
  // `reprieve` (kt_preempt_gangs_reprieve_launch, still one engine call): the victims of that prefix are then put back one by one, the
  // last of the list first, and each stays back as long as the whole gang is still admitted.  The members' own reprieved sets do not
  // compose into this one: the later members meet what the earlier ones reserved.
  GangPreemptResult PreemptGang(const std::vector<std::string>& member_keys, const std::vector<std::string>& candidate_keys,
                                const std::string& now_rfc3339, bool reprieve = false);
  // The first instant in [now, now + horizon] at which PreFilter(pod) is Success if every throttle were reconciled then
  // (temporaryThresholdOverrides begin and end): kt_override_instants for the boundaries, ONE kt_forecast_launch over
  // now ++ boundaries.  What a PreFilter rejection path asks to set a backoff.  A dry run; a mirror on several pages refuses.
  RetryAfterResult RetryAfter(const std::string& pod_key, const std::string& now_rfc3339, int64_t horizon_seconds);
  // The same for a gang (a job whose pods only run together): the first instant in [now, now + horizon] at which an in-order
  // admission of the members — each admitted member reserves against the throttles the later ones meet — admits all of them, and
  // per judged instant the member that stops it.  kt_override_instants for the boundaries, ONE kt_forecast_gangs_launch over
  // now ++ boundaries.  The members' own RetryAfter answers do not compose into this one.  A dry run; a member named twice, an
  // unknown key, an empty gang and a mirror on several pages answer an error.
  GangRetryAfterResult RetryAfterGang(const std::vector<std::string>& member_keys, const std::string& now_rfc3339, int64_t horizon_seconds);
  // PreemptGang under ElasticGang's rule — the eviction set of a job admitted with minMember: at least `min_members` of the
  // members, and every member whose `required` byte is set (empty: none), have to succeed; the shortest prefix of the candidates
  // that achieves it, with `reprieve` shrunk to a minimal set.  A quorum outside 1 .. size or a `required` of another length answers
  // an error worded as AdmitElasticGangs words it; a mirror on several pages answers the "pages" error.  Nothing is changed
  ElasticGangPreemptResult PreemptElasticGang(const std::vector<std::string>& member_keys, int64_t min_members,
                                              const std::vector<uint8_t>& required, const std::vector<std::string>& candidate_keys,
                                              const std::string& now_rfc3339, bool reprieve = false);
  // RetryAfterGang under ElasticGang's rule — the backoff of a job admitted with minMember: at least `min_members` of the members,
  // walked in order (one that fails reserves nowhere), and every member whose `required` byte is set (empty: none) succeed.  The
  // boundaries come from kt_override_instants, then ONE kt_forecast_gangs_elastic_launch over now ++ boundaries.  A rule defect
  // answers an error worded as AdmitElasticGangs words it; a mirror on several pages answers the "pages" error.  Nothing is changed
  ElasticGangRetryAfterResult RetryAfterElasticGang(const std::vector<std::string>& member_keys, int64_t min_members,
                                                    const std::vector<uint8_t>& required, const std::string& now_rfc3339,
                                                    int64_t horizon_seconds);

  // When do `want` replicas fit: per instant of now ++ the override boundaries in (now, now + horizon] the number of further pods
  // of pod_key's shape that PreFilter + Reserve would admit one after the other if every throttle were reconciled then (at most
  // `want`), the throttle that stops the next one, and the first instant at which all `want` fit.  kt_override_instants for the
  // boundaries, ONE kt_headroom_forecast_launch over now ++ boundaries with cap = want — what an autoscaler asks before it
  // scales a Job up for the night window.  A dry run; the reserved totals are read as they stand.  An unknown key, want < 1 and a
  // mirror on several pages answer an error.
  ScaleAfterResult ScaleAfter(const std::string& pod_key, int64_t want, const std::string& now_rfc3339, int64_t horizon_seconds);

  // The same for a gang: per instant of now ++ the override boundaries the number of further whole replicas of the members' shapes
  // that AdmitGangs would admit one after the other if every throttle were reconciled then (at most `want`), the throttle and the
  // member that stop the next one, and the first instant at which all `want` fit.  Each admitted member reserves against the
  // throttles the later members and the later replicas meet: the members' own ScaleAfter answers do not compose into this one.
  // ONE kt_headroom_forecast_gangs_launch over now ++ boundaries with cap = want.  A dry run; a member named twice, an unknown key,
  // an empty gang, want < 1 and a mirror on several pages answer an error.
  GangScaleAfterResult ScaleAfterGang(const std::vector<std::string>& member_keys, int64_t want, const std::string& now_rfc3339,
                                      int64_t horizon_seconds);

  // ---- reconcile of every responsible throttle at `now` (RFC3339); fills per-throttle status by Key()
  bool ReconcileAll(const std::string& now_rfc3339, std::map<std::string, ThrottleStatus>* out, std::string* err);

  // CheckThrottleStatus of (pod, throttle key) from the last PreFilter of that pod ("" = not affected)
  std::string LastStatusOf(const std::string& throttle_key) const;

  struct Impl;  // engine handle, dictionaries, reserved cache

 private:
  friend std::unique_ptr<KubeThrottler> NewPlugin(const PluginArgs&, std::string*);
  KubeThrottler() = default;
  std::unique_ptr<Impl> p_;
};

// NewPlugin (plugin.go:63-146): validates the args like DecodePluginArgs (plugin_args.go:42-60) and creates
// the engine.  Returns nullptr + err on failure (no GPU => KT_ERR_NO_DEVICE text).
std::unique_ptr<KubeThrottler> NewPlugin(const PluginArgs& args, std::string* err);

}  // namespace kth
