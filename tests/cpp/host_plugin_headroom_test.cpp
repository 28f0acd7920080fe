// host_plugin_headroom_test — KubeThrottler::Headroom (one kt_paged_headroom over the mirror's pages) on plugin A against the plain
// calls on a twin B: fresh pods of the probed pod's shape go through PreFilter and, on Success, Reserve one after the other; the
// count of those admitted is the headroom, and the throttle Headroom names blocks the first one that is not.
// Scenarios: one throttle with a count and cpu; reservations made in between (the answer moves with the reserved totals, a pod
// that holds a reservation itself is answered as the totals stand); a pod no throttle affects; a cluster of 20 resource names
// (two pages) whose limiting name lives on the second page.  Needs a GPU.  Exit code 0 = all expectations held.
#include <cstdio>
#include <string>

#include "kt_host.hpp"

using namespace kth;

static int g_fail = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      ++g_fail;                                                       \
      fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                                 \
  } while (0)

static std::unique_ptr<KubeThrottler> Make() {
  PluginArgs a;
  a.name = "kube-throttler";
  a.targetSchedulerName = "my-scheduler";
  std::string err;
  auto k = NewPlugin(a, &err);
  if (!k) fprintf(stderr, "NewPlugin: %s\n", err.c_str());
  return k;
}
static Pod MakePod(const std::string& name, const ResourceList& requests, const std::string& app = "job") {
  Pod p;
  p.ns = "ns1";
  p.name = name;
  p.labels["app"] = app;
  p.schedulerName = "my-scheduler";
  p.phase = "Pending";
  Container c;
  c.requests = requests;
  p.containers.push_back(c);
  return p;
}

static KubeThrottler *A, *B;
static int g_copy = 0;
static Pod Fed(const Pod& p) {
  std::string e;
  EXPECT(A->OnPodAdd(p, &e) && B->OnPodAdd(p, &e));
  return p;
}
// The plain way, on B: fresh pods shaped like `shape`, PreFilter + Reserve until one is not admitted (at most cap); the copies
// are taken out again.  *blocker_is_blocking: the throttle A named holds a blocking status for the first pod that did not fit.
static int64_t PlainHeadroom(const Pod& shape, int64_t cap, const std::string& named, bool* named_blocks) {
  std::vector<Pod> made;
  std::string e;
  int64_t n = 0;
  *named_blocks = false;
  for (; n < cap; ++n) {
    Pod c = shape;
    c.name = "copy" + std::to_string(g_copy++);
    made.push_back(c);
    Status st = B->PreFilter(c);
    if (st.IsSuccess()) st = B->Reserve(c);
    if (!st.IsSuccess()) {
      const std::string s = named.empty() ? std::string() : B->LastStatusOf(named);
      *named_blocks = !s.empty() && s != "not-throttled";
      break;
    }
  }
  for (auto& c : made) {
    B->Unreserve(c);
    EXPECT(B->OnPodDelete(c.Key(), &e));
  }
  return n;
}
// Headroom on A == the plain way on B
static HeadroomResult Both(const Pod& p, int64_t cap) {
  HeadroomResult got = A->Headroom(p.Key(), cap);
  EXPECT(got.error.empty());
  bool named_blocks = false;
  const int64_t want = PlainHeadroom(p, cap, got.limiting, &named_blocks);
  if (got.copies != want) fprintf(stderr, "%s: Headroom %lld, the plain way %lld\n", p.Key().c_str(), (long long)got.copies, (long long)want);
  EXPECT(got.copies == want);
  EXPECT(got.limiting.empty() == (want == cap));
  EXPECT(named_blocks == (want < cap));
  return got;
}

int main() {
  auto a = Make(), b = Make();
  if (!a || !b) return 2;
  A = a.get(), B = b.get();
  std::string err;
  Namespace ns{"ns1", {}};
  Throttle t;  // 6 pods, 3 cpu for the pods of the job label
  t.ns = "ns1", t.name = "jobs", t.throttlerName = "kube-throttler";
  t.threshold.hasCounts = true, t.threshold.pod = 6;
  t.threshold.requests = {{"cpu", "3"}};
  SelectorTerm term;
  term.podSelector.matchLabels["app"] = "job";
  t.selectorTerms.push_back(term);
  for (auto* k : {A, B}) EXPECT(k->OnNamespaceAdd(ns, &err) && k->OnThrottleAdd(t, &err));
  std::map<std::string, ThrottleStatus> st;
  for (auto* k : {A, B}) EXPECT(k->ReconcileAll("2026-01-01T00:00:00Z", &st, &err));

  // ---- one throttle: cpu stops the big pods, the count the small ones, a request above the threshold fits never
  Pod half = Fed(MakePod("half", {{"cpu", "500m"}})), small = Fed(MakePod("small", {{"cpu", "100m"}}));
  Pod big = Fed(MakePod("big", {{"cpu", "1200m"}})), huge = Fed(MakePod("huge", {{"cpu", "4"}}));
  Pod other = Fed(MakePod("other", {{"cpu", "4"}}, "web"));
  HeadroomResult r = Both(half, 24);
  EXPECT(r.copies == 6 && r.limiting == "ns1/jobs");
  EXPECT(Both(small, 24).copies == 6);
  EXPECT(Both(big, 24).copies == 2);
  EXPECT(Both(huge, 24).copies == 0);
  EXPECT(Both(half, 4).copies == 4);  // the cap
  r = Both(other, 9);                 // no throttle affects it
  EXPECT(r.copies == 9 && r.limiting.empty());
  EXPECT(!A->Headroom("ns1/nobody", 4).error.empty());
  EXPECT(!A->Headroom(half.Key(), 0).error.empty());

  // ---- the answer moves with the reserved totals; `half` holds a reservation itself and is answered as the totals stand
  for (auto* k : {A, B}) {
    EXPECT(k->PreFilter(half).IsSuccess() && k->Reserve(half).IsSuccess());
    EXPECT(k->PreFilter(big).IsSuccess() && k->Reserve(big).IsSuccess());
  }
  EXPECT(Both(half, 24).copies == 2);  // 1.7 of 3 cpu reserved: 2 x 500m more; 2 of 6 pods
  EXPECT(Both(small, 24).copies == 4);  // the count
  EXPECT(Both(big, 24).copies == 1);
  for (auto* k : {A, B}) k->Unreserve(big);
  EXPECT(Both(half, 24).copies == 5);

  // ---- 20 resource names (two pages): every name of the threshold allows 10, the pod asks 3 of a name on the second page
  Throttle w;
  w.ns = "ns1", w.name = "wide", w.throttlerName = "kube-throttler";
  for (int i = 0; i < 20; ++i) {
    char name[32];
    snprintf(name, sizeof name, "example.com/r%02d", i);
    w.threshold.requests[name] = "10";
  }
  SelectorTerm wt;
  wt.podSelector.matchLabels["app"] = "wide";
  w.selectorTerms.push_back(wt);
  for (auto* k : {A, B}) EXPECT(k->OnThrottleAdd(w, &err));
  for (auto* k : {A, B}) EXPECT(k->ReconcileAll("2026-01-01T00:00:00Z", &st, &err));
  Pod w1 = Fed(MakePod("w1", {{"example.com/r00", "1"}, {"example.com/r17", "2"}, {"example.com/r19", "3"}}, "wide"));
  Pod w2 = Fed(MakePod("w2", {{"example.com/r01", "2"}, {"example.com/r18", "1"}}, "wide"));
  r = Both(w1, 24);
  EXPECT(r.copies == 3 && r.limiting == "ns1/wide");
  EXPECT(Both(w2, 24).copies == 5);
  for (auto* k : {A, B}) EXPECT(k->PreFilter(w1).IsSuccess() && k->Reserve(w1).IsSuccess());
  EXPECT(Both(w1, 24).copies == 2);
  EXPECT(Both(w2, 24).copies == 5);
  EXPECT(Both(half, 24).copies == 5);  // the first throttle, untouched by the wide one

  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
