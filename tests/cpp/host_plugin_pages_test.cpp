// host_plugin_pages_test — the C++ plugin mirror with more than 16 resource names (one engine per page of 16).
// Plugin A learns its names as they arrive: page 1 is created by a name first seen AFTER a ReconcileAll.  Twin B
// registers every name up front through resourceScales.  Both must answer PreFilter (codes, reasons, events),
// Reserve / Unreserve, ReconcileAll (UsedStrings, throttledRequests, counts) alike, and A's AdmitQueue must equal
// PreFilter + Reserve pod by pod on B.  Needs a GPU.  Exit code 0 = all expectations held.
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

static const char* NOW = "2026-01-01T00:00:00Z";
static std::string R(int i) { return "example.com/r" + std::to_string(100 + i).substr(1); }

static std::unique_ptr<KubeThrottler> Make(bool all_names) {
  PluginArgs a;
  a.name = "kube-throttler";
  a.targetSchedulerName = "my-scheduler";
  if (all_names) {
    a.resourceScales["cpu"] = -3;
    for (int i = 0; i < 30; ++i) a.resourceScales[R(i)] = 0;
  }
  std::string err;
  auto k = NewPlugin(a, &err);
  if (!k) fprintf(stderr, "NewPlugin: %s\n", err.c_str());
  return k;
}
static Pod MakePod(const std::string& name, const ResourceList& req, bool scheduled) {
  Pod p;
  p.ns = "ns1";
  p.name = name;
  p.labels["app"] = "web";
  p.schedulerName = "my-scheduler";
  p.phase = scheduled ? "Running" : "Pending";
  if (scheduled) p.nodeName = "node-1";
  Container c;
  c.requests = req;
  p.containers.push_back(c);
  return p;
}
static Throttle MakeThr(const std::string& name, int pods, const ResourceList& req) {
  Throttle t;
  t.ns = "ns1";
  t.name = name;
  t.throttlerName = "kube-throttler";
  if (pods >= 0) t.threshold.hasCounts = true, t.threshold.pod = pods;
  t.threshold.requests = req;
  SelectorTerm term;
  term.podSelector.matchLabels["app"] = "web";
  t.selectorTerms.push_back(term);
  return t;
}
static bool Same(const Status& a, const Status& b) { 
  if (a.code != b.code || a.reasons != b.reasons || a.events.size() != b.events.size()) return false;
  for (size_t i = 0; i < a.events.size(); ++i)
    if (a.events[i].message != b.events[i].message) return false;
  return true;
}
static void Feed(KubeThrottler& k, const Pod& p) { std::string e; EXPECT(k.OnPodAdd(p, &e)); if (!e.empty()) fprintf(stderr, "%s\n", e.c_str()); }
static void Feed(KubeThrottler& k, const Throttle& t) { std::string e; EXPECT(k.OnThrottleAdd(t, &e)); if (!e.empty()) fprintf(stderr, "%s\n", e.c_str()); }

static void SameReconcile(KubeThrottler& a, KubeThrottler& b) {
  std::map<std::string, ThrottleStatus> sa, sb;
  std::string err;
  EXPECT(a.ReconcileAll(NOW, &sa, &err));
  EXPECT(b.ReconcileAll(NOW, &sb, &err));
  EXPECT(sa.size() == sb.size());
  for (auto& kv : sa) {
    auto it = sb.find(kv.first);
    EXPECT(it != sb.end());
    if (it == sb.end()) continue;
    const ThrottleStatus &x = kv.second, &y = it->second;
    EXPECT(x.UsedStrings() == y.UsedStrings());
    EXPECT(x.throttledRequests == y.throttledRequests);
    EXPECT(x.usedHasCounts == y.usedHasCounts && x.usedPod == y.usedPod && x.throttledPod == y.throttledPod);
    EXPECT(x.error == y.error && x.calculatedThresholdUpdated == y.calculatedThresholdUpdated);
  }
}

int main() {
  auto A = Make(false), B = Make(true);
  if (!A || !B) return 2;
  std::string err;
  Namespace ns{"ns1", {}};
  for (auto* k : {A.get(), B.get()}) EXPECT(k->OnNamespaceAdd(ns, &err));
  // phase 1: 16 names (cpu + r00..r14) — A holds one page, B two
  ResourceList th1{{"cpu", "2"}, {R(3), "3"}};  // cpu + r00..r13, and r14 in t2: A's first page is full
  for (int i = 0; i < 14; ++i)
    if (i != 3) th1[R(i)] = "9";
  Throttle t1 = MakeThr("t1", 10, th1), t2 = MakeThr("t2", -1, {{R(14), "5"}});
  // spec allows 1 pod, an override active at NOW allows 10: after the reconcile the calculated threshold is 10
  Throttle t3 = MakeThr("t3", 1, {});
  TemporaryThresholdOverride o;
  o.begin = "2025-01-01T00:00:00Z", o.end = "2027-01-01T00:00:00Z";
  o.threshold.hasCounts = true, o.threshold.pod = 10;
  t3.overrides.push_back(o);
  for (auto* k : {A.get(), B.get()}) Feed(*k, t1), Feed(*k, t2), Feed(*k, t3);
  for (int i = 0; i < 3; ++i) {
    Pod p = MakePod("run" + std::to_string(i), {{"cpu", "500m"}, {R(3), "1"}, {R(14), "2"}, {R(7), "1"}}, true);
    for (auto* k : {A.get(), B.get()}) Feed(*k, p);
  }
  SameReconcile(*A, *B);
  // phase 2: names r20.. first seen after the reconcile — A opens page 1 now, seeded with the count part of every status
  Throttle t4 = MakeThr("t4", -1, {{R(20), "3"}});
  for (auto* k : {A.get(), B.get()}) Feed(*k, t4);
  Pod q0 = MakePod("q0", {{R(20), "2"}, {R(25), "1"}, {"cpu", "100m"}}, false);
  Pod q1 = MakePod("q1", {{R(20), "2"}}, false);
  Pod big = MakePod("big", {{R(3), "5"}}, false);
  Pod full = MakePod("full", {{R(14), "2"}}, false);
  for (auto* k : {A.get(), B.get()}) Feed(*k, q0), Feed(*k, q1), Feed(*k, big), Feed(*k, full);
  for (const Pod* p : {&q0, &q1, &big, &full}) {
    Status sa = A->PreFilter(*p), sb = B->PreFilter(*p);
    EXPECT(Same(sa, sb));
    EXPECT(A->LastStatusOf("ns1/t4") == B->LastStatusOf("ns1/t4"));
    EXPECT(A->LastStatusOf("ns1/t3") == B->LastStatusOf("ns1/t3"));
  }
  EXPECT(A->PreFilter(q0).IsSuccess());  // t3: 3 pods used + 1 against the CALCULATED 10 (a page without its status: spec's 1)
  EXPECT(A->PreFilter(big).code == UnschedulableAndUnresolvable);
  EXPECT(!A->PreFilter(big).events.empty());
  EXPECT(A->PreFilter(full).reasons == std::vector<std::string>{"throttle[active]=ns1/t2"});
  // Reserve / Unreserve across the pages
  for (auto* k : {A.get(), B.get()}) EXPECT(k->Reserve(q0).IsSuccess());
  Status sa = A->PreFilter(q1), sb = B->PreFilter(q1);
  EXPECT(Same(sa, sb));
  EXPECT(sa.reasons == std::vector<std::string>{"throttle[insufficient]=ns1/t4"});
  for (auto* k : {A.get(), B.get()}) k->Unreserve(q0);
  EXPECT(A->PreFilter(q1).IsSuccess() && B->PreFilter(q1).IsSuccess());
  for (auto* k : {A.get(), B.get()}) EXPECT(k->Reserve(q0).IsSuccess());
  q0.nodeName = "node-1", q0.phase = "Running";
  for (auto* k : {A.get(), B.get()}) Feed(*k, q0);
  SameReconcile(*A, *B);
  // AdmitQueue on A == PreFilter + Reserve pod by pod on B
  std::vector<std::string> keys;
  for (int i = 0; i < 6; ++i) {
    Pod p = MakePod("a" + std::to_string(i), {{R(20), i % 2 ? "1" : "0"}, {"cpu", "400m"}, {R(28), "1"}}, false);
    for (auto* k : {A.get(), B.get()}) Feed(*k, p);
    keys.push_back(p.Key());
  }
  std::vector<Status> got = A->AdmitQueue(keys);
  int admitted = 0, blocked = 0;
  for (size_t i = 0; i < keys.size(); ++i) {
    Pod p = MakePod("a" + std::to_string(i), {{R(20), i % 2 ? "1" : "0"}, {"cpu", "400m"}, {R(28), "1"}}, false);
    Status want = B->PreFilter(p);
    if (want.IsSuccess()) want = B->Reserve(p);
    EXPECT(Same(got[i], want));
    admitted += got[i].IsSuccess(), blocked += !got[i].IsSuccess();
  }
  EXPECT(admitted > 0 && blocked > 0);
  SameReconcile(*A, *B);
  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
