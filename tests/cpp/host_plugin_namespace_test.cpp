// host_plugin_namespace_test — Namespace events on the C++ plugin mirror.
// Plugin A LIVES through them: a Throttle and pods arrive before their Namespace object (the implicit "no object" row),
// OnNamespaceAdd afterwards, OnNamespaceAdd again with other labels (an update), OnNamespaceDelete, OnNamespaceDelete of a
// name nobody knows, the object's return.  At every checkpoint a twin B is built in one go from the state A has reached
// (Namespace objects first, then throttles, then pods).  Both must answer ReconcileAll (UsedStrings, throttledRequests,
// counts), PreFilter (codes, reasons, events, LastStatusOf) and Reserve / Unreserve alike, and A's AdmitQueue must equal
// PreFilter + Reserve pod by pod on B.  Run once with 3 resource names and once with 23 (two pages).
// Needs a GPU.  Exit code 0 = all expectations held.
#include <cstdio>
#include <string>

#include "kt_host.hpp"

using namespace kth;

static int g_fail = 0;
#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      ++g_fail;                                                       \
      fprintf(stderr, "FAIL %s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, g_where.c_str()); \
    }                                                                 \
  } while (0)

static std::string g_where;
static const char* NOW = "2026-01-01T00:00:00Z";
static std::string R(int i) { return "example.com/r" + std::to_string(100 + i).substr(1); }

static std::unique_ptr<KubeThrottler> Make() {
  PluginArgs a;
  a.name = "kube-throttler";
  a.targetSchedulerName = "my-scheduler";
  std::string err;
  auto k = NewPlugin(a, &err);
  if (!k) fprintf(stderr, "NewPlugin: %s\n", err.c_str());
  return k;
}
static Pod MakePod(const std::string& ns, const std::string& name, const ResourceList& req, bool scheduled) {
  Pod p;
  p.ns = ns;
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
static Throttle MakeThr(bool cluster, const std::string& ns, const std::string& name, int pods, const ResourceList& req) {
  Throttle t;
  t.cluster = cluster;
  t.ns = ns;
  t.name = name;
  t.throttlerName = "kube-throttler";
  if (pods >= 0) t.threshold.hasCounts = true, t.threshold.pod = pods;
  t.threshold.requests = req;
  SelectorTerm term;
  term.podSelector.matchLabels["app"] = "web";
  if (cluster) term.namespaceSelector.matchLabels["env"] = "prod";
  t.selectorTerms.push_back(term);
  return t;
}
static bool Same(const Status& a, const Status& b) {
  if (a.code != b.code || a.reasons != b.reasons || a.events.size() != b.events.size()) return false;
  for (size_t i = 0; i < a.events.size(); ++i)
    if (a.events[i].message != b.events[i].message) return false;
  return true;
}
static void Feed(KubeThrottler& k, const Namespace& n) { std::string e; EXPECT(k.OnNamespaceAdd(n, &e)); if (!e.empty()) fprintf(stderr, "%s\n", e.c_str()); }
static void Feed(KubeThrottler& k, const Pod& p) { std::string e; EXPECT(k.OnPodAdd(p, &e)); if (!e.empty()) fprintf(stderr, "%s\n", e.c_str()); }
static void Feed(KubeThrottler& k, const Throttle& t) { std::string e; EXPECT(k.OnThrottleAdd(t, &e)); if (!e.empty()) fprintf(stderr, "%s\n", e.c_str()); }

// the state A has reached: what a twin is built from in one go
struct World {
  std::map<std::string, Namespace> namespaces;  // the Namespace objects that exist
  std::vector<Throttle> throttles;
  std::vector<Pod> pods;
};

static void SameReconcile(KubeThrottler& a, KubeThrottler& b) {
  std::map<std::string, ThrottleStatus> sa, sb;
  std::string err;
  EXPECT(a.ReconcileAll(NOW, &sa, &err));
  EXPECT(b.ReconcileAll(NOW, &sb, &err));
  EXPECT(sa.size() == sb.size() && !sa.empty());
  for (auto& kv : sa) {
    auto it = sb.find(kv.first);
    EXPECT(it != sb.end());
    if (it == sb.end()) continue;
    const ThrottleStatus &x = kv.second, &y = it->second;
    EXPECT(x.UsedStrings() == y.UsedStrings());
    EXPECT(x.throttledRequests == y.throttledRequests);
    EXPECT(x.usedHasCounts == y.usedHasCounts && x.usedPod == y.usedPod && x.throttledPod == y.throttledPod);
    EXPECT(x.error == y.error);  // (calculatedThresholdUpdated is the twin's first reconcile against A's n-th: not compared)
  }
}

// A against a twin built from `w`; returns what A's PreFilter says of the pod `probe` (code and reasons as one string)
static std::string Checkpoint(KubeThrottler& A, const World& w, const std::string& where, const Pod& probe) {
  g_where = where;
  auto B = Make();
  if (!B) { ++g_fail; return ""; }
  for (auto& kv : w.namespaces) Feed(*B, kv.second);
  for (auto& t : w.throttles) Feed(*B, t);
  for (auto& p : w.pods) Feed(*B, p);
  SameReconcile(A, *B);
  std::vector<const Pod*> pending;
  for (auto& p : w.pods)
    if (p.nodeName.empty()) pending.push_back(&p);
  EXPECT(pending.size() >= 4);
  for (const Pod* p : pending) {
    Status sa = A.PreFilter(*p), sb = B->PreFilter(*p);
    EXPECT(Same(sa, sb));
    for (auto& t : w.throttles) EXPECT(A.LastStatusOf(t.Key()) == B->LastStatusOf(t.Key()));
  }
  // Reserve / Unreserve: the first pending pod reserves, the others are judged behind it, then without it again
  Status ra = A.Reserve(*pending[0]), rb = B->Reserve(*pending[0]);
  EXPECT(Same(ra, rb));
  for (const Pod* p : pending) EXPECT(Same(A.PreFilter(*p), B->PreFilter(*p)));
  A.Unreserve(*pending[0]), B->Unreserve(*pending[0]);
  for (const Pod* p : pending) EXPECT(Same(A.PreFilter(*p), B->PreFilter(*p)));
  // AdmitQueue on A == PreFilter + Reserve pod by pod on B; afterwards nothing stays reserved on either
  std::vector<std::string> keys;
  for (const Pod* p : pending) keys.push_back(p->Key());
  std::vector<Status> got = A.AdmitQueue(keys);
  EXPECT(got.size() == keys.size());
  for (size_t i = 0; i < pending.size() && i < got.size(); ++i) {
    Status want = B->PreFilter(*pending[i]);
    if (want.IsSuccess()) want = B->Reserve(*pending[i]);
    EXPECT(Same(got[i], want));
  }
  for (size_t i = 0; i < pending.size() && i < got.size(); ++i)
    if (got[i].IsSuccess()) A.Unreserve(*pending[i]), B->Unreserve(*pending[i]);
  SameReconcile(A, *B);
  Status s = A.PreFilter(probe);
  EXPECT(Same(s, B->PreFilter(probe)));
  std::string out = std::to_string((int)s.code);
  for (auto& r : s.reasons) out += " " + r;
  printf("  %-58s %s\n", where.c_str(), out.c_str());
  return out;
}

static void Run(bool wide) {
  const std::string tag = wide ? "two pages: " : "one page: ";
  auto A = Make();
  if (!A) { ++g_fail; return; }
  std::string err;
  World w;
  // requests and thresholds: 3 resource names, or 23 (cpu, memory, r00..r20: r16.. sit on the second page)
  ResourceList small{{"cpu", "300m"}, {"memory", "64Mi"}, {R(3), "1"}}, cthr{{"cpu", "1500m"}, {R(3), "3"}}, tthr{{"cpu", "1"}, {"memory", "1Gi"}};
  if (wide) {  // (r03 and r18 are full with three running pods: c-web is active on either page once it reaches "late")
    for (int i = 0; i <= 20; ++i) cthr[R(i)] = i == 3 || i == 18 ? "3" : "9";
    small[R(18)] = "1", small[R(20)] = "1";
    tthr[R(20)] = "3";
  }
  // a namespace with its object, a ClusterThrottle over env=prod, and pods there
  Namespace prod{"prod-a", {{"env", "prod"}}};
  Feed(*A, prod), w.namespaces[prod.name] = prod;
  Throttle cweb = MakeThr(true, "", "c-web", 5, cthr);
  Feed(*A, cweb), w.throttles.push_back(cweb);
  for (auto& p : {MakePod("prod-a", "a-run", small, true), MakePod("prod-a", "a-pend0", small, false), MakePod("prod-a", "a-pend1", small, false)})
    Feed(*A, p), w.pods.push_back(p);
  // a Throttle and pods of "late" arrive BEFORE its Namespace object: the implicit row without an object
  Throttle tweb = MakeThr(false, "late", "t-web", -1, tthr);
  Feed(*A, tweb), w.throttles.push_back(tweb);
  for (auto& p : {MakePod("late", "run0", small, true), MakePod("late", "run1", small, true), MakePod("late", "pend0", small, false),
                  MakePod("late", "pend1", small, false), MakePod("late", "pend2", small, false)})
    Feed(*A, p), w.pods.push_back(p);
  const Pod probe = MakePod("late", "pend0", small, false);
  const std::string no_object = Checkpoint(*A, w, tag + "a Throttle and pods before their Namespace object", probe);
  Namespace late{"late", {{"env", "prod"}}};
  Feed(*A, late), w.namespaces[late.name] = late;
  const std::string as_prod = Checkpoint(*A, w, tag + "OnNamespaceAdd afterwards (env=prod)", probe);
  late.labels["env"] = "dev";
  Feed(*A, late), w.namespaces[late.name] = late;
  const std::string as_dev = Checkpoint(*A, w, tag + "OnNamespaceAdd again with other labels (env=dev)", probe);
  EXPECT(A->OnNamespaceDelete("late", &err));
  w.namespaces.erase("late");
  const std::string deleted = Checkpoint(*A, w, tag + "OnNamespaceDelete", probe);
  EXPECT(A->OnNamespaceDelete("nobody-knows-it", &err));
  const std::string unknown = Checkpoint(*A, w, tag + "OnNamespaceDelete of an unknown name", probe);
  late.labels["env"] = "prod";
  Feed(*A, late), w.namespaces[late.name] = late;
  const std::string back = Checkpoint(*A, w, tag + "the object's return (env=prod)", probe);
  g_where = tag + "what the probe pod was told";
  EXPECT(no_object.substr(0, 1) == std::to_string((int)Error) && deleted == no_object && unknown == no_object);
  EXPECT(as_prod != no_object && as_dev != no_object && as_prod != as_dev && back == as_prod);
}

int main() {
  Run(false);
  Run(true);
  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
