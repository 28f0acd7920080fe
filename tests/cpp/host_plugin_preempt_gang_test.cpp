// host_plugin_preempt_gang_test — KubeThrottler::PreemptGang (one kt_preempt_gangs_launch + kt_preempt_gangs_fetch on the mirror's
// engine) on plugin A against the plain calls on a twin B: per prefix length delete the candidates, ReconcileAll, AdmitGangs of the
// one gang (un-reserved again when it was admitted); then only the named victims are deleted on B, which must let the gang in as
// well.  The scenario is the 20 pods of host_plugin_preempt_test (4 pending, 16 on a node) under a Throttle (pod count and cpu) and
// a ClusterThrottle (amd.com/gpu).  Every query is printed as
//     PREEMPTGANG <members joined by +> <list> -> <victim names separated by commas | pass | none> <blocking member | ->
// for tests/test_host_preempt_gang_gpu.py, which holds the lines to the manifest model of the same scenario.  Last: a mirror that
// runs on two pages (20 resource names) answers an error.  Needs a GPU.  Exit code 0 = all expectations held.
#include <algorithm>
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

static const char* kNow = "2026-01-01T00:00:00Z";

static std::unique_ptr<KubeThrottler> Make() {
  PluginArgs a;
  a.name = "kube-throttler";
  a.targetSchedulerName = "my-scheduler";
  std::string err;
  auto k = NewPlugin(a, &err);
  if (!k) fprintf(stderr, "NewPlugin: %s\n", err.c_str());
  return k;
}
static Pod MakePod(const std::string& name, const Labels& labels, const ResourceList& requests, bool running) {
  Pod p;
  p.ns = "ns1";
  p.name = name;
  p.labels = labels;
  p.schedulerName = "my-scheduler";
  p.phase = running ? "Running" : "Pending";
  if (running) p.nodeName = "node-1";
  Container c;
  c.requests = requests;
  p.containers.push_back(c);
  return p;
}

static KubeThrottler *A, *B;
static std::map<std::string, Pod> g_pods;  // by Key()

static void Reconcile(KubeThrottler* k) {
  std::map<std::string, ThrottleStatus> st;
  std::string e;
  EXPECT(k->ReconcileAll(kNow, &st, &e));
}
// The gang on B as things stand there: AdmitGangs of the one gang; an admitted gang is un-reserved again
static bool GangPasses(const std::vector<Pod>& gang) {
  std::vector<std::string> keys;
  for (auto& p : gang) keys.push_back(p.Key());
  const GangAdmission r = B->AdmitGangs({keys});
  const bool ok = r.admitted.size() == 1 && r.admitted[0] == 1;
  if (ok)
    for (auto& p : gang) B->Unreserve(p);
  return ok;
}
// The plain way, on B: the smallest k for which the gang is admitted once cands[:k] are deleted and everything is reconciled; -1:
// none.  The deleted pods are fed again afterwards.
static int PlainPrefix(const std::vector<Pod>& gang, const std::vector<std::string>& cands) {
  std::string e;
  int found = -1;
  size_t deleted = 0;
  for (size_t k = 0; k <= cands.size(); ++k) {
    if (k) {
      EXPECT(B->OnPodDelete(cands[k - 1], &e));
      deleted = k;
    }
    Reconcile(B);
    if (GangPasses(gang)) {
      found = (int)k;
      break;
    }
  }
  for (size_t j = 0; j < deleted; ++j) EXPECT(B->OnPodAdd(g_pods[cands[j]], &e));
  Reconcile(B);
  return found;
}
static bool PassesWithout(const std::vector<Pod>& gang, const std::vector<std::string>& gone) {
  std::string e;
  for (auto& key : gone) EXPECT(B->OnPodDelete(key, &e));
  Reconcile(B);
  const bool ok = GangPasses(gang);
  for (auto& key : gone) EXPECT(B->OnPodAdd(g_pods[key], &e));
  Reconcile(B);
  return ok;
}
// the first member B does not admit with nothing deleted ("" when the gang passes): the members before it were admitted
static std::string PlainBlocker(const std::vector<Pod>& gang) {
  Reconcile(B);
  std::string blocker;
  std::vector<const Pod*> reserved;
  for (auto& p : gang) {
    Status st = B->PreFilter(p);
    if (st.IsSuccess()) st = B->Reserve(p);
    if (!st.IsSuccess()) {
      blocker = p.Key();
      break;
    }
    reserved.push_back(&p);
  }
  for (auto* p : reserved) B->Unreserve(*p);
  return blocker;
}
static GangPreemptResult Both(const std::string& list_name, const std::vector<Pod>& gang, const std::vector<std::string>& cands) {
  std::vector<std::string> keys;
  std::string names;
  for (auto& p : gang) keys.push_back(p.Key()), names += (names.empty() ? "" : "+") + p.name;
  GangPreemptResult res = A->PreemptGang(keys, cands, kNow);
  const PreemptResult& got = res.preempt;
  EXPECT(got.error.empty());
  const int want = PlainPrefix(gang, cands);
  std::string text;
  for (auto& v : got.victims) text += (text.empty() ? "" : ",") + v.substr(v.find('/') + 1);
  if (got.victims.empty()) text = got.none ? "none" : "pass";
  printf("PREEMPTGANG %s %s -> %s %s\n", names.c_str(), list_name.c_str(), text.c_str(),
         res.blocker.empty() ? "-" : res.blocker.substr(res.blocker.find('/') + 1).c_str());
  EXPECT(got.none == (want < 0));
  EXPECT(!got.none || got.victims.empty());
  EXPECT(res.blocker == PlainBlocker(gang));
  EXPECT(res.blocker.empty() == (want == 0));
  if (want == 0) EXPECT(got.victims.empty());
  if (want > 0) {
    // every victim lies in the plain prefix and in the caller's order; the prefix ends with a victim (all requests are positive:
    // a shorter prefix would pass otherwise); deleting the victims alone lets the gang in
    EXPECT(!got.victims.empty() && got.victims.back() == cands[(size_t)want - 1]);
    size_t at = 0;
    for (auto& v : got.victims) {
      auto it = std::find(cands.begin() + (long)at, cands.begin() + want, v);
      EXPECT(it != cands.begin() + want);
      at = (size_t)(it - cands.begin()) + 1;
    }
    EXPECT(PassesWithout(gang, got.victims));
    if (got.victims.size() > 1) EXPECT(!PassesWithout(gang, std::vector<std::string>(got.victims.begin(), got.victims.end() - 1)));
  }
  return res;
}

int main() {
  auto a = Make(), b = Make();
  if (!a || !b) return 2;
  A = a.get(), B = b.get();
  std::string err;
  Namespace ns{"ns1", {}};
  Throttle jobs;  // 12 pods, 6 cpu for the pods of the job label
  jobs.ns = "ns1", jobs.name = "jobs", jobs.throttlerName = "kube-throttler";
  jobs.threshold.hasCounts = true, jobs.threshold.pod = 12;
  jobs.threshold.requests = {{"cpu", "6"}};
  SelectorTerm jt;
  jt.podSelector.matchLabels["app"] = "job";
  jobs.selectorTerms.push_back(jt);
  Throttle gpus;  // 4 gpus for the batch tier, in every namespace
  gpus.cluster = true, gpus.name = "gpus", gpus.throttlerName = "kube-throttler";
  gpus.threshold.requests = {{"amd.com/gpu", "4"}};
  SelectorTerm gt;
  gt.podSelector.matchLabels["tier"] = "batch";
  gpus.selectorTerms.push_back(gt);
  for (auto* k : {A, B}) EXPECT(k->OnNamespaceAdd(ns, &err) && k->OnThrottleAdd(jobs, &err) && k->OnThrottleAdd(gpus, &err));

  // 16 pods on a node: r03, r07, r11, r15 are web pods, the even ones are of the batch tier, every fourth holds a gpu; r05 has
  // finished and r10 belongs to another scheduler (neither counts)
  std::vector<Pod> all;
  std::vector<std::string> up, down;
  for (int i = 0; i < 16; ++i) {
    char name[8];
    snprintf(name, sizeof name, "r%02d", i);
    Labels l{{"app", i % 4 == 3 ? "web" : "job"}};
    if (i % 2 == 0) l["tier"] = "batch";
    ResourceList rq{{"cpu", std::to_string((i % 3 + 1) * 500) + "m"}};
    if (i % 4 == 0) rq["amd.com/gpu"] = "1";
    Pod p = MakePod(name, l, rq, true);
    if (i == 5) p.phase = "Succeeded";
    if (i == 10) p.schedulerName = "default-scheduler";
    all.push_back(p);
    up.push_back(p.Key());
  }
  down.assign(up.rbegin(), up.rend());
  Pod cpu2 = MakePod("cpu2", {{"app", "job"}}, {{"cpu", "2"}}, false);
  Pod gpu2 = MakePod("gpu2", {{"app", "job"}, {"tier", "batch"}}, {{"cpu", "500m"}, {"amd.com/gpu", "2"}}, false);
  Pod huge = MakePod("huge", {{"app", "job"}}, {{"cpu", "8"}}, false);
  Pod free_ = MakePod("free", {{"app", "web"}}, {{"cpu", "1"}}, false);
  for (const Pod& p : {cpu2, gpu2, huge, free_}) all.push_back(p);
  EXPECT(all.size() == 20);
  for (auto& p : all) {
    g_pods[p.Key()] = p;
    EXPECT(A->OnPodAdd(p, &err) && B->OnPodAdd(p, &err));
  }
  Reconcile(B);  // A keeps the status of a cluster nobody has reconciled: the query reconciles on its own

  GangPreemptResult r = Both("up", {cpu2, gpu2}, up);
  EXPECT(!r.preempt.none && r.preempt.victims.size() >= 2);
  // the members alone, for the comparison: over `down` the gang needs more victims than either of them
  const size_t alone_cpu2 = A->Preempt(cpu2.Key(), down, kNow).victims.size(), alone_gpu2 = A->Preempt(gpu2.Key(), down, kNow).victims.size();
  r = Both("down", {cpu2, gpu2}, down);
  EXPECT(!r.preempt.none && r.preempt.victims.size() > std::max(alone_cpu2, alone_gpu2));
  Both("up", {gpu2, cpu2}, up);
  Both("down", {gpu2, cpu2}, down);
  r = Both("up", {cpu2, free_}, up);  // no throttle affects the second member: the first one's answer
  EXPECT(r.preempt.victims == A->Preempt(cpu2.Key(), up, kNow).victims);
  Both("down", {cpu2, free_}, down);
  r = Both("up", {cpu2, huge}, up);  // pod-requests-exceeds-threshold of the second member
  EXPECT(r.preempt.none && r.blocker == cpu2.Key());
  EXPECT(Both("down", {cpu2, huge}, down).preempt.none);
  // a dry run: the same question has the same answer, and A's PreFilter still blocks
  EXPECT(A->PreemptGang({cpu2.Key(), gpu2.Key()}, up, kNow).preempt.victims == Both("up", {cpu2, gpu2}, up).preempt.victims);
  Reconcile(A);
  EXPECT(!A->PreFilter(cpu2).IsSuccess());
  EXPECT(!A->PreemptGang({"ns1/nobody"}, up, kNow).preempt.error.empty());
  EXPECT(!A->PreemptGang({}, up, kNow).preempt.error.empty());
  EXPECT(!A->PreemptGang({cpu2.Key()}, {"ns1/nobody"}, kNow).preempt.error.empty());
  EXPECT(!A->PreemptGang({cpu2.Key(), cpu2.Key()}, up, kNow).preempt.error.empty());       // a member named twice
  EXPECT(!A->PreemptGang({cpu2.Key(), "ns1/r00"}, up, kNow).preempt.error.empty());        // a member that is a candidate
  EXPECT(!A->PreemptGang({cpu2.Key()}, {"ns1/r00", "ns1/r00"}, kNow).preempt.error.empty());  // a candidate named twice
  EXPECT(!A->PreemptGang({cpu2.Key()}, up, "not-a-time").preempt.error.empty());

  // ---- 20 resource names open a second page: the query has no paged form and says so
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
  EXPECT(A->OnThrottleAdd(w, &err));
  r = A->PreemptGang({cpu2.Key(), gpu2.Key()}, up, kNow);
  EXPECT(r.preempt.error.find("pages") != std::string::npos && r.preempt.victims.empty());

  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
