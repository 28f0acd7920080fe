// host_plugin_reprieve_test — KubeThrottler::Preempt(.., reprieve = true) (one kt_preempt_reprieve_launch + kt_preempt_fetch on the
// mirror's engine) on plugin A against the walk done the plain way on a twin B: the shortest prefix by delete + ReconcileAll +
// PreFilter, then from that prefix deleted the candidates are put back one by one, the last first, each staying back when the pod
// still passes after a ReconcileAll.  The NAMES must be equal.  The scenario is that of host_plugin_preempt_test: 20 pods (4 pending,
// 16 on a node, among them a finished one, one of another scheduler and pods no throttle selects) under a Throttle (pod count and
// cpu) and a ClusterThrottle (amd.com/gpu).  Every query is printed as
//     REPRIEVE <pod> <list> -> <victim names separated by commas | pass | none>
// for tests/test_host_reprieve_gpu.py, which holds the lines to the manifest model of the same scenario.  Last: a mirror that runs
// on two pages (20 resource names) answers an error.  Needs a GPU.  Exit code 0 = all expectations held.
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
static void Gone(const std::vector<std::string>& cands, const std::vector<char>& out, bool gone) {
  std::string e;
  for (size_t j = 0; j < cands.size(); ++j)
    if (out[j]) EXPECT(gone ? B->OnPodDelete(cands[j], &e) : B->OnPodAdd(g_pods[cands[j]], &e));
}
// The plain way, on B: the victims of the walk; *prefix = the shortest prefix (-1: none).  B is as before afterwards.
static std::vector<std::string> PlainWalk(const Pod& pod, const std::vector<std::string>& cands, int* prefix) {
  std::string e;
  std::vector<char> out(cands.size(), 0);
  *prefix = -1;
  for (size_t k = 0; k <= cands.size(); ++k) {
    if (k) {
      EXPECT(B->OnPodDelete(cands[k - 1], &e));
      out[k - 1] = 1;
    }
    Reconcile(B);
    if (B->PreFilter(pod).IsSuccess()) {
      *prefix = (int)k;
      break;
    }
  }
  std::vector<std::string> victims;
  if (*prefix > 0) {
    for (int j = *prefix - 1; j >= 0; --j) {  // put c_j back: does the pod still pass?
      EXPECT(B->OnPodAdd(g_pods[cands[(size_t)j]], &e));
      Reconcile(B);
      if (B->PreFilter(pod).IsSuccess()) out[(size_t)j] = 0;
      else EXPECT(B->OnPodDelete(cands[(size_t)j], &e));
    }
    for (size_t j = 0; j < cands.size(); ++j)
      if (out[j]) victims.push_back(cands[j]);
    Gone(cands, out, false);
  } else {
    Gone(cands, out, false);
  }
  Reconcile(B);
  return victims;
}
static PreemptResult Both(const std::string& list_name, const Pod& pod, const std::vector<std::string>& cands) {
  PreemptResult got = A->Preempt(pod.Key(), cands, kNow, /*reprieve=*/true);
  PreemptResult whole = A->Preempt(pod.Key(), cands, kNow);
  EXPECT(got.error.empty() && whole.error.empty());
  int want_prefix = -1;
  const std::vector<std::string> want = PlainWalk(pod, cands, &want_prefix);
  std::string text;
  for (auto& v : got.victims) text += (text.empty() ? "" : ",") + v.substr(v.find('/') + 1);
  if (got.victims.empty()) text = got.none ? "none" : "pass";
  printf("REPRIEVE %s %s -> %s\n", pod.name.c_str(), list_name.c_str(), text.c_str());
  EXPECT(got.none == (want_prefix < 0) && got.none == whole.none);
  EXPECT(got.victims == want);
  // a subset of the prefix victims, in the caller's order, that keeps the last of them (the prefix is the shortest)
  EXPECT(std::includes(whole.victims.begin(), whole.victims.end(), got.victims.begin(), got.victims.end(),
                       [&](const std::string& x, const std::string& y) {
                         return std::find(cands.begin(), cands.end(), x) < std::find(cands.begin(), cands.end(), y);
                       }));
  if (!whole.victims.empty()) EXPECT(!got.victims.empty() && got.victims.back() == whole.victims.back());
  return got;
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

  const std::vector<std::string> web{"ns1/r03", "ns1/r07", "ns1/r11"};
  PreemptResult r = Both("up", cpu2, up);
  EXPECT(!r.none && !r.victims.empty() && r.victims.size() < A->Preempt(cpu2.Key(), up, kNow).victims.size());  // somebody is reprieved
  Both("down", cpu2, down);
  r = Both("up", gpu2, up);
  EXPECT(!r.none && !r.victims.empty());
  Both("down", gpu2, down);
  EXPECT(Both("up", huge, up).none);  // pod-requests-exceeds-threshold
  r = Both("up", free_, up);          // no throttle affects it
  EXPECT(!r.none && r.victims.empty());
  EXPECT(Both("web", cpu2, web).none);  // nobody of the list counts in a throttle of the pod
  EXPECT(Both("empty", gpu2, {}).none);
  // a dry run: the same question has the same answer, the default is the prefix query, and A's PreFilter still blocks
  EXPECT(A->Preempt(cpu2.Key(), up, kNow, true).victims == Both("up", cpu2, up).victims);
  EXPECT(A->Preempt(cpu2.Key(), up, kNow).victims == A->Preempt(cpu2.Key(), up, kNow, false).victims);
  Reconcile(A);
  EXPECT(!A->PreFilter(cpu2).IsSuccess());
  EXPECT(!A->Preempt("ns1/nobody", up, kNow, true).error.empty());
  EXPECT(!A->Preempt(cpu2.Key(), {"ns1/nobody"}, kNow, true).error.empty());
  EXPECT(!A->Preempt(cpu2.Key(), {"ns1/r00", "ns1/r00"}, kNow, true).error.empty());  // a candidate named twice
  EXPECT(!A->Preempt(cpu2.Key(), up, "not-a-time", true).error.empty());

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
  r = A->Preempt(cpu2.Key(), up, kNow, true);
  EXPECT(r.error.find("pages") != std::string::npos && r.victims.empty());

  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
