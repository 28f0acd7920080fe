// host_plugin_preempt_elastic_gang_test — KubeThrottler::PreemptElasticGang (one kt_preempt_gangs_elastic_launch +
// kt_preempt_gangs_elastic_fetch on the mirror's engine) on plugin A against the plain calls on a twin B: per prefix length delete
// the candidates, ReconcileAll, AdmitElasticGangs of the one gang (un-reserved again where members stayed); then only the named
// victims are deleted on B, which must let the quorum in with exactly the members A reports.  The scenario is the 20 pods of
// host_plugin_preempt_test (4 pending, 16 on a node) under a Throttle (pod count and cpu) and a ClusterThrottle (amd.com/gpu).
// Every query is printed as
//     PREEMPTELASTIC <members joined by +> <quorum> <required bits | -> <list> <reprieve 0|1> -> <victims | pass | none> <blocker | -> <members in>
// for tests/test_preempt_gangs_elastic_gpu.py, which holds the lines to Engine.preempt_gangs_elastic on the same scenario written as
// manifests.  Last: the rule's defects are worded as AdmitElasticGangs words them, and a mirror that runs on two pages (20 resource
// names) answers the "pages" error.  Needs a GPU.  Exit code 0 = all expectations held.
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

struct Rule {
  int64_t quorum;
  std::vector<uint8_t> required;  // empty: none
};

static void Reconcile(KubeThrottler* k) {
  std::map<std::string, ThrottleStatus> st;
  std::string e;
  EXPECT(k->ReconcileAll(kNow, &st, &e));
}
// The gang on B as things stand there: AdmitElasticGangs of the one gang -> the members that stay (0: the rule is not met); they
// are un-reserved again
static int64_t MembersIn(const std::vector<Pod>& gang, const Rule& rule) {
  ElasticGang g;
  for (auto& p : gang) g.members.push_back(p.Key());
  g.min_members = rule.quorum, g.required = rule.required;
  const ElasticGangAdmission r = B->AdmitElasticGangs({g});
  EXPECT(r.members.size() == 1 && r.status.size() == gang.size());
  const int64_t in = r.members.empty() ? 0 : r.members[0];
  if (in > 0)
    for (size_t i = 0; i < gang.size(); ++i)
      if (r.status[i].IsSuccess()) B->Unreserve(gang[i]);
  return in;
}
// The plain way, on B: the smallest k for which the rule is met once cands[:k] are deleted and everything is reconciled; -1: none.
// The deleted pods are fed again afterwards.
static int PlainPrefix(const std::vector<Pod>& gang, const Rule& rule, const std::vector<std::string>& cands) {
  std::string e;
  int found = -1;
  size_t deleted = 0;
  for (size_t k = 0; k <= cands.size(); ++k) {
    if (k) {
      EXPECT(B->OnPodDelete(cands[k - 1], &e));
      deleted = k;
    }
    Reconcile(B);
    if (MembersIn(gang, rule) > 0) {
      found = (int)k;
      break;
    }
  }
  for (size_t j = 0; j < deleted; ++j) EXPECT(B->OnPodAdd(g_pods[cands[j]], &e));
  Reconcile(B);
  return found;
}
static int64_t MembersInWithout(const std::vector<Pod>& gang, const Rule& rule, const std::vector<std::string>& gone) {
  std::string e;
  for (auto& key : gone) EXPECT(B->OnPodDelete(key, &e));
  Reconcile(B);
  const int64_t in = MembersIn(gang, rule);
  for (auto& key : gone) EXPECT(B->OnPodAdd(g_pods[key], &e));
  Reconcile(B);
  return in;
}
// with nothing deleted, on B: the members walked in order, one that fails reserving nowhere -> the first required member that does
// not succeed, else the first member that does not ("" when everybody does); *in: how many succeed
static std::string PlainBlocker(const std::vector<Pod>& gang, const Rule& rule, int64_t* in) {
  Reconcile(B);
  std::string first, first_required;
  std::vector<const Pod*> reserved;
  for (size_t i = 0; i < gang.size(); ++i) {
    Status st = B->PreFilter(gang[i]);
    if (st.IsSuccess()) st = B->Reserve(gang[i]);
    if (st.IsSuccess()) {
      reserved.push_back(&gang[i]);
      continue;
    }
    if (first.empty()) first = gang[i].Key();
    if (first_required.empty() && !rule.required.empty() && rule.required[i]) first_required = gang[i].Key();
  }
  *in = (int64_t)reserved.size();
  for (auto* p : reserved) B->Unreserve(*p);
  return first_required.empty() ? first : first_required;
}
static ElasticGangPreemptResult Both(const std::string& list_name, const std::vector<Pod>& gang, const Rule& rule, const std::vector<std::string>& cands,
                                     bool reprieve) {
  std::vector<std::string> keys;
  std::string names, bits;
  for (auto& p : gang) keys.push_back(p.Key()), names += (names.empty() ? "" : "+") + p.name;
  for (uint8_t r : rule.required) bits += r ? "1" : "0";
  ElasticGangPreemptResult res = A->PreemptElasticGang(keys, rule.quorum, rule.required, cands, kNow, reprieve);
  const PreemptResult& got = res.preempt;
  EXPECT(got.error.empty());
  const int want = PlainPrefix(gang, rule, cands);
  std::string text;
  for (auto& v : got.victims) text += (text.empty() ? "" : ",") + v.substr(v.find('/') + 1);
  if (got.victims.empty()) text = got.none ? "none" : "pass";
  printf("PREEMPTELASTIC %s %lld %s %s %d -> %s %s %lld\n", names.c_str(), (long long)rule.quorum, bits.empty() ? "-" : bits.c_str(), list_name.c_str(),
         reprieve ? 1 : 0, text.c_str(), res.blocker.empty() ? "-" : res.blocker.substr(res.blocker.find('/') + 1).c_str(), (long long)res.members);
  EXPECT(got.none == (want < 0));
  EXPECT(!got.none || got.victims.empty());
  int64_t in0 = 0;
  const std::string blocker0 = PlainBlocker(gang, rule, &in0);
  EXPECT(res.blocker == (want == 0 ? std::string() : blocker0));
  if (want == 0) EXPECT(got.victims.empty() && res.members == in0);
  if (want < 0) EXPECT(res.members == in0);
  if (want > 0) {
    // every victim lies in the plain prefix and in the caller's order; deleting the victims alone lets exactly `members` members in
    size_t at = 0;
    for (auto& v : got.victims) {
      auto it = std::find(cands.begin() + (long)at, cands.begin() + want, v);
      EXPECT(it != cands.begin() + want);
      at = (size_t)(it - cands.begin()) + 1;
    }
    EXPECT(!got.victims.empty());
    EXPECT(res.members >= rule.quorum && MembersInWithout(gang, rule, got.victims) == res.members);
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

  const Rule one{1, {}}, both{2, {}}, second{1, {0, 1}}, first{1, {1, 0}};
  for (bool reprieve : {false, true}) {
    // the whole gang is PreemptGang's answer ...
    ElasticGangPreemptResult r = Both("down", {cpu2, gpu2}, both, down, reprieve);
    EXPECT(r.preempt.victims == A->PreemptGang({cpu2.Key(), gpu2.Key()}, down, kNow, reprieve).preempt.victims && r.members == 2);
    // ... one of the two needs fewer victims
    const size_t whole = r.preempt.victims.size();
    r = Both("down", {cpu2, gpu2}, one, down, reprieve);
    EXPECT(!r.preempt.none && r.preempt.victims.size() < whole);
    Both("up", {cpu2, gpu2}, one, up, reprieve);
    Both("up", {cpu2, gpu2}, second, up, reprieve);
    Both("down", {cpu2, gpu2}, second, down, reprieve);
    Both("up", {gpu2, cpu2}, second, up, reprieve);
    // the member that asks more than the threshold: optional it does not matter, required the rule is out of reach
    r = Both("up", {cpu2, huge}, one, up, reprieve);
    EXPECT(!r.preempt.none && r.members == 1);
    EXPECT(r.preempt.victims == A->Preempt(cpu2.Key(), up, kNow, reprieve).victims);
    r = Both("up", {cpu2, huge}, second, up, reprieve);
    EXPECT(r.preempt.none && r.blocker == huge.Key());
    r = Both("up", {huge, cpu2}, second, up, reprieve);
    EXPECT(!r.preempt.none && r.blocker == cpu2.Key());
    // no throttle affects the optional member: it is in as things stand, and that is the quorum
    r = Both("down", {cpu2, free_}, one, down, reprieve);
    EXPECT(!r.preempt.none && r.preempt.victims.empty() && r.blocker.empty() && r.members == 1);
    Both("down", {cpu2, free_}, first, down, reprieve);
  }
  // a dry run: the same question has the same answer, and A's PreFilter still blocks
  EXPECT(A->PreemptElasticGang({cpu2.Key(), gpu2.Key()}, 1, {}, up, kNow).preempt.victims == Both("up", {cpu2, gpu2}, one, up, false).preempt.victims);
  Reconcile(A);
  EXPECT(!A->PreFilter(cpu2).IsSuccess());
  // the rule's defects, worded as AdmitElasticGangs words them
  EXPECT(A->PreemptElasticGang({cpu2.Key(), gpu2.Key()}, 0, {}, up, kNow).preempt.error == "PreemptElasticGang: gang 0 asks for 0 of its 2 members");
  EXPECT(A->PreemptElasticGang({cpu2.Key(), gpu2.Key()}, 3, {}, up, kNow).preempt.error == "PreemptElasticGang: gang 0 asks for 3 of its 2 members");
  EXPECT(A->PreemptElasticGang({cpu2.Key(), gpu2.Key()}, 1, {1}, up, kNow).preempt.error ==
         "PreemptElasticGang: gang 0 has 2 members and 1 required flags");
  ElasticGang defect;
  defect.members = {cpu2.Key(), gpu2.Key()}, defect.min_members = 3;
  const ElasticGangAdmission refused = A->AdmitElasticGangs({defect});
  EXPECT(!refused.status.empty() && !refused.status[0].reasons.empty() && refused.status[0].reasons[0] == "AdmitElasticGangs: gang 0 asks for 3 of its 2 members");
  EXPECT(!A->PreemptElasticGang({"ns1/nobody"}, 1, {}, up, kNow).preempt.error.empty());
  EXPECT(!A->PreemptElasticGang({}, 1, {}, up, kNow).preempt.error.empty());
  EXPECT(!A->PreemptElasticGang({cpu2.Key()}, 1, {}, {"ns1/nobody"}, kNow).preempt.error.empty());
  EXPECT(!A->PreemptElasticGang({cpu2.Key(), cpu2.Key()}, 1, {}, up, kNow).preempt.error.empty());         // a member named twice
  EXPECT(!A->PreemptElasticGang({cpu2.Key(), "ns1/r00"}, 1, {}, up, kNow).preempt.error.empty());          // a member that is a candidate
  EXPECT(!A->PreemptElasticGang({cpu2.Key()}, 1, {}, {"ns1/r00", "ns1/r00"}, kNow).preempt.error.empty());  // a candidate named twice
  EXPECT(!A->PreemptElasticGang({cpu2.Key()}, 1, {}, up, "not-a-time").preempt.error.empty());

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
  const ElasticGangPreemptResult paged = A->PreemptElasticGang({cpu2.Key(), gpu2.Key()}, 1, {}, up, kNow);
  EXPECT(paged.preempt.error.find("pages") != std::string::npos && paged.preempt.victims.empty());

  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
