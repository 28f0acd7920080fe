// host_plugin_headroom_gang_test — KubeThrottler::HeadroomGang (one kt_headroom_gangs_launch + kt_headroom_gangs_fetch on the
// mirror's engine) on plugin A against the plain calls: a twin plugin fed with the same objects and reconciled at the same
// instant, to which fresh replicas of the gang (pods of the members' shapes under new names) are added and admitted with
// AdmitGangs, one gang at a time, until one is rolled back — the number admitted and the first member of the next one that is not
// Success are HeadroomGang's copies and blocker.
// The scenario: a Throttle "jobs" on the job label (cpu 4) with three running job pods (1500m together), and a Throttle "few" on
// the worker role (7 pods).  A job replica is a launcher (250m) and two workers (300m each, role worker): 850m per replica against
// 2500m of room lets two through, the second worker of the third is stopped by "jobs"; the workers alone (600m, two pods per
// replica) get three replicas through, then "few" stops the second worker.  Every query is printed as
//     HEADROOMGANG <members joined by +> <cap> -> <copies> <limiting throttle key | -> <blocker name | ->
// for tests/test_host_headroom_gang_gpu.py, which holds the lines to the manifest model of the same scenario.  Last: a mirror that
// runs on two pages (20 resource names) answers an error.  Needs a GPU.  Exit code 0 = all expectations held.
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

static const char* kNow = "2026-01-01T12:00:00Z";

static std::unique_ptr<KubeThrottler> Make() {
  PluginArgs a;
  a.name = "kube-throttler";
  a.targetSchedulerName = "my-scheduler";
  std::string err;
  auto k = NewPlugin(a, &err);
  if (!k) fprintf(stderr, "NewPlugin: %s\n", err.c_str());
  return k;
}
static Pod MakePod(const std::string& ns, const std::string& name, const Labels& labels, const ResourceList& requests, bool running) {
  Pod p;
  p.ns = ns;
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

static std::vector<Throttle> g_throttles;
static std::vector<Pod> g_all;

static bool Feed(KubeThrottler* k) {
  std::string err;
  Namespace ns{"ns1", {}};
  bool ok = k->OnNamespaceAdd(ns, &err);
  for (auto& t : g_throttles) ok = ok && k->OnThrottleAdd(t, &err);
  for (auto& p : g_all) ok = ok && k->OnPodAdd(p, &err);
  std::map<std::string, ThrottleStatus> st;
  return ok && k->ReconcileAll(kNow, &st, &err);
}

// HeadroomGang on A, and the plain way on a fresh twin: replicas under new names, AdmitGangs one gang at a time
static GangHeadroomResult Both(KubeThrottler* A, const std::vector<Pod>& gang, int64_t cap) {
  std::vector<std::string> keys;
  std::string joined;
  for (auto& p : gang) {
    keys.push_back(p.Key());
    joined += (joined.empty() ? "" : "+") + p.name;
  }
  const GangHeadroomResult res = A->HeadroomGang(keys, cap);
  EXPECT(res.headroom.error.empty());
  auto twin = Make();
  int64_t copies = 0;
  std::string plain_blocker;
  if (!twin || !Feed(twin.get())) {
    ++g_fail;
  } else {
    for (; copies < cap && plain_blocker.empty(); ++copies) {
      std::vector<std::string> replica;
      std::string err;
      for (auto& p : gang) {
        Pod c = p;
        c.name = p.name + "-replica" + std::to_string(copies);
        EXPECT(twin->OnPodAdd(c, &err));
        replica.push_back(c.Key());
      }
      const GangAdmission adm = twin->AdmitGangs({replica});
      EXPECT(adm.status.size() == gang.size() && adm.admitted.size() == 1);
      if (adm.admitted.size() == 1 && adm.admitted[0] == 1) continue;
      for (size_t j = 0; j < adm.status.size() && j < gang.size(); ++j)
        if (!adm.status[j].IsSuccess()) {  // the first member the twin does not admit: the members before it were admitted
          plain_blocker = keys[j];
          break;
        }
      EXPECT(!plain_blocker.empty());
      break;
    }
    EXPECT(res.headroom.copies == copies);
    EXPECT(res.blocker == plain_blocker);
  }
  EXPECT(res.blocker.empty() == (res.headroom.copies == cap));
  std::string name = "-";
  for (auto& p : gang)
    if (p.Key() == res.blocker) name = p.name;
  printf("HEADROOMGANG %s %lld -> %lld %s %s\n", joined.c_str(), (long long)cap, (long long)res.headroom.copies,
         res.headroom.limiting.empty() ? "-" : res.headroom.limiting.c_str(), name.c_str());
  return res;
}

int main() {
  auto a = Make();
  if (!a) return 2;
  KubeThrottler* A = a.get();
  Throttle jobs, few;
  jobs.ns = "ns1", jobs.name = "jobs", jobs.throttlerName = "kube-throttler";
  jobs.threshold.requests = {{"cpu", "4"}};
  SelectorTerm jt;
  jt.podSelector.matchLabels["app"] = "job";
  jobs.selectorTerms.push_back(jt);
  few.ns = "ns1", few.name = "few", few.throttlerName = "kube-throttler";
  few.threshold.hasCounts = true, few.threshold.pod = 7;
  SelectorTerm ft;
  ft.podSelector.matchLabels["role"] = "worker";
  few.selectorTerms.push_back(ft);
  g_throttles = {jobs, few};
  for (int i = 0; i < 3; ++i) g_all.push_back(MakePod("ns1", "r" + std::to_string(i), {{"app", "job"}}, {{"cpu", "500m"}}, true));
  Pod launcher = MakePod("ns1", "launcher", {{"app", "job"}}, {{"cpu", "250m"}}, false);
  Pod w1 = MakePod("ns1", "w1", {{"app", "job"}, {"role", "worker"}}, {{"cpu", "300m"}}, false);
  Pod w2 = MakePod("ns1", "w2", {{"app", "job"}, {"role", "worker"}}, {{"cpu", "300m"}}, false);
  Pod huge = MakePod("ns1", "huge", {{"app", "job"}}, {{"cpu", "20"}}, false);      // exceeds the threshold
  Pod free_ = MakePod("ns1", "free", {{"app", "web"}}, {{"cpu", "1"}}, false);      // no throttle affects it
  Pod ghost = MakePod("ghost", "ghost", {{"app", "job"}}, {{"cpu", "100m"}}, false);  // no Namespace object: PreFilter is an Error
  for (const Pod& p : {launcher, w1, w2, huge, free_, ghost}) g_all.push_back(p);
  EXPECT(Feed(A));

  GangHeadroomResult r = Both(A, {launcher, w1, w2}, 10);
  EXPECT(r.headroom.copies == 2 && r.headroom.limiting == jobs.Key() && r.blocker == w2.Key());
  r = Both(A, {w2, w1, launcher}, 10);  // the other order: the same number, the other blocker
  EXPECT(r.headroom.copies == 2 && r.headroom.limiting == jobs.Key() && r.blocker == launcher.Key());
  r = Both(A, {w1, w2}, 10);  // 600m and two worker pods per replica: the pod count decides
  EXPECT(r.headroom.copies == 3 && r.headroom.limiting == few.Key() && r.blocker == w2.Key());
  r = Both(A, {launcher, w1, w2}, 2);  // the cap
  EXPECT(r.headroom.copies == 2 && r.headroom.limiting.empty() && r.blocker.empty());
  r = Both(A, {launcher}, 50);  // a gang of one: Headroom's answer
  const HeadroomResult one = A->Headroom(launcher.Key(), 50);
  EXPECT(one.error.empty() && r.headroom.copies == one.copies && r.headroom.limiting == one.limiting && r.headroom.copies == 10);
  r = Both(A, {launcher, free_}, 50);  // a member no throttle affects neither is checked nor reserves
  EXPECT(r.headroom.copies == 10 && r.blocker == launcher.Key());
  r = Both(A, {launcher, huge, w1}, 10);
  EXPECT(r.headroom.copies == 0 && r.headroom.limiting == jobs.Key() && r.blocker == huge.Key());
  r = Both(A, {launcher, ghost, huge}, 10);  // the Error member is the blocker: nobody is limiting
  EXPECT(r.headroom.copies == 0 && r.headroom.limiting.empty() && r.blocker == ghost.Key());
  r = Both(A, {huge, ghost}, 10);  // ... unless a throttle stops a member in front of it
  EXPECT(r.headroom.copies == 0 && r.headroom.limiting == jobs.Key() && r.blocker == huge.Key());
  // a dry run: the same question has the same answer, and nothing was reserved on A
  EXPECT(A->HeadroomGang({launcher.Key(), w1.Key(), w2.Key()}, 10).headroom.copies == 2);
  EXPECT(A->PreFilter(launcher).IsSuccess() && A->PreFilter(w1).IsSuccess());
  // the refusals, in the mirror's own words (nothing reaches the engine) and in the engine's
  EXPECT(A->HeadroomGang({w1.Key(), "ns1/nobody"}, 10).headroom.error == "pod ns1/nobody is not known to the plugin (OnPodAdd first)");
  EXPECT(A->HeadroomGang({w1.Key(), w2.Key(), w1.Key()}, 10).headroom.error == "HeadroomGang: pod " + w1.Key() + " is a member twice");
  EXPECT(A->HeadroomGang({}, 10).headroom.error == "HeadroomGang: a gang without members");
  EXPECT(!A->HeadroomGang({w1.Key()}, 0).headroom.error.empty());
  EXPECT(!A->HeadroomGang({w1.Key()}, (int64_t)1 << 31).headroom.error.empty());

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
  std::string err;
  EXPECT(A->OnThrottleAdd(w, &err));
  r = A->HeadroomGang({launcher.Key(), w1.Key()}, 10);
  EXPECT(r.headroom.error.find("pages") != std::string::npos && r.headroom.copies == 0 && r.blocker.empty());

  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
