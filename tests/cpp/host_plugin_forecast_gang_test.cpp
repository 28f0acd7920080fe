// host_plugin_forecast_gang_test — KubeThrottler::RetryAfterGang (kt_override_instants, then one kt_forecast_gangs_launch +
// kt_forecast_gangs_fetch on the mirror's engine) on plugin A against the plain calls: for every instant RetryAfterGang judged, a
// FRESH twin plugin fed with the same objects, ReconcileAll at that instant and AdmitGangs of the one gang, read as a dry run —
// each instant on the state as it is, never on top of the previous one.
// The scenario is that of host_plugin_forecast_test — a Throttle on the job label (cpu 2) with a night window (22:00 - 06:00:
// cpu 10) and a freeze hour (14:00 - 15:00: cpu 500m), three running job pods (1500m together) — with a second small pending job
// pod: "small" (250m) and "small2" (300m) each pass now on their own (1750m, 1800m), the job of both does not (2050m > 2) and
// starts only with the night window.  Every query is printed as
//     RETRYGANG <members joined by +> <horizon seconds> -> <instant | never> <one verdict digit per judged instant> <blockers>
// (blockers: per judged instant the blocking member's name or -, separated by commas) for tests/test_host_forecast_gang_gpu.py,
// which holds the lines to the manifest model of the same scenario.  Last: a mirror that runs on two pages (20 resource names)
// answers an error.  Needs a GPU.  Exit code 0 = all expectations held.
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

static Throttle g_jobs;
static std::vector<Pod> g_all;

static bool Feed(KubeThrottler* k) {
  std::string err;
  Namespace ns{"ns1", {}};
  bool ok = k->OnNamespaceAdd(ns, &err) && k->OnThrottleAdd(g_jobs, &err);
  for (auto& p : g_all) ok = ok && k->OnPodAdd(p, &err);
  return ok;
}
static std::string Text(int64_t s, int32_t ns) {
  const time_t tt = (time_t)s;
  struct tm g;
  gmtime_r(&tt, &g);
  char buf[64];
  size_t n = strftime(buf, sizeof buf, "%Y-%m-%dT%H:%M:%S", &g);
  if (ns) n += (size_t)snprintf(buf + n, sizeof buf - n, ".%09d", ns);
  snprintf(buf + n, sizeof buf - n, "Z");
  return buf;
}

// RetryAfterGang on A, and the plain way per judged instant on a fresh twin
static GangRetryAfterResult Both(KubeThrottler* A, const std::vector<Pod>& gang, int64_t horizon) {
  std::vector<std::string> keys;
  std::string joined;
  for (auto& p : gang) {
    keys.push_back(p.Key());
    joined += (joined.empty() ? "" : "+") + p.name;
  }
  GangRetryAfterResult res = A->RetryAfterGang(keys, kNow, horizon);
  const RetryAfterResult& got = res.retry;
  EXPECT(got.error.empty());
  EXPECT(!got.instants.empty() && got.instants.size() == got.verdicts_at.size() && got.instants.size() == res.blockers_at.size());
  std::string digits, blockers;
  int first = -1;
  for (size_t k = 0; k < got.instants.size() && k < res.blockers_at.size(); ++k) {
    auto twin = Make();
    if (!twin) {
      ++g_fail;
      break;
    }
    EXPECT(Feed(twin.get()));
    std::map<std::string, ThrottleStatus> st;
    std::string e;
    EXPECT(twin->ReconcileAll(Text(got.instants[k].first, got.instants[k].second), &st, &e));
    const GangAdmission adm = twin->AdmitGangs({keys});
    const bool ok = adm.admitted.size() == 1 && adm.admitted[0] == 1;
    EXPECT(adm.status.size() == gang.size());
    std::string plain_blocker;  // the first member the twin does not admit: the members before it were admitted
    for (size_t j = 0; j < adm.status.size() && j < gang.size(); ++j)
      if (!adm.status[j].IsSuccess()) {
        plain_blocker = keys[j];
        break;
      }
    EXPECT(ok == plain_blocker.empty());
    EXPECT(ok == (got.verdicts_at[k] == 0));
    EXPECT(res.blockers_at[k] == plain_blocker);
    if (ok && first < 0) first = (int)k;
    digits += (char)('0' + got.verdicts_at[k]);
    std::string name = "-";
    for (auto& p : gang)
      if (p.Key() == res.blockers_at[k]) name = p.name;
    blockers += (k ? "," : "") + name;
  }
  EXPECT(got.has == (first >= 0));
  if (got.has && first >= 0) {
    EXPECT(got.instantSec == got.instants[(size_t)first].first && got.instantNsec == got.instants[(size_t)first].second);
    EXPECT(got.instant == Text(got.instantSec, got.instantNsec));
  }
  printf("RETRYGANG %s %lld -> %s %s %s\n", joined.c_str(), (long long)horizon, got.has ? got.instant.c_str() : "never", digits.c_str(),
         blockers.c_str());
  return res;
}

int main() {
  auto a = Make();
  if (!a) return 2;
  KubeThrottler* A = a.get();
  g_jobs.ns = "ns1", g_jobs.name = "jobs", g_jobs.throttlerName = "kube-throttler";
  g_jobs.threshold.requests = {{"cpu", "2"}};
  SelectorTerm jt;
  jt.podSelector.matchLabels["app"] = "job";
  g_jobs.selectorTerms.push_back(jt);
  TemporaryThresholdOverride freeze, night;
  freeze.begin = "2026-01-01T14:00:00Z", freeze.end = "2026-01-01T15:00:00Z";
  freeze.threshold.requests = {{"cpu", "500m"}};
  night.begin = "2026-01-01T22:00:00Z", night.end = "2026-01-02T06:00:00Z";
  night.threshold.requests = {{"cpu", "10"}};
  g_jobs.overrides = {freeze, night};
  for (int i = 0; i < 3; ++i) g_all.push_back(MakePod("r" + std::to_string(i), {{"app", "job"}}, {{"cpu", "500m"}}, true));
  Pod job = MakePod("job", {{"app", "job"}}, {{"cpu", "1"}}, false);        // 1500m + 1 > 2: blocked until the night window
  Pod small = MakePod("small", {{"app", "job"}}, {{"cpu", "250m"}}, false);  // passes now, not in the freeze hour
  Pod small2 = MakePod("small2", {{"app", "job"}}, {{"cpu", "300m"}}, false);  // passes now; with `small` 2050m > 2
  Pod huge = MakePod("huge", {{"app", "job"}}, {{"cpu", "20"}}, false);     // exceeds every threshold
  Pod free_ = MakePod("free", {{"app", "web"}}, {{"cpu", "1"}}, false);     // no throttle affects it
  for (const Pod& p : {job, small, small2, huge, free_}) g_all.push_back(p);
  EXPECT(Feed(A));  // A keeps the status of a cluster nobody has reconciled: the query reconciles on its own

  const int64_t day = 86400;
  // each member alone passes now ...
  EXPECT(A->RetryAfter(small.Key(), kNow, day).instant == kNow);
  EXPECT(A->RetryAfter(small2.Key(), kNow, day).instant == kNow);
  // ... the job of both only from the night window's begin, and the second member is who stops it before
  GangRetryAfterResult r = Both(A, {small, small2}, day);
  EXPECT(r.retry.has && r.retry.instant == "2026-01-01T22:00:00Z");
  // now, the freeze hour's begin and end + 1 ns, the night window's begin and end + 1 ns
  EXPECT(r.retry.instants.size() == 5 && r.retry.instants[2].second == 1 && r.retry.instants[4].second == 1);
  EXPECT(r.blockers_at.size() == 5 && r.blockers_at[0] == small2.Key() && r.blockers_at[1] == small.Key() && r.blockers_at[3].empty());
  r = Both(A, {small2, small}, day);  // the other order: the same instant, the other blocker
  EXPECT(r.retry.has && r.retry.instant == "2026-01-01T22:00:00Z" && r.blockers_at.size() == 5 && r.blockers_at[0] == small.Key());
  r = Both(A, {small, small2}, 3600);  // no boundary inside the hour: only `now` is judged
  EXPECT(!r.retry.has && r.retry.instants.size() == 1);
  r = Both(A, {small, small2}, 10 * 3600);  // (now, now + 10 h] ends at 22:00:00 exactly: the window's begin is inside
  EXPECT(r.retry.has && r.retry.instant == "2026-01-01T22:00:00Z");
  r = Both(A, {small, small2}, 10 * 3600 - 1);
  EXPECT(!r.retry.has);
  r = Both(A, {small}, day);  // a gang of one: RetryAfter's answer
  EXPECT(r.retry.has && r.retry.instant == kNow);
  r = Both(A, {small, free_}, day);  // a member no throttle affects neither is checked nor reserves
  EXPECT(r.retry.has && r.retry.instant == kNow);
  r = Both(A, {small, huge, small2}, 7 * day);
  EXPECT(!r.retry.has && r.blockers_at.size() == 5 && r.blockers_at[3] == huge.Key());
  r = Both(A, {job, small, small2}, day);
  EXPECT(r.retry.has && r.retry.instant == "2026-01-01T22:00:00Z" && r.blockers_at[0] == job.Key());
  // a dry run: the same question has the same answer, and nothing was reserved on A
  EXPECT(A->RetryAfterGang({small.Key(), small2.Key()}, kNow, day).retry.instant == "2026-01-01T22:00:00Z");
  {
    std::map<std::string, ThrottleStatus> st;
    std::string e;
    EXPECT(A->ReconcileAll(kNow, &st, &e));
  }
  EXPECT(A->PreFilter(small).IsSuccess() && A->PreFilter(small2).IsSuccess());
  // the refusals, in the mirror's own words (nothing reaches the engine)
  EXPECT(A->RetryAfterGang({small.Key(), "ns1/nobody"}, kNow, day).retry.error == "pod ns1/nobody is not known to the plugin (OnPodAdd first)");
  EXPECT(A->RetryAfterGang({small.Key(), small2.Key(), small.Key()}, kNow, day).retry.error ==
         "RetryAfterGang: pod " + small.Key() + " is a member twice");
  EXPECT(A->RetryAfterGang({}, kNow, day).retry.error == "RetryAfterGang: a gang without members");
  EXPECT(!A->RetryAfterGang({small.Key()}, "not-a-time", day).retry.error.empty());
  EXPECT(A->RetryAfterGang({small.Key()}, kNow, -1).retry.error == "RetryAfterGang: horizon -1 s");
  for (const GangRetryAfterResult& bad : {A->RetryAfterGang({small.Key(), small.Key()}, kNow, day), A->RetryAfterGang({}, kNow, day)})
    EXPECT(!bad.retry.has && bad.retry.instants.empty() && bad.retry.verdicts_at.empty() && bad.blockers_at.empty());

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
  r = A->RetryAfterGang({small.Key(), small2.Key()}, kNow, day);
  EXPECT(r.retry.error.find("pages") != std::string::npos && !r.retry.has && r.retry.verdicts_at.empty() && r.blockers_at.empty());

  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
