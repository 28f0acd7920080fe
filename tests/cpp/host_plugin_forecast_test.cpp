// host_plugin_forecast_test — KubeThrottler::RetryAfter (kt_override_instants, then one kt_forecast_launch + kt_forecast_fetch on the
// mirror's engine) on plugin A against the plain calls: for every instant RetryAfter judged, a FRESH twin plugin fed with the same
// objects, ReconcileAll at that instant and PreFilter — each instant on the state as it is, never on top of the previous one.
// The scenario is a Throttle on the job label (cpu 2) with a night window (22:00 - 06:00: cpu 10) and a freeze hour (14:00 - 15:00:
// cpu 500m), three running job pods (1500m together) and four pending pods.  Every query is printed as
//     RETRY <pod> <horizon seconds> -> <instant | never> <one verdict digit per judged instant>
// for tests/test_host_forecast_gpu.py, which holds the lines to the manifest model of the same scenario.  Last: a mirror that runs
// on two pages (20 resource names) answers an error.  Needs a GPU.  Exit code 0 = all expectations held.
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

// RetryAfter on A, and the plain way per judged instant on a fresh twin
static RetryAfterResult Both(KubeThrottler* A, const Pod& pod, int64_t horizon) {
  RetryAfterResult got = A->RetryAfter(pod.Key(), kNow, horizon);
  EXPECT(got.error.empty());
  EXPECT(!got.instants.empty() && got.instants.size() == got.verdicts_at.size());
  std::string digits;
  int first = -1;
  for (size_t k = 0; k < got.instants.size(); ++k) {
    auto twin = Make();
    if (!twin) {
      ++g_fail;
      break;
    }
    EXPECT(Feed(twin.get()));
    std::map<std::string, ThrottleStatus> st;
    std::string e;
    EXPECT(twin->ReconcileAll(Text(got.instants[k].first, got.instants[k].second), &st, &e));
    const bool ok = twin->PreFilter(pod).IsSuccess();
    EXPECT(ok == (got.verdicts_at[k] == 0));
    if (ok && first < 0) first = (int)k;
    digits += (char)('0' + got.verdicts_at[k]);
  }
  EXPECT(got.has == (first >= 0));
  if (got.has && first >= 0) {
    EXPECT(got.instantSec == got.instants[(size_t)first].first && got.instantNsec == got.instants[(size_t)first].second);
    EXPECT(got.instant == Text(got.instantSec, got.instantNsec));
  }
  printf("RETRY %s %lld -> %s %s\n", pod.name.c_str(), (long long)horizon, got.has ? got.instant.c_str() : "never", digits.c_str());
  return got;
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
  Pod job = MakePod("job", {{"app", "job"}}, {{"cpu", "1"}}, false);     // 1500m + 1 > 2: blocked until the night window
  Pod small = MakePod("small", {{"app", "job"}}, {{"cpu", "250m"}}, false);  // passes now, not in the freeze hour
  Pod huge = MakePod("huge", {{"app", "job"}}, {{"cpu", "20"}}, false);   // exceeds every threshold
  Pod free_ = MakePod("free", {{"app", "web"}}, {{"cpu", "1"}}, false);   // no throttle affects it
  for (const Pod& p : {job, small, huge, free_}) g_all.push_back(p);
  EXPECT(Feed(A));  // A keeps the status of a cluster nobody has reconciled: the query reconciles on its own

  const int64_t day = 86400;
  RetryAfterResult r = Both(A, job, day);
  EXPECT(r.has && r.instant == "2026-01-01T22:00:00Z");
  // now, the freeze hour's begin and end + 1 ns, the night window's begin and end + 1 ns
  EXPECT(r.instants.size() == 5 && r.instants[2].second == 1 && r.instants[4].second == 1);
  r = Both(A, job, 3600);  // no boundary inside the hour: only `now` is judged
  EXPECT(!r.has && r.instants.size() == 1);
  r = Both(A, job, 10 * 3600);  // (now, now + 10 h] ends at 22:00:00 exactly: the window's begin is inside
  EXPECT(r.has && r.instant == "2026-01-01T22:00:00Z");
  r = Both(A, job, 10 * 3600 - 1);
  EXPECT(!r.has);
  r = Both(A, small, day);
  EXPECT(r.has && r.instant == kNow);
  r = Both(A, huge, 7 * day);
  EXPECT(!r.has);
  r = Both(A, free_, day);
  EXPECT(r.has && r.instant == kNow);
  // a dry run: the same question has the same answer, and A's PreFilter still blocks
  EXPECT(A->RetryAfter(job.Key(), kNow, day).instant == "2026-01-01T22:00:00Z");
  {
    std::map<std::string, ThrottleStatus> st;
    std::string e;
    EXPECT(A->ReconcileAll(kNow, &st, &e));
  }
  EXPECT(!A->PreFilter(job).IsSuccess());
  EXPECT(!A->RetryAfter("ns1/nobody", kNow, day).error.empty());
  EXPECT(!A->RetryAfter(job.Key(), "not-a-time", day).error.empty());
  EXPECT(!A->RetryAfter(job.Key(), kNow, -1).error.empty());

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
  r = A->RetryAfter(job.Key(), kNow, day);
  EXPECT(r.error.find("pages") != std::string::npos && !r.has && r.verdicts_at.empty());

  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
