// host_plugin_scale_after_test — KubeThrottler::ScaleAfter (kt_override_instants, then one kt_headroom_forecast_launch +
// kt_headroom_forecast_fetch on the mirror's engine) on plugin A against the plain calls: for every instant ScaleAfter judged, a
// FRESH twin plugin fed with the same objects, ReconcileAll at that instant, then fresh pods of the probed pod's shape through
// PreFilter and, on Success, Reserve one after the other — each instant on the state as it is, never on top of the previous one.
// The count of those admitted is the instant's copies, and the throttle ScaleAfter names blocks the first one that is not.
// The scenario is a Throttle on the job label (cpu 2) with a night window (22:00 - 06:00: cpu 10) and a freeze hour (14:00 - 15:00:
// cpu 500m), a second Throttle on the same label that admits 8 pods at any time, three running job pods (1500m together) and
// pending pods of four shapes.  Last: the error answers, and a mirror that runs on two pages (20 resource names) answers an error.
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

static Throttle g_jobs, g_count;
static std::vector<Pod> g_all;

static bool Feed(KubeThrottler* k) {
  std::string err;
  Namespace ns{"ns1", {}};
  bool ok = k->OnNamespaceAdd(ns, &err) && k->OnThrottleAdd(g_jobs, &err) && k->OnThrottleAdd(g_count, &err);
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

// ScaleAfter on A, and the plain way per judged instant on a fresh twin
static ScaleAfterResult Both(KubeThrottler* A, const Pod& shape, int64_t want, int64_t horizon) {
  ScaleAfterResult got = A->ScaleAfter(shape.Key(), want, kNow, horizon);
  EXPECT(got.error.empty());
  EXPECT(!got.instants.empty() && got.instants.size() == got.copies_at.size() && got.instants.size() == got.limiting_at.size());
  int first = -1;
  std::string line;
  for (size_t k = 0; k < got.copies_at.size(); ++k) {
    auto twin = Make();
    if (!twin) {
      ++g_fail;
      break;
    }
    EXPECT(Feed(twin.get()));
    std::map<std::string, ThrottleStatus> st;
    std::string e;
    EXPECT(twin->ReconcileAll(Text(got.instants[k].first, got.instants[k].second), &st, &e));
    int64_t n = 0;
    bool named_blocks = false;
    for (; n < want; ++n) {
      Pod c = shape;
      c.name = "copy" + std::to_string(n);
      EXPECT(twin->OnPodAdd(c, &e));
      Status s = twin->PreFilter(c);
      if (s.IsSuccess()) s = twin->Reserve(c);
      if (!s.IsSuccess()) {
        const std::string named = got.limiting_at[k].empty() ? std::string() : twin->LastStatusOf(got.limiting_at[k]);
        named_blocks = !named.empty() && named != "not-throttled";
        break;
      }
    }
    if (got.copies_at[k] != n)
      fprintf(stderr, "%s at %zu: ScaleAfter %lld, the plain way %lld\n", shape.Key().c_str(), k, (long long)got.copies_at[k], (long long)n);
    EXPECT(got.copies_at[k] == n);
    EXPECT(got.limiting_at[k].empty() == (n == want));
    EXPECT(named_blocks == (n < want));
    if (n >= want && first < 0) first = (int)k;
    line += " " + std::to_string(got.copies_at[k]);
  }
  EXPECT(got.found == (first >= 0));
  if (got.found && first >= 0) {
    EXPECT(got.instantSec == got.instants[(size_t)first].first && got.instantNsec == got.instants[(size_t)first].second);
    EXPECT(got.instant == Text(got.instantSec, got.instantNsec));
  }
  printf("SCALE %s x%lld %lld -> %s%s\n", shape.name.c_str(), (long long)want, (long long)horizon, got.found ? got.instant.c_str() : "never",
         line.c_str());
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
  g_count.ns = "ns1", g_count.name = "count", g_count.throttlerName = "kube-throttler";
  g_count.threshold.hasCounts = true, g_count.threshold.pod = 8;
  g_count.selectorTerms.push_back(jt);
  for (int i = 0; i < 3; ++i) g_all.push_back(MakePod("r" + std::to_string(i), {{"app", "job"}}, {{"cpu", "500m"}}, true));
  Pod job = MakePod("job", {{"app", "job"}}, {{"cpu", "2"}}, false);         // 1500m + 2 > 2 now; at night (10 - 1.5) / 2 = 4 copies
  Pod small = MakePod("small", {{"app", "job"}}, {{"cpu", "250m"}}, false);  // 2 now, none in the freeze hour, at night the count's 5
  Pod huge = MakePod("huge", {{"app", "job"}}, {{"cpu", "20"}}, false);      // exceeds every threshold
  Pod free_ = MakePod("free", {{"app", "web"}}, {{"cpu", "1"}}, false);      // no throttle affects it
  for (const Pod& p : {job, small, huge, free_}) g_all.push_back(p);
  EXPECT(Feed(A));  // A keeps the status of a cluster nobody has reconciled: the query reconciles on its own

  const int64_t day = 86400;
  // now, the freeze hour's begin and end + 1 ns, the night window's begin and end + 1 ns
  ScaleAfterResult r = Both(A, job, 4, day);
  EXPECT(r.found && r.instant == "2026-01-01T22:00:00Z" && r.instants.size() == 5);
  EXPECT((r.copies_at == std::vector<int64_t>{0, 0, 0, 4, 0}));
  EXPECT(r.limiting_at[0] == g_jobs.Key() && r.limiting_at[3].empty());
  r = Both(A, job, 5, day);  // the night window admits four of them, not five
  EXPECT(!r.found && r.copies_at[3] == 4 && r.limiting_at[3] == g_jobs.Key());
  r = Both(A, job, 4, 3600);  // no boundary inside the hour: only `now` is judged
  EXPECT(!r.found && r.instants.size() == 1);
  r = Both(A, small, 2, day);
  EXPECT(r.found && r.instant == kNow);
  EXPECT((r.copies_at == std::vector<int64_t>{2, 0, 2, 2, 2}));
  r = Both(A, small, 5, day);
  EXPECT(r.found && r.instant == "2026-01-01T22:00:00Z" && r.copies_at[0] == 2 && r.limiting_at[0] == g_jobs.Key());
  r = Both(A, small, 6, day);  // 3 run: the count of 8 stops the sixth, whatever the hour
  EXPECT(!r.found && r.copies_at[3] == 5 && r.limiting_at[3] == g_count.Key());
  r = Both(A, huge, 1, 7 * day);
  EXPECT(!r.found);
  r = Both(A, free_, 40, day);
  EXPECT(r.found && r.instant == kNow && r.copies_at[0] == 40);
  // a dry run: the same question has the same answer, and A's PreFilter still blocks
  EXPECT(A->ScaleAfter(job.Key(), 4, kNow, day).instant == "2026-01-01T22:00:00Z");
  {
    std::map<std::string, ThrottleStatus> st;
    std::string e;
    EXPECT(A->ReconcileAll(kNow, &st, &e));
  }
  EXPECT(!A->PreFilter(job).IsSuccess());
  // ---- the error answers
  EXPECT(A->ScaleAfter("ns1/nobody", 1, kNow, day).error.find("is not known to the plugin") != std::string::npos);
  EXPECT(!A->ScaleAfter(job.Key(), 0, kNow, day).error.empty() && !A->ScaleAfter(job.Key(), -2, kNow, day).error.empty());
  EXPECT(A->ScaleAfter(job.Key(), 0, kNow, day).copies_at.empty());
  EXPECT(!A->ScaleAfter(job.Key(), 1, "not-a-time", day).error.empty());
  EXPECT(!A->ScaleAfter(job.Key(), 1, kNow, -1).error.empty());

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
  r = A->ScaleAfter(job.Key(), 4, kNow, day);
  EXPECT(r.error.find("pages") != std::string::npos && !r.found && r.copies_at.empty());

  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
