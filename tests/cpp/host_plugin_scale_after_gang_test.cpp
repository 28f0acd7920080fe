// host_plugin_scale_after_gang_test — KubeThrottler::ScaleAfterGang (kt_override_instants, then one
// kt_headroom_forecast_gangs_launch + kt_headroom_forecast_gangs_fetch on the mirror's engine) on plugin A against the plain calls:
// for every instant ScaleAfterGang judged, a FRESH twin plugin fed with the same objects, ReconcileAll at that instant, then fresh
// replicas of the gang — per member a fresh pod of its shape through PreFilter and, on Success, Reserve, member after member, copy
// after copy — each instant on the state as it is, never on top of the previous one.  The count of whole replicas admitted is the
// instant's copies, the first member that is not admitted is the blocker, and the throttle ScaleAfterGang names blocks it.
// The scenario is that of host_plugin_scale_after_test: a Throttle on the job label (cpu 2) with a night window (22:00 - 06:00:
// cpu 10) and a freeze hour (14:00 - 15:00: cpu 500m), a second Throttle on the same label that admits 8 pods at any time, three
// running job pods (1500m together) and pending pods of several shapes.  Last: the error answers, and a mirror that runs on two
// pages (20 resource names) answers an error.  Needs a GPU.  Exit code 0 = all expectations held.
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

// ScaleAfterGang on A, and the plain way per judged instant on a fresh twin
static GangScaleAfterResult Both(KubeThrottler* A, const std::vector<Pod>& gang, int64_t want, int64_t horizon) {
  std::vector<std::string> keys;
  std::string joined;
  for (auto& p : gang) {
    keys.push_back(p.Key());
    joined += (joined.empty() ? "" : "+") + p.name;
  }
  GangScaleAfterResult res = A->ScaleAfterGang(keys, want, kNow, horizon);
  const ScaleAfterResult& got = res.scale;
  EXPECT(got.error.empty());
  EXPECT(!got.instants.empty() && got.instants.size() == got.copies_at.size() && got.instants.size() == got.limiting_at.size() &&
         got.instants.size() == res.blockers_at.size());
  int first = -1;
  std::string line;
  for (size_t k = 0; k < got.copies_at.size() && k < res.blockers_at.size(); ++k) {
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
    std::string plain_blocker;  // the first member of the first replica that is not admitted: everybody before it was
    for (; n < want && plain_blocker.empty(); ++n) {
      for (size_t j = 0; j < gang.size(); ++j) {
        Pod c = gang[j];
        c.name = gang[j].name + "-copy" + std::to_string(n);
        EXPECT(twin->OnPodAdd(c, &e));
        Status s = twin->PreFilter(c);
        if (s.IsSuccess()) s = twin->Reserve(c);
        if (!s.IsSuccess()) {
          const std::string named = got.limiting_at[k].empty() ? std::string() : twin->LastStatusOf(got.limiting_at[k]);
          named_blocks = !named.empty() && named != "not-throttled";
          plain_blocker = keys[j];
          break;
        }
      }
      if (!plain_blocker.empty()) break;
    }
    if (got.copies_at[k] != n)
      fprintf(stderr, "%s at %zu: ScaleAfterGang %lld, the plain way %lld\n", joined.c_str(), k, (long long)got.copies_at[k], (long long)n);
    EXPECT(got.copies_at[k] == n);
    EXPECT(res.blockers_at[k] == plain_blocker);
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
  printf("SCALEGANG %s x%lld %lld -> %s%s\n", joined.c_str(), (long long)want, (long long)horizon, got.found ? got.instant.c_str() : "never",
         line.c_str());
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
  g_count.ns = "ns1", g_count.name = "count", g_count.throttlerName = "kube-throttler";
  g_count.threshold.hasCounts = true, g_count.threshold.pod = 8;
  g_count.selectorTerms.push_back(jt);
  for (int i = 0; i < 3; ++i) g_all.push_back(MakePod("r" + std::to_string(i), {{"app", "job"}}, {{"cpu", "500m"}}, true));
  Pod driver = MakePod("driver", {{"app", "job"}}, {{"cpu", "2"}}, false);     // 1500m + 2 > 2 now
  Pod small = MakePod("small", {{"app", "job"}}, {{"cpu", "250m"}}, false);    // passes now on its own, not in the freeze hour
  Pod small2 = MakePod("small2", {{"app", "job"}}, {{"cpu", "300m"}}, false);  // passes now on its own; with `small` 2050m > 2
  Pod tiny = MakePod("tiny", {{"app", "job"}}, {{"cpu", "100m"}}, false);
  Pod huge = MakePod("huge", {{"app", "job"}}, {{"cpu", "20"}}, false);        // exceeds every threshold
  Pod free_ = MakePod("free", {{"app", "web"}}, {{"cpu", "1"}}, false);        // no throttle affects it
  for (const Pod& p : {driver, small, small2, tiny, huge, free_}) g_all.push_back(p);
  EXPECT(Feed(A));  // A keeps the status of a cluster nobody has reconciled: the query reconciles on its own

  const int64_t day = 86400;
  // now, the freeze hour's begin and end + 1 ns, the night window's begin and end + 1 ns.  550m per replica: none now (2050m > 2),
  // at night the count's 8 admits two replicas (3 run + 4) and the first member of the third
  GangScaleAfterResult r = Both(A, {small, small2}, 2, day);
  EXPECT(r.scale.found && r.scale.instant == "2026-01-01T22:00:00Z" && r.scale.instants.size() == 5);
  EXPECT((r.scale.copies_at == std::vector<int64_t>{0, 0, 0, 2, 0}));
  EXPECT(r.blockers_at[0] == small2.Key() && r.blockers_at[1] == small.Key() && r.blockers_at[3].empty());
  EXPECT(r.scale.limiting_at[0] == g_jobs.Key() && r.scale.limiting_at[3].empty());
  r = Both(A, {small, small2}, 3, day);
  EXPECT(!r.scale.found && r.scale.copies_at[3] == 2 && r.scale.limiting_at[3] == g_count.Key() && r.blockers_at[3] == small2.Key());
  r = Both(A, {small2, small}, 3, day);  // the other order: the same copies, the other blocker
  EXPECT(!r.scale.found && r.scale.copies_at[3] == 2 && r.blockers_at[0] == small.Key() && r.blockers_at[3] == small.Key());
  r = Both(A, {small, small2}, 2, 3600);  // no boundary inside the hour: only `now` is judged
  EXPECT(!r.scale.found && r.scale.instants.size() == 1);
  // 350m per replica: one now (1850m; the second replica's `small` would make 2200m), none in the freeze hour, two at night
  r = Both(A, {tiny, small}, 1, day);
  EXPECT(r.scale.found && r.scale.instant == kNow);
  EXPECT((r.scale.copies_at == std::vector<int64_t>{1, 0, 1, 1, 1}));
  r = Both(A, {tiny, small}, 2, day);
  EXPECT(r.scale.found && r.scale.instant == "2026-01-01T22:00:00Z" && r.scale.copies_at[0] == 1 && r.blockers_at[0] == small.Key());
  // the driver and two executors: 2550m per replica, at night (10 - 1.5) / 2.55 = 3 by cpu, the count admits one (3 run + 3)
  r = Both(A, {driver, small, small2}, 2, day);
  EXPECT(!r.scale.found && r.scale.copies_at[3] == 1 && r.scale.limiting_at[3] == g_count.Key() && r.blockers_at[0] == driver.Key());
  r = Both(A, {small}, 5, day);  // a gang of one: ScaleAfter's answer
  const ScaleAfterResult one = A->ScaleAfter(small.Key(), 5, kNow, day);
  EXPECT(r.scale.found == one.found && r.scale.instant == one.instant && r.scale.copies_at == one.copies_at && r.scale.limiting_at == one.limiting_at);
  r = Both(A, {free_, small}, 2, day);  // a member no throttle affects neither is checked nor reserves
  EXPECT(r.scale.found && r.scale.instant == kNow && r.scale.copies_at[0] == 2);
  r = Both(A, {small, huge}, 1, 7 * day);
  EXPECT(!r.scale.found && r.blockers_at[3] == huge.Key());
  // a dry run: the same question has the same answer, and nothing was reserved on A
  EXPECT(A->ScaleAfterGang({small.Key(), small2.Key()}, 2, kNow, day).scale.instant == "2026-01-01T22:00:00Z");
  {
    std::map<std::string, ThrottleStatus> st;
    std::string e;
    EXPECT(A->ReconcileAll(kNow, &st, &e));
  }
  EXPECT(A->PreFilter(small).IsSuccess() && A->PreFilter(small2).IsSuccess() && !A->PreFilter(driver).IsSuccess());
  // ---- the error answers, in the mirror's own words (nothing reaches the engine)
  EXPECT(A->ScaleAfterGang({small.Key(), "ns1/nobody"}, 1, kNow, day).scale.error == "pod ns1/nobody is not known to the plugin (OnPodAdd first)");
  EXPECT(A->ScaleAfterGang({small.Key(), small2.Key(), small.Key()}, 1, kNow, day).scale.error ==
         "ScaleAfterGang: pod " + small.Key() + " is a member twice");
  EXPECT(A->ScaleAfterGang({}, 1, kNow, day).scale.error == "ScaleAfterGang: a gang without members");
  EXPECT(A->ScaleAfterGang({small.Key()}, 0, kNow, day).scale.error == "ScaleAfterGang: want 0" && !A->ScaleAfterGang({small.Key()}, -2, kNow, day).scale.error.empty());
  EXPECT(!A->ScaleAfterGang({small.Key()}, 1, "not-a-time", day).scale.error.empty());
  EXPECT(A->ScaleAfterGang({small.Key()}, 1, kNow, -1).scale.error == "ScaleAfterGang: horizon -1 s");
  for (const GangScaleAfterResult& bad : {A->ScaleAfterGang({small.Key(), small.Key()}, 1, kNow, day), A->ScaleAfterGang({}, 1, kNow, day),
                                          A->ScaleAfterGang({small.Key()}, 0, kNow, day)})
    EXPECT(!bad.scale.found && bad.scale.instants.empty() && bad.scale.copies_at.empty() && bad.blockers_at.empty());

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
  r = A->ScaleAfterGang({small.Key(), small2.Key()}, 2, kNow, day);
  EXPECT(r.scale.error.find("pages") != std::string::npos && !r.scale.found && r.scale.copies_at.empty() && r.blockers_at.empty());

  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
