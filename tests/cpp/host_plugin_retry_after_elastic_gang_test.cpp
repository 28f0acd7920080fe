// host_plugin_retry_after_elastic_gang_test — KubeThrottler::RetryAfterElasticGang (kt_override_instants, then one
// kt_forecast_gangs_elastic_launch + kt_forecast_gangs_elastic_fetch on the mirror's engine) on plugin A against the plain calls: for
// every instant it judged, a FRESH twin plugin fed with the same objects, ReconcileAll at that instant and AdmitElasticGangs of the one
// gang — each instant on the state as it is, never on top of the previous one.
// The scenario is the case a throttle-major judge gets wrong.  Throttle "lead" selects app=a under cpu 5, with a night window
// (22:00 - 06:00: cpu 100); throttle "tier" selects tier=x under cpu 10; nothing runs.  m0 {app=a, tier=x}, m1 and m2 {app=b,
// tier=x} ask 6 each.  By day m0 exceeds "lead" (6 > 5) and therefore does NOT weigh on "tier": m1 passes there, m2 does not
// (12 > 10) — successes [no, yes, no].  At night m0 passes both and reserves 6 on "tier", which shuts m1 and m2 out — [yes, no, no].
// Every query is printed as
//     RETRYELASTIC <members joined by +> <min> <required digits or -> <horizon seconds> -> <instant | never> <verdict digits> <counts> <blockers>
// (counts and blockers per judged instant, separated by commas; a blocker is the member's name or -) for
// tests/test_forecast_gangs_elastic_gpu.py, which holds the lines to the engine call on the same scenario.  Then the rule defects in
// the mirror's own words, and last a mirror that runs on two pages (20 resource names) answers the "pages" error.  Needs a GPU.
// Exit code 0 = all expectations held.
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
static const char* kNight = "2026-01-01T22:00:00Z";

static std::unique_ptr<KubeThrottler> Make() {
  PluginArgs a;
  a.name = "kube-throttler";
  a.targetSchedulerName = "my-scheduler";
  std::string err;
  auto k = NewPlugin(a, &err);
  if (!k) fprintf(stderr, "NewPlugin: %s\n", err.c_str());
  return k;
}
static Pod MakePod(const std::string& name, const Labels& labels, const std::string& cpu) {
  Pod p;
  p.ns = "ns1";
  p.name = name;
  p.labels = labels;
  p.schedulerName = "my-scheduler";
  p.phase = "Pending";
  Container c;
  c.requests = {{"cpu", cpu}};
  p.containers.push_back(c);
  return p;
}

static Throttle g_lead, g_tier;
static std::vector<Pod> g_all;

static bool Feed(KubeThrottler* k) {
  std::string err;
  Namespace ns{"ns1", {}};
  bool ok = k->OnNamespaceAdd(ns, &err) && k->OnThrottleAdd(g_lead, &err) && k->OnThrottleAdd(g_tier, &err);
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

// RetryAfterElasticGang on A, and the plain way per judged instant on a fresh twin
static ElasticGangRetryAfterResult Both(KubeThrottler* A, const std::vector<Pod>& gang, int64_t min_members, const std::vector<uint8_t>& required,
                                        int64_t horizon) {
  ElasticGang eg;
  std::string joined, req_digits;
  for (auto& p : gang) {
    eg.members.push_back(p.Key());
    joined += (joined.empty() ? "" : "+") + p.name;
  }
  eg.min_members = min_members, eg.required = required;
  for (uint8_t r : required) req_digits += r ? '1' : '0';
  ElasticGangRetryAfterResult res = A->RetryAfterElasticGang(eg.members, min_members, required, kNow, horizon);
  const RetryAfterResult& got = res.retry;
  EXPECT(got.error.empty());
  const size_t m = got.instants.size();
  EXPECT(m > 0 && got.verdicts_at.size() == m && res.blockers_at.size() == m && res.members_at.size() == m);
  std::string digits, counts, blockers;
  int first = -1;
  for (size_t k = 0; k < m && res.blockers_at.size() == m && res.members_at.size() == m; ++k) {
    auto twin = Make();
    if (!twin) {
      ++g_fail;
      break;
    }
    EXPECT(Feed(twin.get()));
    std::map<std::string, ThrottleStatus> st;
    std::string e;
    EXPECT(twin->ReconcileAll(Text(got.instants[k].first, got.instants[k].second), &st, &e));
    const ElasticGangAdmission adm = twin->AdmitElasticGangs({eg});
    EXPECT(adm.status.size() == gang.size() && adm.members.size() == 1);
    int64_t succeeded = 0;
    std::string first_out, first_required_out;
    for (size_t j = 0; j < adm.status.size() && j < gang.size(); ++j) {
      if (adm.status[j].IsSuccess()) {
        ++succeeded;
        continue;
      }
      if (first_out.empty()) first_out = eg.members[j];
      if (first_required_out.empty() && !required.empty() && required[j]) first_required_out = eg.members[j];
    }
    const bool ok = adm.members.size() == 1 && adm.members[0] > 0;
    EXPECT(ok == (got.verdicts_at[k] == 0));
    EXPECT(res.members_at[k] == succeeded);
    if (ok) EXPECT(adm.members[0] == res.members_at[k]);
    EXPECT(res.blockers_at[k] == (ok ? std::string() : !first_required_out.empty() ? first_required_out : first_out));
    if (ok && first < 0) first = (int)k;
    digits += (char)('0' + got.verdicts_at[k]);
    counts += (k ? "," : "") + std::to_string(res.members_at[k]);
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
  printf("RETRYELASTIC %s %lld %s %lld -> %s %s %s %s\n", joined.c_str(), (long long)min_members, req_digits.empty() ? "-" : req_digits.c_str(),
         (long long)horizon, got.has ? got.instant.c_str() : "never", digits.c_str(), counts.c_str(), blockers.c_str());
  return res;
}

int main() {
  auto a = Make();
  if (!a) return 2;
  KubeThrottler* A = a.get();
  g_lead.ns = "ns1", g_lead.name = "lead", g_lead.throttlerName = "kube-throttler";
  g_lead.threshold.requests = {{"cpu", "5"}};
  SelectorTerm lt;
  lt.podSelector.matchLabels["app"] = "a";
  g_lead.selectorTerms.push_back(lt);
  TemporaryThresholdOverride night;
  night.begin = kNight, night.end = "2026-01-02T06:00:00Z";
  night.threshold.requests = {{"cpu", "100"}};
  g_lead.overrides = {night};
  g_tier.ns = "ns1", g_tier.name = "tier", g_tier.throttlerName = "kube-throttler";
  g_tier.threshold.requests = {{"cpu", "10"}};
  SelectorTerm tt;
  tt.podSelector.matchLabels["tier"] = "x";
  g_tier.selectorTerms.push_back(tt);
  Pod m0 = MakePod("m0", {{"app", "a"}, {"tier", "x"}}, "6");
  Pod m1 = MakePod("m1", {{"app", "b"}, {"tier", "x"}}, "6");
  Pod m2 = MakePod("m2", {{"app", "b"}, {"tier", "x"}}, "6");
  g_all = {m0, m1, m2};
  EXPECT(Feed(A));  // A keeps the status of a cluster nobody has reconciled: the query reconciles on its own

  const int64_t day = 86400;
  // the worked example: now, the night window's begin and its end + 1 ns
  ElasticGangRetryAfterResult r = Both(A, {m0, m1, m2}, 1, {}, day);  // one member fits at every instant — not the same one
  EXPECT(r.retry.has && r.retry.instant == kNow && r.retry.instants.size() == 3 && r.retry.instants[2].second == 1);
  EXPECT(r.members_at == std::vector<int64_t>({1, 1, 1}));
  r = Both(A, {m0, m1, m2}, 1, {0, 1, 0}, day);  // the override that lets the first member in shuts the required one out
  EXPECT(r.retry.has && r.retry.instant == kNow && r.retry.verdicts_at == std::vector<uint8_t>({0, 1, 0}));
  EXPECT(r.blockers_at.size() == 3 && r.blockers_at[0].empty() && r.blockers_at[1] == m1.Key());
  r = Both(A, {m0, m1, m2}, 1, {1, 0, 0}, day);  // the lead is required: only the night lets it in
  EXPECT(r.retry.has && r.retry.instant == kNight && r.blockers_at.size() == 3 && r.blockers_at[0] == m0.Key() && r.blockers_at[1].empty());
  r = Both(A, {m0, m1, m2}, 2, {}, day);  // two never fit; the blocker is m0 by day and m1 at night
  EXPECT(!r.retry.has && r.blockers_at.size() == 3 && r.blockers_at[0] == m0.Key() && r.blockers_at[1] == m1.Key());
  r = Both(A, {m1, m2, m0}, 2, {}, day);  // the other order: m1 takes "tier" first, so m0 does not fit there at night either
  EXPECT(!r.retry.has && r.members_at == std::vector<int64_t>({1, 1, 1}));
  r = Both(A, {m0, m1, m2}, 1, {1, 0, 0}, 3600);  // no boundary inside the hour: only `now` is judged
  EXPECT(!r.retry.has && r.retry.instants.size() == 1);
  r = Both(A, {m0, m1, m2}, 3, {}, day);  // the whole gang: RetryAfterGang's answer
  const GangRetryAfterResult whole = A->RetryAfterGang({m0.Key(), m1.Key(), m2.Key()}, kNow, day);
  EXPECT(whole.retry.error.empty() && r.retry.verdicts_at == whole.retry.verdicts_at && r.blockers_at == whole.blockers_at && r.retry.has == whole.retry.has);
  // a dry run: the same question has the same answer, and nothing was reserved on A
  EXPECT(A->RetryAfterElasticGang({m0.Key(), m1.Key(), m2.Key()}, 1, {1, 0, 0}, kNow, day).retry.instant == kNight);
  {
    std::map<std::string, ThrottleStatus> st;
    std::string e;
    EXPECT(A->ReconcileAll(kNow, &st, &e));
  }
  EXPECT(A->PreFilter(m1).IsSuccess() && A->PreFilter(m2).IsSuccess() && !A->PreFilter(m0).IsSuccess());

  // the rule defects and the other refusals, in the mirror's own words (nothing reaches the engine)
  const std::vector<std::string> keys = {m0.Key(), m1.Key(), m2.Key()};
  EXPECT(A->RetryAfterElasticGang(keys, 0, {}, kNow, day).retry.error == "RetryAfterElasticGang: gang 0 asks for 0 of its 3 members");
  EXPECT(A->RetryAfterElasticGang(keys, 4, {}, kNow, day).retry.error == "RetryAfterElasticGang: gang 0 asks for 4 of its 3 members");
  EXPECT(A->RetryAfterElasticGang(keys, 1, {1, 0}, kNow, day).retry.error == "RetryAfterElasticGang: gang 0 has 3 members and 2 required flags");
  EXPECT(A->RetryAfterElasticGang({}, 1, {}, kNow, day).retry.error == "RetryAfterElasticGang: a gang without members");
  EXPECT(A->RetryAfterElasticGang({m0.Key(), "ns1/nobody"}, 1, {}, kNow, day).retry.error == "pod ns1/nobody is not known to the plugin (OnPodAdd first)");
  EXPECT(A->RetryAfterElasticGang({m0.Key(), m1.Key(), m0.Key()}, 1, {}, kNow, day).retry.error ==
         "RetryAfterElasticGang: pod " + m0.Key() + " is a member twice");
  EXPECT(!A->RetryAfterElasticGang(keys, 1, {}, "not-a-time", day).retry.error.empty());
  EXPECT(A->RetryAfterElasticGang(keys, 1, {}, kNow, -1).retry.error == "RetryAfterElasticGang: horizon -1 s");
  for (const ElasticGangRetryAfterResult& bad : {A->RetryAfterElasticGang(keys, 4, {}, kNow, day), A->RetryAfterElasticGang({}, 1, {}, kNow, day)})
    EXPECT(!bad.retry.has && bad.retry.instants.empty() && bad.retry.verdicts_at.empty() && bad.blockers_at.empty() && bad.members_at.empty());

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
  r = A->RetryAfterElasticGang(keys, 1, {}, kNow, day);
  EXPECT(r.retry.error.find("pages") != std::string::npos && !r.retry.has && r.retry.verdicts_at.empty() && r.blockers_at.empty() && r.members_at.empty());

  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
