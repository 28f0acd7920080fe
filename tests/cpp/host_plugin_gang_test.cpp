// host_plugin_gang_test — KubeThrottler::AdmitGangs (one kt_paged_admit_gangs per segment) on plugin A against the plain calls on
// a twin B: per gang PreFilter and, on Success, Reserve for every member, then Unreserve of all members when one did not succeed.
// Scenarios: an admitted gang followed by Unreserve of one member; a rolled-back gang that leaves the reservation map without its
// members (the pod behind it in the same call fits only because of that); a gang with a repeated key, which takes the plain path,
// between two engine segments.  Needs a GPU.  Exit code 0 = all expectations held.
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

static std::unique_ptr<KubeThrottler> Make() {
  PluginArgs a;
  a.name = "kube-throttler";
  a.targetSchedulerName = "my-scheduler";
  std::string err;
  auto k = NewPlugin(a, &err);
  if (!k) fprintf(stderr, "NewPlugin: %s\n", err.c_str());
  return k;
}
static Pod MakePod(const std::string& name, const std::string& cpu) {
  Pod p;
  p.ns = "ns1";
  p.name = name;
  p.labels["app"] = "job";
  p.schedulerName = "my-scheduler";
  p.phase = "Pending";
  Container c;
  c.requests = {{"cpu", cpu}};
  p.containers.push_back(c);
  return p;
}
static bool Same(const Status& a, const Status& b) {
  if (a.code != b.code || a.reasons != b.reasons || a.events.size() != b.events.size()) return false;
  for (size_t i = 0; i < a.events.size(); ++i)
    if (a.events[i].message != b.events[i].message) return false;
  return true;
}

static KubeThrottler *A, *B;
static Pod Fed(const std::string& name, const std::string& cpu = "500m") {
  Pod p = MakePod(name, cpu);
  std::string e;
  EXPECT(A->OnPodAdd(p, &e) && B->OnPodAdd(p, &e));
  return p;
}
// the plain way, on B
static uint8_t PlainGang(const std::vector<Pod>& gang, std::vector<Status>* out) {
  bool all = true;
  for (auto& p : gang) {
    Status st = B->PreFilter(p);
    if (st.IsSuccess()) st = B->Reserve(p);
    all &= st.IsSuccess();
    out->push_back(st);
  }
  if (!all)
    for (auto& p : gang) B->Unreserve(p);
  return all ? 1 : 0;
}
// AdmitGangs on A == the plain way on B: per-pod answers and gang flags
static std::vector<uint8_t> Both(const std::vector<std::vector<Pod>>& gangs) {
  std::vector<std::vector<std::string>> keys;
  std::vector<Status> want;
  std::vector<uint8_t> want_flags;
  for (auto& g : gangs) {
    keys.emplace_back();
    for (auto& p : g) keys.back().push_back(p.Key());
    want_flags.push_back(PlainGang(g, &want));
  }
  GangAdmission got = A->AdmitGangs(keys);
  EXPECT(got.admitted == want_flags);
  EXPECT(got.status.size() == want.size());
  for (size_t i = 0; i < want.size() && i < got.status.size(); ++i) EXPECT(Same(got.status[i], want[i]));
  return got.admitted;
}
static void SameProbe(const Pod& p, bool success) {
  Status sa = A->PreFilter(p), sb = B->PreFilter(p);
  EXPECT(Same(sa, sb));
  EXPECT(sa.IsSuccess() == success);
}

int main() {
  auto a = Make(), b = Make();
  if (!a || !b) return 2;
  A = a.get(), B = b.get();
  std::string err;
  Namespace ns{"ns1", {}};
  Throttle t;  // 6 pods, 3 cpu for the pods of the job label
  t.ns = "ns1", t.name = "jobs", t.throttlerName = "kube-throttler";
  t.threshold.hasCounts = true, t.threshold.pod = 6;
  t.threshold.requests = {{"cpu", "3"}};
  SelectorTerm term;
  term.podSelector.matchLabels["app"] = "job";
  t.selectorTerms.push_back(term);
  for (auto* k : {A, B}) EXPECT(k->OnNamespaceAdd(ns, &err) && k->OnThrottleAdd(t, &err));
  std::map<std::string, ThrottleStatus> st;
  for (auto* k : {A, B}) EXPECT(k->ReconcileAll("2026-01-01T00:00:00Z", &st, &err));
  Pod p2500 = Fed("p2500", "2500m"), p3000 = Fed("p3000", "3");

  // ---- an admitted gang, then Unreserve of one member: reserved 2 pods / 1 cpu -> 1 pod / 500m
  Pod a0 = Fed("a0"), a1 = Fed("a1");
  EXPECT(Both({{a0, a1}}) == std::vector<uint8_t>{1});
  SameProbe(p2500, false);  // 1 + 2.5 > 3
  for (auto* k : {A, B}) k->Unreserve(a0);
  SameProbe(p2500, true);  // 0.5 + 2.5 = 3

  // ---- a rolled-back gang: b0..b4 reserve (6 pods / 3 cpu), b5 is blocked; the next gang of the SAME call fits only when the
  //      five are gone again, from the engine and from the reservation map
  std::vector<Pod> bs;
  for (int i = 0; i < 6; ++i) bs.push_back(Fed("b" + std::to_string(i)));
  EXPECT(Both({bs, {p2500}}) == (std::vector<uint8_t>{0, 1}));
  for (auto& p : bs) {  // not in the map: Unreserve changes nothing
    A->Unreserve(p);
    B->Unreserve(p);
  }
  SameProbe(bs[0], false);  // a1 + p2500 hold 3 cpu
  for (auto* k : {A, B}) k->Unreserve(p2500);
  SameProbe(p2500, true);
  SameProbe(p3000, false);

  // ---- a gang with a repeated key goes the plain way, between two engine segments; the last gang is rolled back
  Pod d0 = Fed("d0"), d1 = Fed("d1"), c0 = Fed("c0"), e0 = Fed("e0"), e1 = Fed("e1"), e2 = Fed("e2");
  EXPECT(Both({{d0, d1}, {c0, c0}, {e0, e1, e2}}) == (std::vector<uint8_t>{1, 1, 0}));
  SameProbe(e0, true);     // a1, d0, d1, c0: 4 pods / 2 cpu
  SameProbe(p2500, false);
  for (auto* k : {A, B}) k->Unreserve(c0);
  SameProbe(p2500, false);  // 1.5 + 2.5
  for (auto* k : {A, B}) k->Unreserve(d0);
  SameProbe(p2500, false);  // 1 + 2.5
  for (auto* k : {A, B}) k->Unreserve(d1);
  SameProbe(p2500, true);
  // a pod that is already reserved: its gang goes the plain way too
  EXPECT(Both({{a1, e0}}) == std::vector<uint8_t>{1});
  SameProbe(p2500, false);

  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
