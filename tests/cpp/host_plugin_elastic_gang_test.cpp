// host_plugin_elastic_gang_test — KubeThrottler::AdmitElasticGangs (one kt_paged_admit_gangs_elastic per segment) on plugin A against
// the plain calls on a twin B: per gang PreFilter and, on Success, Reserve for every member, then Unreserve of all members when fewer
// than min_members succeeded or a required one did not.  The throttle names 20 resources, so the mirror runs on two pages, and the
// name that blocks (r17) lives on the second one.  Scenarios: a kept partial gang (the blocked member is not in the reservation
// map, the others are); a required member that fails (the gang is rolled back although its quorum succeeded, the gang behind it in
// the same call fits only because of that); a gang holding an already-reserved pod, which takes the plain path, between two engine
// segments, with an empty gang beside it; refused rules.  Needs a GPU.  Exit code 0 = all expectations held.
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

static std::string R(int i) { return "example.com/r" + std::to_string(100 + i).substr(1); }

static std::unique_ptr<KubeThrottler> Make() {
  PluginArgs a;
  a.name = "kube-throttler";
  a.targetSchedulerName = "my-scheduler";
  std::string err;
  auto k = NewPlugin(a, &err);
  if (!k) fprintf(stderr, "NewPlugin: %s\n", err.c_str());
  return k;
}
static Pod MakePod(const std::string& name, const ResourceList& req) {
  Pod p;
  p.ns = "ns1";
  p.name = name;
  p.labels["app"] = "job";
  p.schedulerName = "my-scheduler";
  p.phase = "Pending";
  Container c;
  c.requests = req;
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
static Pod Fed(const std::string& name, const ResourceList& req = {{"cpu", "500m"}}) {
  Pod p = MakePod(name, req);
  std::string e;
  EXPECT(A->OnPodAdd(p, &e) && B->OnPodAdd(p, &e));
  return p;
}
struct Job {
  std::vector<Pod> pods;
  int64_t min_members;
  std::vector<uint8_t> required;  // empty: none
};
// the plain way, on B
static int64_t PlainJob(const Job& job, std::vector<Status>* out) {
  int64_t n_in = 0;
  bool required_out = false;
  for (size_t i = 0; i < job.pods.size(); ++i) {
    Status st = B->PreFilter(job.pods[i]);
    if (st.IsSuccess()) st = B->Reserve(job.pods[i]);
    if (st.IsSuccess()) ++n_in;
    else if (!job.required.empty() && job.required[i]) required_out = true;
    out->push_back(st);
  }
  const bool kept = n_in >= job.min_members && !required_out;
  if (!kept)
    for (auto& p : job.pods) B->Unreserve(p);
  return kept ? n_in : 0;
}
// AdmitElasticGangs on A == the plain way on B: per-pod answers and the members that stay per gang
static std::vector<int64_t> Both(const std::vector<Job>& jobs) {
  std::vector<ElasticGang> gangs;
  std::vector<Status> want;
  std::vector<int64_t> want_members;
  for (auto& j : jobs) {
    ElasticGang g;
    for (auto& p : j.pods) g.members.push_back(p.Key());
    g.min_members = j.min_members, g.required = j.required;
    gangs.push_back(g);
    want_members.push_back(PlainJob(j, &want));
  }
  ElasticGangAdmission got = A->AdmitElasticGangs(gangs);
  EXPECT(got.members == want_members);
  EXPECT(got.status.size() == want.size());
  for (size_t i = 0; i < want.size() && i < got.status.size(); ++i) EXPECT(Same(got.status[i], want[i]));
  return got.members;
}
static void SameProbe(const Pod& p, bool success) {
  Status sa = A->PreFilter(p), sb = B->PreFilter(p);
  EXPECT(Same(sa, sb));
  EXPECT(sa.IsSuccess() == success);
}
static void UnreserveBoth(const Pod& p) {
  A->Unreserve(p);
  B->Unreserve(p);
}

int main() {
  auto a = Make(), b = Make();
  if (!a || !b) return 2;
  A = a.get(), B = b.get();
  std::string err;
  Namespace ns{"ns1", {}};
  Throttle t;  // 6 pods, 3 cpu, 4 of r17 for the pods of the job label; cpu + r00..r18 = 20 names: two pages, r17 on the second
  t.ns = "ns1", t.name = "jobs", t.throttlerName = "kube-throttler";
  t.threshold.hasCounts = true, t.threshold.pod = 6;
  t.threshold.requests = {{"cpu", "3"}};
  for (int i = 0; i < 19; ++i) t.threshold.requests[R(i)] = i == 17 ? "4" : "99";
  SelectorTerm term;
  term.podSelector.matchLabels["app"] = "job";
  t.selectorTerms.push_back(term);
  for (auto* k : {A, B}) EXPECT(k->OnNamespaceAdd(ns, &err) && k->OnThrottleAdd(t, &err));
  std::map<std::string, ThrottleStatus> st;
  for (auto* k : {A, B}) EXPECT(k->ReconcileAll("2026-01-01T00:00:00Z", &st, &err));
  Pod p2500 = Fed("p2500", {{"cpu", "2500m"}}), p3000 = Fed("p3000", {{"cpu", "3"}});

  // ---- a kept partial gang: k0, k1 (3 of r17) and k3 reserve, k2 (3 more of r17) is blocked on the second page; 3 of 4 with a
  //      quorum of 2: kept.  p2500 behind it in the same call does not fit beside 1.5 cpu
  Pod k0 = Fed("k0"), k1 = Fed("k1", {{"cpu", "500m"}, {R(17), "3"}}), k2 = Fed("k2", {{"cpu", "100m"}, {R(17), "3"}}), k3 = Fed("k3");
  EXPECT(Both({{{k0, k1, k2, k3}, 2, {}}, {{p2500}, 1, {}}}) == (std::vector<int64_t>{3, 0}));
  SameProbe(p2500, false);
  UnreserveBoth(k2);  // not in the map: nothing changes
  SameProbe(p2500, false);
  SameProbe(k2, false);  // r17: 3 + 3 > 4
  UnreserveBoth(k0);
  SameProbe(p2500, false);  // 1 + 2.5 > 3
  UnreserveBoth(k1);
  SameProbe(p2500, true);  // 0.5 + 2.5 = 3
  SameProbe(k2, true);     // r17 is free again
  UnreserveBoth(k3);
  SameProbe(p3000, true);

  // ---- a required member fails: x asks for more cpu than the threshold, m0 and m1 reserve; 2 of 3 with a quorum of 2, but x is
  //      required: rolled back.  [p2500, m2] behind it in the same call fits only when m0 and m1 are gone again
  Pod x = Fed("x", {{"cpu", "4"}}), m0 = Fed("m0"), m1 = Fed("m1"), m2 = Fed("m2");
  EXPECT(Both({{{x, m0, m1}, 2, {1, 0, 0}}, {{p2500, m2}, 2, {}}}) == (std::vector<int64_t>{0, 2}));
  UnreserveBoth(m0);  // not in the map
  UnreserveBoth(m1);
  SameProbe(m0, false);  // p2500 + m2 hold 3 cpu
  UnreserveBoth(p2500);
  SameProbe(p2500, true);  // 0.5 + 2.5 = 3
  UnreserveBoth(m2);
  SameProbe(p3000, true);
  // the same gang without the flag is kept
  EXPECT(Both({{{x, m0, m1}, 2, {}}}) == (std::vector<int64_t>{2}));
  UnreserveBoth(m0);
  UnreserveBoth(m1);
  SameProbe(p3000, true);

  // ---- refused rules: every status is an Error and nothing is reserved
  {
    ElasticGangAdmission r = A->AdmitElasticGangs({ElasticGang{{m0.Key(), m1.Key()}, 0, {}}});
    EXPECT(r.status.size() == 2 && r.status[0].code == Error && r.status[1].code == Error && r.members == std::vector<int64_t>{0});
    r = A->AdmitElasticGangs({ElasticGang{{m0.Key(), m1.Key()}, 3, {}}});
    EXPECT(r.status.size() == 2 && r.status[0].code == Error && r.members == std::vector<int64_t>{0});
    r = A->AdmitElasticGangs({ElasticGang{{m0.Key()}, 1, {}}, ElasticGang{{m1.Key(), m2.Key()}, 1, {1}}});
    EXPECT(r.status.size() == 3 && r.status[0].code == Error && r.status[2].code == Error && r.members == (std::vector<int64_t>{0, 0}));
    SameProbe(p3000, true);
  }

  // ---- r0 is already reserved: its gang takes the plain path, between two engine segments, an empty gang beside it
  Pod r0 = Fed("r0");
  for (auto* k : {A, B}) EXPECT(k->PreFilter(r0).IsSuccess() && k->Reserve(r0).IsSuccess());
  Pod d0 = Fed("d0"), d1 = Fed("d1"), c0 = Fed("c0"), cbig = Fed("cbig", {{"cpu", "2500m"}});
  Pod e0 = Fed("e0"), e1 = Fed("e1", {{"cpu", "500m"}, {R(17), "5"}}), e2 = Fed("e2"), f0 = Fed("f0"), f1 = Fed("f1"), f2 = Fed("f2");
  // [d0 d1] kept whole (3 pods / 1.5 cpu); [r0 c0 cbig] plain: r0 and c0 succeed, cbig is blocked, 2 of 3 kept (4 pods / 2 cpu); the
  // empty gang; [e0 e1 e2] needs all three, e1 asks for more r17 than the threshold: rolled back; [f0 f1 f2]: f0 and f1 fill the
  // throttle (6 pods / 3 cpu), f2 is blocked, a quorum of 1: kept with 2
  EXPECT(Both({{{d0, d1}, 2, {}}, {{r0, c0, cbig}, 2, {}}, {{}, 0, {}}, {{e0, e1, e2}, 3, {}}, {{f0, f1, f2}, 1, {0, 0, 0}}}) ==
         (std::vector<int64_t>{2, 2, 0, 0, 2}));
  SameProbe(f2, false);
  UnreserveBoth(e0);  // not in the map
  UnreserveBoth(e2);
  UnreserveBoth(cbig);
  UnreserveBoth(f2);
  SameProbe(f2, false);
  UnreserveBoth(f0);
  SameProbe(f2, true);  // 5 pods / 2.5 cpu
  for (const Pod* p : {&f1, &c0, &r0, &d0}) UnreserveBoth(*p);
  SameProbe(p2500, true);  // d1 alone: 0.5 + 2.5 = 3
  UnreserveBoth(d1);
  SameProbe(p3000, true);

  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
