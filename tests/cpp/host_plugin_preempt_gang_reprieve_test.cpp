// host_plugin_preempt_gang_reprieve_test — KubeThrottler::PreemptGang(.., reprieve = true) (one kt_preempt_gangs_reprieve_launch +
// kt_preempt_gangs_fetch on the mirror's engine) on plugin A against the walk done the plain way on a twin B: the shortest prefix by
// delete + ReconcileAll + AdmitGangs of the one gang, then from that prefix deleted the candidates are put back one by one, the last
// first, each staying back when the gang is still admitted after a ReconcileAll.  The NAMES must be equal.  Two scenarios of the
// directed table of tests/preempt_gangs_reprieve_reference.py, each on a pair of fresh plugins, pods named p<row>, one Throttle of
// cpu 10 over all of them:
//     gang-one-one-six               members 2 and 1 pending, 4 running beside the candidates 1, 1, 6
//     reserved-prefix-keeps-victims  members 3 and 3 pending, the candidates four running 2s
// Every query is printed as
//     GANGREPRIEVE <scenario> <walk | plain> -> <victim names separated by commas | pass | none>
// for tests/test_host_preempt_gang_reprieve_gpu.py, which holds the lines to the table.  Last: a mirror that runs on two pages (20
// resource names) answers an error.  Needs a GPU.  Exit code 0 = all expectations held.
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
static Pod MakePod(const std::string& name, const std::string& cpu, bool running) {
  Pod p;
  p.ns = "ns1";
  p.name = name;
  p.labels = {{"app", "job"}};
  p.schedulerName = "my-scheduler";
  p.phase = running ? "Running" : "Pending";
  if (running) p.nodeName = "node-1";
  Container c;
  c.requests = {{"cpu", cpu}};
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
// The gang on B as things stand there: AdmitGangs of the one gang; an admitted gang is un-reserved again
static bool GangPasses(const std::vector<Pod>& gang) {
  std::vector<std::string> keys;
  for (auto& p : gang) keys.push_back(p.Key());
  const GangAdmission r = B->AdmitGangs({keys});
  const bool ok = r.admitted.size() == 1 && r.admitted[0] == 1;
  if (ok)
    for (auto& p : gang) B->Unreserve(p);
  return ok;
}
// The plain way, on B: the victims of the walk; *prefix = the shortest prefix (-1: none).  B is as before afterwards.
static std::vector<std::string> PlainWalk(const std::vector<Pod>& gang, const std::vector<std::string>& cands, int* prefix) {
  std::string e;
  std::vector<char> out(cands.size(), 0);
  *prefix = -1;
  for (size_t k = 0; k <= cands.size(); ++k) {
    if (k) {
      EXPECT(B->OnPodDelete(cands[k - 1], &e));
      out[k - 1] = 1;
    }
    Reconcile(B);
    if (GangPasses(gang)) {
      *prefix = (int)k;
      break;
    }
  }
  std::vector<std::string> victims;
  if (*prefix > 0) {
    for (int j = *prefix - 1; j >= 0; --j) {  // put c_j back: is the gang still admitted?
      EXPECT(B->OnPodAdd(g_pods[cands[(size_t)j]], &e));
      Reconcile(B);
      if (GangPasses(gang)) out[(size_t)j] = 0;
      else EXPECT(B->OnPodDelete(cands[(size_t)j], &e));
    }
    for (size_t j = 0; j < cands.size(); ++j)
      if (out[j]) victims.push_back(cands[j]);
  }
  for (size_t j = 0; j < cands.size(); ++j)
    if (out[j]) EXPECT(B->OnPodAdd(g_pods[cands[j]], &e));
  Reconcile(B);
  return victims;
}
static std::string Names(const PreemptResult& r) {
  std::string text;
  for (auto& v : r.victims) text += (text.empty() ? "" : ",") + v.substr(v.find('/') + 1);
  if (r.victims.empty()) text = r.none ? "none" : "pass";
  return text;
}

// pods p0 .. p<n-1> with the given cpu, the first `pending` of them pending: the gang; the candidates are `cands` (rows)
static GangPreemptResult Scenario(const char* name, const std::vector<const char*>& cpu, size_t pending, const std::vector<int>& cands,
                                  std::vector<Pod>* gang_out = nullptr, std::vector<std::string>* cands_out = nullptr) {
  auto a = Make(), b = Make();
  GangPreemptResult none;
  if (!a || !b) {
    ++g_fail;
    return none;
  }
  A = a.get(), B = b.get();
  g_pods.clear();
  std::string err;
  Namespace ns{"ns1", {}};
  Throttle line;  // 10 cpu for the pods of the job label
  line.ns = "ns1", line.name = "line", line.throttlerName = "kube-throttler";
  line.threshold.requests = {{"cpu", "10"}};
  SelectorTerm t;
  t.podSelector.matchLabels["app"] = "job";
  line.selectorTerms.push_back(t);
  for (auto* k : {A, B}) EXPECT(k->OnNamespaceAdd(ns, &err) && k->OnThrottleAdd(line, &err));
  std::vector<Pod> all, gang;
  for (size_t i = 0; i < cpu.size(); ++i) {
    Pod p = MakePod("p" + std::to_string(i), cpu[i], i >= pending);
    all.push_back(p);
    if (i < pending) gang.push_back(p);
    g_pods[p.Key()] = p;
    EXPECT(A->OnPodAdd(p, &err) && B->OnPodAdd(p, &err));
  }
  Reconcile(B);  // A keeps the status of a cluster nobody has reconciled: the query reconciles on its own
  std::vector<std::string> keys, list;
  for (auto& p : gang) keys.push_back(p.Key());
  for (int c : cands) list.push_back(all[(size_t)c].Key());

  GangPreemptResult got = A->PreemptGang(keys, list, kNow, /*reprieve=*/true);
  GangPreemptResult whole = A->PreemptGang(keys, list, kNow);
  EXPECT(got.preempt.error.empty() && whole.preempt.error.empty());
  printf("GANGREPRIEVE %s walk -> %s\n", name, Names(got.preempt).c_str());
  printf("GANGREPRIEVE %s plain -> %s\n", name, Names(whole.preempt).c_str());
  int want_prefix = -1;
  const std::vector<std::string> want = PlainWalk(gang, list, &want_prefix);
  EXPECT(got.preempt.none == (want_prefix < 0) && got.preempt.none == whole.preempt.none);
  EXPECT(got.preempt.victims == want);
  EXPECT(got.blocker == whole.blocker);
  // the default is the prefix query: every candidate of the plain prefix that counts, whatever flag is spelled out
  EXPECT(whole.preempt.victims == A->PreemptGang(keys, list, kNow, false).preempt.victims);
  EXPECT(want_prefix <= 0 || whole.preempt.victims == std::vector<std::string>(list.begin(), list.begin() + want_prefix));
  // a subset of the prefix victims, in the caller's order, that keeps the last of them (the prefix is the shortest)
  EXPECT(std::includes(whole.preempt.victims.begin(), whole.preempt.victims.end(), got.preempt.victims.begin(), got.preempt.victims.end(),
                       [&](const std::string& x, const std::string& y) {
                         return std::find(list.begin(), list.end(), x) < std::find(list.begin(), list.end(), y);
                       }));
  if (!whole.preempt.victims.empty()) EXPECT(!got.preempt.victims.empty() && got.preempt.victims.back() == whole.preempt.victims.back());
  // a dry run: the same question has the same answer
  EXPECT(A->PreemptGang(keys, list, kNow, true).preempt.victims == got.preempt.victims);
  if (gang_out) *gang_out = gang;
  if (cands_out) *cands_out = list;

  if (gang_out) {  // the last scenario: the members alone, the refusals and the paged mirror, while A and B are alive
    for (auto& p : gang) {
      const PreemptResult alone = A->Preempt(p.Key(), list, kNow, /*reprieve=*/true);
      printf("GANGREPRIEVE %s alone-%s -> %s\n", name, p.name.c_str(), Names(alone).c_str());
    }
    EXPECT(!A->PreemptGang({"ns1/nobody"}, list, kNow, true).preempt.error.empty());
    EXPECT(!A->PreemptGang({}, list, kNow, true).preempt.error.empty());
    EXPECT(!A->PreemptGang(keys, {"ns1/nobody"}, kNow, true).preempt.error.empty());
    EXPECT(!A->PreemptGang({keys[0], keys[0]}, list, kNow, true).preempt.error.empty());     // a member named twice
    EXPECT(!A->PreemptGang({keys[0], list[0]}, list, kNow, true).preempt.error.empty());     // a member that is a candidate
    EXPECT(!A->PreemptGang(keys, {list[0], list[0]}, kNow, true).preempt.error.empty());     // a candidate named twice
    EXPECT(!A->PreemptGang(keys, list, "not-a-time", true).preempt.error.empty());
    // ---- 20 resource names open a second page: the query has no paged form and says so
    Throttle w;
    w.ns = "ns1", w.name = "wide", w.throttlerName = "kube-throttler";
    for (int i = 0; i < 20; ++i) {
      char rn[32];
      snprintf(rn, sizeof rn, "example.com/r%02d", i);
      w.threshold.requests[rn] = "10";
    }
    SelectorTerm wt;
    wt.podSelector.matchLabels["app"] = "wide";
    w.selectorTerms.push_back(wt);
    EXPECT(A->OnThrottleAdd(w, &err));
    const GangPreemptResult r = A->PreemptGang(keys, list, kNow, true);
    EXPECT(r.preempt.error.find("pages") != std::string::npos && r.preempt.victims.empty());
  }
  A = B = nullptr;
  return got;
}

int main() {
  GangPreemptResult r = Scenario("gang-one-one-six", {"2", "1", "4", "1", "1", "6"}, 2, {3, 4, 5});
  EXPECT(r.preempt.victims == std::vector<std::string>{"ns1/p5"});
  std::vector<Pod> gang;
  std::vector<std::string> list;
  r = Scenario("reserved-prefix-keeps-victims", {"3", "3", "2", "2", "2", "2"}, 2, {2, 3, 4, 5}, &gang, &list);
  EXPECT((r.preempt.victims == std::vector<std::string>{"ns1/p2", "ns1/p3"}));

  if (g_fail) {
    printf("%d expectation(s) failed\n", g_fail);
    return 1;
  }
  printf("all expectations held\n");
  return 0;
}
