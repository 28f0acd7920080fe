"""The paged preemption query (kt_paged_preempt) pinned on the CPU.

tests/paged_preempt_reference.py (delete, oracle reconcile per page, OR of the calc_updated / error bytes, oracle check per page,
combine) is held to the manifest-level model of tests/manifest_model.py, which has no notion of dimensions or pages, on random
clusters over 40 resource names; ``paging.paged_preempt_of`` — the closed form that states the whole-threshold and whole-error
rules — is held to the reference on the same clusters and on the directed cases.  tests/test_paged_preempt_gpu.py holds the
kernels to the same reference."""
import copy
import functools

import pytest

import paged_preempt_reference as PPR
import preempt_reference as PR
import test_manifest_model as TM
from kube_throttler_amd import paging
from kube_throttler_amd.objects import ClusterState
from manifest_model import Model, calculate_threshold
from test_paged_admit_cpu import _manifest, admission_case

NOW = PPR.NOW
# picked on the CPU so that the reference alone meets the counts of test_the_cases_are_not_vacuous
SEEDS = [65, 66, 109, 110, 118, 215]
FACTOR = 3  # the thresholds of wide_cluster times 3: pending pods are blocked by a few running ones, not by their own request


@functools.lru_cache(maxsize=None)
def paged_case(seed):
    """(cs with loosened thresholds and the status written back, page snapshots, [(preemptor row, candidate rows)]) — built
    once and shared, never changed."""
    from oracle import kt_oracle
    cs, _ = admission_case(seed, kt_oracle, factor=FACTOR)
    snaps = [b.snapshot for b in cs.build_pages()]
    return cs, snaps, PR.preempt_cases(seed, snaps[0], n_cases=8)


@functools.lru_cache(maxsize=None)
def reference_answers(seed, on_equal):
    """[(prefix, reprieved victims)] per case of ``paged_case(seed)`` — computed once and shared."""
    from oracle import kt_oracle
    _, snaps, cases = paged_case(seed)
    return [PPR.reference(snaps, kt_oracle, p, cands, NOW, on_equal) for p, cands in cases]


# ---- the manifest level: pods deleted by name, every responsible throttle reconciled by the model, the status written, check ----
def model_passes_without(cs, p, deleted, on_equal) -> bool:
    work = copy.deepcopy(cs)
    gone = set(int(c) for c in deleted)
    pod = work.pods[p]
    work.pods = [q for i, q in enumerate(work.pods) if i not in gone]
    model = Model(work)
    for thr in work.throttles:
        if not model._responsible(thr):
            continue
        r = model.reconcile(thr, NOW)
        if r is None:
            continue  # a selector error: the stored status stays
        st = dict(thr.get("status") or {})
        st["used"] = _manifest(r["used"])
        if r["updated"]:  # replaced as a whole, over all names
            errored = calculate_threshold(thr.get("spec") or {}, NOW)[1]
            st["calculatedThreshold"] = {"threshold": _manifest(r["calc"]), "calculatedAt": TM.NOW_TEXT,
                                         "messages": [f"index {i}: unparsable" for i in errored]}
        st["throttled"] = {"resourceCounts": {"pod": r["throttled"][0]}, "resourceRequests": dict(r["throttled"][1])}
        thr["status"] = st
    return model.check(pod, on_equal)[0] == "allow"


def model_prefix(cs, p, cands, on_equal) -> int:
    model = Model(cs)
    if model.check(cs.pods[p], False)[0] == "error":
        return -1
    m_eff = next((j for j, c in enumerate(cands) if model.check(cs.pods[c], False)[0] == "error"), len(cands))
    return next((k for k in range(m_eff + 1) if model_passes_without(cs, p, cands[:k], on_equal)), -1)


def model_reprieve(cs, p, cands, prefix, on_equal):
    if prefix <= 0:
        return [0] * len(cands)
    victims = [int(j < prefix) for j in range(len(cands))]
    for j in range(prefix - 1, -1, -1):
        if model_passes_without(cs, p, [c for q, c in enumerate(cands) if victims[q] and q != j], on_equal):
            victims[j] = 0
    return victims


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_equals_the_manifest_model(seed):
    cs, snaps, cases = paged_case(seed)
    assert len(snaps) >= 3
    for (p, cands), (k, victims) in zip(cases, reference_answers(seed, False)):
        want = model_prefix(cs, p, cands, False)
        assert k == want, f"seed {seed} pod {p}"
        assert victims == model_reprieve(cs, p, cands, want, False), f"seed {seed} pod {p}: reprieve"


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("on_equal", [False, True])
def test_closed_form_equals_the_reference_on_wide_clusters(seed, on_equal, oracle_mod):
    _, snaps, cases = paged_case(seed)
    ctx = paging.paged_preempt_context(snaps, NOW)
    for (p, cands), (k, walked) in zip(cases, reference_answers(seed, on_equal)):
        prefix, victims = paging.paged_preempt_of(snaps, p, cands, NOW, on_equal, ctx=ctx)
        assert prefix == k, f"seed {seed} pod {p} on_equal={on_equal}"
        PPR.check_victims(snaps, oracle_mod, p, cands, prefix, victims, NOW, on_equal)
        assert paging.paged_preempt_of(snaps, p, cands, NOW, on_equal, reprieve=True, ctx=ctx) == (k, walked), f"seed {seed} pod {p}: reprieve"


@pytest.mark.parametrize("name", sorted(PPR.DIRECTED))
def test_closed_form_equals_the_reference_on_directed_cases(name, oracle_mod):
    snaps, p, cands = PPR.DIRECTED[name]()
    for on_equal in (False, True):
        want = PPR.reference(snaps, oracle_mod, p, cands, NOW, on_equal)
        prefix, victims = paging.paged_preempt_of(snaps, p, cands, NOW, on_equal)
        assert prefix == want[0], f"{name} on_equal={on_equal}"
        PPR.check_victims(snaps, oracle_mod, p, cands, prefix, victims, NOW, on_equal)
        assert paging.paged_preempt_of(snaps, p, cands, NOW, on_equal, reprieve=True) == want, f"{name} on_equal={on_equal}: reprieve"


def test_the_directed_answers(oracle_mod):
    snaps, p, cands = PPR.non_monotone()
    assert [PR.reference_prefix(s, oracle_mod, p, cands) for s in snaps] == [1, 2]  # the pages' own answers
    assert PPR.reference_prefix(snaps, oracle_mod, p, cands) == 3  # ... and not their maximum
    assert paging.paged_preempt_of(snaps, p, cands, NOW) == (3, [1, 1, 1])
    snaps, p, cands = PPR.second_page_line()
    assert paging.paged_preempt_of(snaps, p, cands, NOW)[0] == 66
    snaps, p, cands = PPR.count_only()
    assert paging.paged_preempt_of(snaps, p, cands, NOW) == (2, [1, 1, 0])
    snaps, p, cands = PPR.reprieve_across_pages()
    assert paging.paged_preempt_of(snaps, p, cands, NOW, reprieve=True) == (2, [1, 1, 0, 0])
    assert [paging.preempt_of(s, p, cands, NOW, reprieve=True) for s in snaps] == [(2, [0, 1, 0, 0]), (1, [1, 0, 0, 0])]


def whole_threshold_cluster():
    """A never-reconciled Throttle with spec.threshold {cpu: 1} and an active override {r19: 1} (r19 lies on page 1); the pending
    pod asks cpu 2 and r19 1, a running victim holds cpu 1 and r19 1.  The reconcile replaces calculatedThreshold — as a whole:
    the new one omits cpu — so the pod is stopped by r19 alone and passes once the victim is gone.  Page 0's own dry reconcile
    replaces nothing (of ITS names the override holds none and the stored threshold holds none: equal by value), so reading
    page 0's own byte would keep spec {cpu: 1} there and answer pod-requests-exceeds-threshold for every k."""
    cs = ClusterState()
    cs.add_namespace("ns0", {"kubernetes.io/metadata.name": "ns0"})
    names = {f"example.com/r{k:02d}": "0" for k in range(20)}
    for name, cpu, running in (("pending", "2", False), ("victim", "1", True)):
        spec = {"schedulerName": "my-scheduler",
                "containers": [{"name": "c", "resources": {"requests": dict(names, cpu=cpu, **{"example.com/r19": "1"})}}]}
        if running:
            spec["nodeName"] = "node-1"
        cs.add({"kind": "Pod", "metadata": {"name": name, "namespace": "ns0", "labels": {"app": "a"}}, "spec": spec,
                "status": {"phase": "Running" if running else "Pending"}})
    cs.add({"kind": "Throttle", "metadata": {"name": "thr", "namespace": "ns0"},
            "spec": {"throttlerName": "kube-throttler", "threshold": {"resourceRequests": {"cpu": "1"}},
                     "selector": {"selectorTerms": [{"podSelector": {"matchLabels": {"app": "a"}}}]},
                     "temporaryThresholdOverrides": [{"begin": "2025-12-01T00:00:00Z", "end": "2026-02-01T00:00:00Z",
                                                      "threshold": {"resourceRequests": {"example.com/r19": "1"}}}]}})
    return cs


def test_the_calculated_threshold_is_read_as_a_whole(oracle_mod):
    cs = whole_threshold_cluster()
    pages = cs.build_pages()
    snaps = [b.snapshot for b in pages]
    assert len(snaps) == 2 and "cpu" in pages[0].dims and "example.com/r19" in pages[1].dims
    updated = [int(oracle_mod.Oracle(s).reconcile(NOW, rows=PR.responsible_rows(s)).calc_updated[0]) for s in snaps]
    assert updated == [0, 1]  # the pages' own bytes disagree
    assert model_prefix(cs, 0, [1], False) == 1
    assert PPR.reference(snaps, oracle_mod, 0, [1]) == (1, [1])
    assert paging.paged_preempt_of(snaps, 0, [1], NOW) == (1, [1])
    assert paging.paged_preempt_of(snaps, 0, [1], NOW, reprieve=True) == (1, [1])
    assert paging.preempt_of(snaps[0], 0, [1], NOW)[0] == -1  # page 0 on its own byte: spec {cpu: 1} against the 2 asked


@pytest.mark.parametrize("seed", range(6))
def test_one_page_is_preempt_of(seed):
    snap = PR.preempt_cluster(seed).build_pages()[0].snapshot
    ctx, pctx = paging.preempt_context(snap, NOW), paging.paged_preempt_context([snap], NOW)
    for p, cands in PR.preempt_cases(seed, snap):
        for on_equal in (False, True):
            for reprieve in (False, True):
                assert paging.paged_preempt_of([snap], p, cands, NOW, on_equal, reprieve=reprieve, ctx=pctx) == \
                    paging.preempt_of(snap, p, cands, NOW, on_equal, ctx=ctx, reprieve=reprieve), f"seed {seed} pod {p}"
    for name, make in PR.DIRECTED.items():
        snap, p, cands = make()
        for reprieve in (False, True):
            assert paging.paged_preempt_of([snap], p, cands, NOW, reprieve=reprieve) == paging.preempt_of(snap, p, cands, NOW, reprieve=reprieve), name


def test_the_cases_are_not_vacuous(oracle_mod):
    positive = none = reprieved = across = 0
    for seed in SEEDS:
        _, snaps, cases = paged_case(seed)
        for (p, cands), (k, walked) in zip(cases, reference_answers(seed, False)):
            positive += k > 0
            none += k == -1
            reprieved += k > 0 and sum(walked) < sum(paging.paged_preempt_of(snaps, p, cands, NOW)[1])  # (the mask: held to the reference above)
            if k > 0:
                own = [PR.reference_prefix(s, oracle_mod, p, cands) for s in snaps]
                # the answer is not the maximum of the pages' own answers, or a page other than page 0 binds
                across += k != max(own) or max(own[1:]) == k > own[0]
    assert positive >= 5 and none >= 3 and reprieved >= 2 and across >= 1, (positive, none, reprieved, across)
