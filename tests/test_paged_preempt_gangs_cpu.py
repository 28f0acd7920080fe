"""The paged gang preemption query (kt_paged_preempt_gangs) pinned on the CPU.

tests/paged_preempt_gangs_reference.py (delete, oracle reconcile per page, OR of the calc_updated / error bytes, then the members
in order: oracle check per page, combine, and on Success the reservation on every page) is held to the manifest-level model of
tests/manifest_model.py, which has no notion of dimensions or pages, on random clusters over 40 resource names;
``paging.paged_preempt_gangs_of`` — the closed form that states the rules pages add — is held to the reference on the same
clusters and on the directed cases, whose answers are written out.  tests/test_paged_preempt_gangs_gpu.py holds the kernels to the
same reference."""
import copy
import functools

import pytest

import paged_preempt_gangs_reference as PGR
import paged_preempt_reference as PPR
import preempt_gangs_reference as GR
import preempt_gangs_reprieve_reference as GRR
import preempt_reference as PR
import test_manifest_model as TM
from kube_throttler_amd import paging
from manifest_model import Model, calculate_threshold
from test_paged_admit_cpu import _manifest, admission_case, reserve
from test_paged_preempt_cpu import whole_threshold_cluster

NOW, NONE = PGR.NOW, PGR.NONE
# Picked on the CPU, in a search of seeds 0 .. 299 at the factors 2, 3, 4, 5, 6 and 8, so that the reference alone meets the counts of
# test_the_cases_are_not_vacuous in full.  (seed, factor): the thresholds of wide_cluster times ``factor`` — at 3, the factor of
# test_paged_preempt_cpu, no gang of 300 seeds needed more victims than its members do alone; at 8 a few running pods block a gang
# that its members, one by one, would pass.
CASES = [(18, 8), (38, 8), (65, 8), (137, 8)]


@functools.lru_cache(maxsize=None)
def paged_gang_case(seed, factor):
    """(cs with loosened thresholds and the status written back, page snapshots, [(member rows, candidate rows)]) — built once and
    shared, never changed."""
    from oracle import kt_oracle
    cs, _ = admission_case(seed, kt_oracle, factor=factor)
    snaps = [b.snapshot for b in cs.build_pages()]
    return cs, snaps, PGR.gang_cases(seed, snaps[0])


@functools.lru_cache(maxsize=None)
def reference_answers(seed, factor, on_equal):
    """[(prefix, reprieved victims, blocker)] per case of ``paged_gang_case`` — computed once and shared."""
    from oracle import kt_oracle
    _, snaps, cases = paged_gang_case(seed, factor)
    return [PGR.reference(snaps, kt_oracle, ms, cands, NOW, on_equal) for ms, cands in cases]


# ---- the manifest level: pods deleted by name, every responsible throttle reconciled by the model, the status written, then the
#      members admitted in order with Reserve (test_paged_admit_cpu.model_admit's steps) ----
def model_first_blocked(cs, members, deleted, on_equal):
    work = copy.deepcopy(cs)
    gone = set(int(c) for c in deleted)
    pods = [work.pods[p] for p in members]
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
    for j, pod in enumerate(pods):
        v, st = model.check(pod, on_equal)
        if v != "allow":
            return j
        reserve(work, st, pod)
    return None


def model_answer(cs, members, cands, on_equal):
    """-> (prefix, reprieved victims, blocker) at the manifest level."""
    model = Model(cs)
    blocker = model_first_blocked(cs, members, [], on_equal)
    ok = all(model.check(cs.pods[p], False)[0] != "error" for p in members)
    prefix = NONE
    if blocker is None:
        prefix, blocker = (0 if ok else NONE), -1
    elif ok:
        m_eff = next((j for j, c in enumerate(cands) if model.check(cs.pods[c], False)[0] == "error"), len(cands))
        prefix = next((k for k in range(1, m_eff + 1) if model_first_blocked(cs, members, cands[:k], on_equal) is None), NONE)
    victims = [int(j < prefix) for j in range(len(cands))]
    for j in range(prefix - 1, -1, -1):
        if model_first_blocked(cs, members, [c for q, c in enumerate(cands) if victims[q] and q != j], on_equal) is None:
            victims[j] = 0
    return prefix, victims, blocker


@pytest.mark.parametrize("seed,factor", CASES)
def test_reference_equals_the_manifest_model(seed, factor):
    cs, snaps, cases = paged_gang_case(seed, factor)
    assert len(snaps) >= 3
    for (ms, cands), got in zip(cases, reference_answers(seed, factor, False)):
        assert got == model_answer(cs, ms, cands, False), f"seed {seed} gang {ms}"


@pytest.mark.parametrize("seed,factor", CASES)
@pytest.mark.parametrize("on_equal", [False, True])
def test_closed_form_equals_the_reference_on_wide_clusters(seed, factor, on_equal, oracle_mod):
    _, snaps, cases = paged_gang_case(seed, factor)
    ctx = paging.paged_preempt_context(snaps, NOW)
    for (ms, cands), (k, walked, blocker) in zip(cases, reference_answers(seed, factor, on_equal)):
        prefix, victims, b = paging.paged_preempt_gangs_of(snaps, ms, cands, NOW, on_equal, ctx=ctx)
        assert (prefix, b) == (k, blocker), f"seed {seed} gang {ms} on_equal={on_equal}"
        PGR.check_victims(snaps, oracle_mod, ms, cands, prefix, victims, NOW, on_equal)
        assert paging.paged_preempt_gangs_of(snaps, ms, cands, NOW, on_equal, reprieve=True, ctx=ctx) == (k, walked, blocker), \
            f"seed {seed} gang {ms}: reprieve"


@pytest.mark.parametrize("name", sorted(PGR.DIRECTED))
def test_the_directed_answers(name, oracle_mod):
    """The written-out answers: the reference gives them, and the closed form equals the reference."""
    build, table = PGR.DIRECTED[name]
    snaps, ms, cands = build()
    for on_equal in (False, True):
        want = PGR.reference(snaps, oracle_mod, ms, cands, NOW, on_equal)
        prefix, mask, blocker = paging.paged_preempt_gangs_of(snaps, ms, cands, NOW, on_equal)
        assert (prefix, blocker) == (want[0], want[2]), f"{name} on_equal={on_equal}"
        PGR.check_victims(snaps, oracle_mod, ms, cands, prefix, mask, NOW, on_equal)
        assert paging.paged_preempt_gangs_of(snaps, ms, cands, NOW, on_equal, reprieve=True) == want, f"{name} on_equal={on_equal}: reprieve"
        if on_equal in table:
            t_prefix, t_mask, t_walked, t_blocker = table[on_equal]
            assert want[0] == t_prefix, name
            assert t_mask is None or mask == t_mask, name
            assert t_walked is None or want[1] == t_walked, name
            assert t_blocker is None or want[2] == t_blocker, name


def test_what_the_directed_cases_pin(oracle_mod):
    snaps, ms, cands = PGR.gang_non_monotone_pages()
    assert [GR.reference(s, oracle_mod, ms, cands)[0] for s in snaps] == [1, 2]  # the pages' own gang prefixes, and not their maximum
    snaps, ms, cands = PGR.reserved_prefix_on_the_second_page()
    assert [PPR.reference_prefix(snaps, oracle_mod, p, cands) for p in ms] == [1, 1]  # each member alone; the gang needs 2
    snaps, ms, cands = PGR.blocker_is_the_minimum_over_pages()
    assert [GR.reference(s, oracle_mod, ms, cands)[1] for s in snaps] == [1, 0]  # page 0 stops member 1, page 1 member 0


@pytest.mark.parametrize("name", sorted(PPR.DIRECTED))
def test_a_gang_of_one_is_paged_preempt_of(name):
    snaps, p, cands = PPR.DIRECTED[name]()
    for on_equal in (False, True):
        for reprieve in (False, True):
            k, victims = paging.paged_preempt_of(snaps, p, cands, NOW, on_equal, reprieve=reprieve)
            assert paging.paged_preempt_gangs_of(snaps, [p], cands, NOW, on_equal, reprieve=reprieve) == (k, victims, -1 if k == 0 else 0)


def test_the_calculated_threshold_is_read_as_a_whole(oracle_mod):
    snaps = [b.snapshot for b in whole_threshold_cluster().build_pages()]
    assert PGR.reference(snaps, oracle_mod, [0], [1]) == (1, [1], 0)
    for reprieve in (False, True):
        assert paging.paged_preempt_gangs_of(snaps, [0], [1], NOW, reprieve=reprieve) == (1, [1], 0)


@pytest.mark.parametrize("seed", range(6))
def test_one_page_is_preempt_gangs_of(seed):
    snap = PR.preempt_cluster(seed).build_pages()[0].snapshot
    ctx, pctx = paging.preempt_context(snap, NOW), paging.paged_preempt_context([snap], NOW)
    for ms, cands in GR.gang_cases(seed, snap):
        for on_equal in (False, True):
            for reprieve in (False, True):
                assert paging.paged_preempt_gangs_of([snap], ms, cands, NOW, on_equal, reprieve=reprieve, ctx=pctx) == \
                    paging.preempt_gangs_of(snap, ms, cands, NOW, on_equal, ctx=ctx, reprieve=reprieve), f"seed {seed} gang {ms}"


def test_one_page_is_preempt_gangs_of_on_the_directed_tables():
    for name, entry in list(GR.DIRECTED.items()) + list(GRR.DIRECTED.items()):
        snap, ms, cands = entry[0]()
        for on_equal in (False, True):
            for reprieve in (False, True):
                assert paging.paged_preempt_gangs_of([snap], ms, cands, NOW, on_equal, reprieve=reprieve) == \
                    paging.preempt_gangs_of(snap, ms, cands, NOW, on_equal, reprieve=reprieve), name


def non_vacuity_counts(oracle_mod):
    """(positive prefixes, NONE, gangs whose prefix exceeds the maximum of the members' own paged prefixes, gangs whose reprieved set
    is smaller than the mask, gangs whose answer differs from the maximum of the pages' own gang prefixes or where a page other than
    page 0 binds) — from the reference alone, over the random cases and (the last three) the directed ones."""
    positive = none = exceeds = reprieved = across = 0
    gangs = []
    for seed, factor in CASES:
        _, snaps, cases = paged_gang_case(seed, factor)
        gangs += [(snaps, ms, cands, ans) for (ms, cands), ans in zip(cases, reference_answers(seed, factor, False))]
    for snaps, ms, cands, (k, walked, _) in gangs:
        positive += k > 0
        none += k == NONE
        if k > 0:
            own = [PPR.reference_prefix(snaps, oracle_mod, p, cands) for p in ms]
            exceeds += all(o >= 0 for o in own) and k > max(own)
            reprieved += sum(walked) < sum(paging.paged_preempt_gangs_of(snaps, ms, cands, NOW)[1])  # (the mask: held to the reference above)
            pages = [GR.reference(s, oracle_mod, ms, cands)[0] for s in snaps]
            across += k != max(pages) or max(pages[1:]) == k > pages[0]
    return positive, none, exceeds, reprieved, across


def test_the_cases_are_not_vacuous(oracle_mod):
    positive, none, exceeds, reprieved, across = non_vacuity_counts(oracle_mod)
    assert positive >= 5 and none >= 3 and exceeds >= 2 and reprieved >= 2 and across >= 1, (positive, none, exceeds, reprieved, across)
