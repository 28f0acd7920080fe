"""The lives of tests/lived_engine.py, replayed on the mirror alone (models and oracle, no GPU): they are not vacuous.

tests/test_queries_after_events_gpu.py holds a live engine to a fresh twin and to the host models after every event of a life.  That
tests something only if the events move the answers and the answers show every kind of outcome — which is checked here, where it
can be checked without a GPU:
  * every event changes at least one model answer of the battery against the step before;
  * over all lives the battery shows a pod admitted, blocked `active`, blocked `insufficient` and an Error; a gang admitted and a gang
    rolled back (a member was admitted, the gang is not); a headroom of 0, one strictly between 0 and CAP and one at CAP; a
    preemption prefix of 0, an inner one and "no prefix helps"; a forecast that flips inside the instants; a headroom forecast
    with copies of 0, inner and CAP, copies and limiting rows that differ between two instants, `first` 0, inner and none; over
    the wide lives a paged gang headroom of 0, inner and CAP, an inner answer that a name of the last page decides, and a
    deciding (throttle, page) pair that moves to the other page;
  * the named steps of the life ``page_one_decides`` each move the web gang's paged headroom entry;
  * the mirror after each life equals a mirror built in one go from the same final placement, in every field a load reads;
  * the refused batches are refused for the stated reason alone, behind a negative, larger, odd request."""
import numpy as np
import pytest

import forecast_reference as FR
import lived_engine as LE
from kube_throttler_amd import snapshot as S

ALL_LIVES = dict(LE.LIVES, **LE.WIDE_LIVES)


@pytest.fixture(scope="module")
def replayed(oracle_mod):
    out = {}
    for name, script in ALL_LIVES.items():
        life = LE.Life(oracle_mod, gpu=False, wide=name in LE.WIDE_LIVES)
        script(life)
        out[name] = life
    return out


@pytest.mark.parametrize("name", list(ALL_LIVES))
def test_every_event_moves_an_answer(name, replayed):
    held = replayed[name].held
    assert len(held) >= 5
    for (before, a), (step, b) in zip(held[:-1], held[1:]):
        moved = LE.differences(a, b)
        print(f"{name}: {step}: {len(moved)} answers moved, e.g. {moved[:4]}")
        assert moved, f"{name}: '{step}' changes no model answer against '{before}'"


def test_namespace_events_move_most_of_the_battery(replayed):
    """A namespace event is no corner of the battery: of its 32 entries the ns2 -> prod swap moves 24, the ns1 delete 30 (all but
    override_instants and the reserved rows) and the object's return moves them all back; the ghost's object moves 22.  (Before
    the four headroom_forecast entries: 28 entries, 20, 26 and 18 moved — each event moves all four of them.)"""
    def moved(name, a, b):
        held = replayed[name].held
        assert len(held[a][1]) == 32
        return len(LE.differences(held[a][1], held[b][1]))

    assert replayed["namespace_labels"].held[1][0] == "ns2 becomes prod"
    assert moved("namespace_labels", 0, 1) == 24
    assert replayed["namespace_deleted_and_back"].held[1][0] == "delete_namespaces takes the object of ns1"
    assert moved("namespace_deleted_and_back", 0, 1) == 30
    assert moved("namespace_deleted_and_back", 0, 2) == 0
    assert replayed["namespace_arrives_after_its_pods"].held[1][0] == "the namespace without an object gets one"
    assert moved("namespace_arrives_after_its_pods", 0, 1) == 22


def test_a_deleted_namespace_answers_error(replayed):
    """The pods of ns1 among the single pods and the gang members answer Error while its object is gone, by the models."""
    life = replayed["namespace_deleted_and_back"]
    b = dict(life.held)["delete_namespaces takes the object of ns1"]
    ns1 = [i for i, p in enumerate(life.q.pods) if life.pl.placement[p].startswith("1") or life.pl.placement[p] == "zero"]
    assert len(ns1) >= 3
    for eq in (False, True):
        assert ((b["check", eq][1][ns1] & np.uint64(3)) == S.VERDICT_ERROR).all()


def test_a_headroom_answer_changes_its_limiting_throttle(replayed):
    """What the threshold edit is for: same pod, another limiting row."""
    held = replayed["threshold_and_override_events"].held  # (the check reads the STORED calculated threshold: the last step's reconcile)
    (_, a), (_, b) = held[0], held[-1]
    la, lb = a["headroom", LE.CAP, False][1], b["headroom", LE.CAP, False][1]
    assert ((la != lb) & (la >= 0) & (lb >= 0)).any(), (la, lb)


def test_the_new_throttle_blocks_a_pod_nobody_blocked(replayed):
    life = replayed["selector_and_row_events"]
    steps = dict(life.held)
    i = list(life.q.pods).index(life.row("none"))
    assert steps["start"]["check", False][1][i] == 0
    assert int(steps["a new throttle appears in a row beyond thr_rows_hi"]["check", False][1][i]) & 3 == S.VERDICT_BLOCK


def test_deleted_rows_answer_as_the_header_says(replayed):
    """0 copies, blocked in front of the deleted member, no limiting throttle."""
    life = replayed["pod_events"]
    b = dict(life.held)["a delete hits a gang member and a candidate"]
    copies, limiting, blocker = b["headroom_gangs", LE.CAP, False]
    assert (copies[2], limiting[2], blocker[2]) == (0, -1, life.q.gang_off[2] + 1)


def _gang_entry(answer, g):
    copies, limiting, blocker = answer
    return int(copies[g]), int(limiting[g]), int(blocker[g])


def _decided_by(life, i, g, eq=False):
    """Which page decides gang g's paged headroom at step number i: None unless the answer is inner (0 < copies < CAP); 0 where it
    is what page 0 alone would answer, 1 where it differs from that (a name of the last page decides) -> (page, entry)."""
    entry = _gang_entry(life.held[i][1]["headroom_gangs", LE.CAP, eq], g)
    if not 0 < entry[0] < LE.CAP:
        return None, entry
    return (0 if entry == _gang_entry(life.alone[i][1][eq], g) else 1), entry


def _paged_gang_headroom_kinds(life):
    """The outcome kinds of the paged gang headroom over one wide life."""
    seen = set()
    assert [step for step, _ in life.alone] == [step for step, _ in life.held]
    for g in range(len(life.q.gang_off) - 1):
        for eq in (False, True):
            pages = [_decided_by(life, i, g, eq) for i in range(len(life.held))]
            for page, (copies, _, _) in pages:
                seen.add("paged headroom_gangs " + ("0" if copies == 0 else "cap" if copies == LE.CAP else "inner"))
                if page == 1:
                    seen.add("paged headroom_gangs page 1 decides an inner answer")
            for (pa, a), (pb, b) in zip(pages[:-1], pages[1:]):
                if {pa, pb} == {0, 1} and a[1] != b[1]:  # the deciding pair moved to the other page: another limiting row, copies inner
                    seen.add("paged headroom_gangs the decider changes page")
    return seen


def test_the_steps_of_page_one_decides_move_the_web_gang(replayed):
    """The web gang's ("headroom_gangs", CAP, False) entry: decided by page 1 once the web throttles leave room, moved by every step
    of PAGE_ONE_STEPS against the step before, and the deciding (throttle, page) pair goes to page 0 and back with copies inner."""
    life = replayed["page_one_decides"]
    g = life.q.WEB_GANG
    names = [step for step, _ in life.held]
    assert names[2:] == list(LE.PAGE_ONE_STEPS)
    at = [_decided_by(life, i, g) for i in range(len(names))]
    print([(n, a) for n, a in zip(names, at)])
    assert at[0][0] is None and at[0][1][0] == 0, f"the web throttles of the start are saturated: {at[0]}"
    assert at[1][0] == 1, f"{names[1]}: {at[1]}, page 0 alone {_gang_entry(life.alone[1][1][False], g)}"
    for i in range(2, len(names)):
        assert at[i][1] != at[i - 1][1], f"'{names[i]}' does not move the web gang's entry: {at[i]}"
        assert at[i][0] is not None, f"'{names[i]}': copies are not inner: {at[i]}"
    assert [a[0] for a in at[1:]] == [1, 1, 1, 1, 0, 1]
    for i in (5, 6):  # the decider switches page: another limiting row
        assert at[i][1][1] != at[i - 1][1][1] and at[i][1][1] >= 0 and at[i - 1][1][1] >= 0, (names[i], at[i - 1], at[i])
    # the pod event is of a member's row and changes nothing but its request of a last-page name
    assert life.row("1wy-p") in life.q.members(g)
    pl, (page, d) = life.pl, life.pl.dim("memory")
    assert page == 1
    was, now = (LE.paging.pod_requests(pl.snaps[1], pl.pod[k]) for k in ("1wy-p", "0wy-p"))
    assert was[d] != now[d] and {k: v for k, v in was.items() if k != d} == {k: v for k, v in now.items() if k != d}
    assert LE.paging.pod_requests(pl.snaps[0], pl.pod["1wy-p"]) == LE.paging.pod_requests(pl.snaps[0], pl.pod["0wy-p"])


def test_the_negative_request_is_on_page_one_alone():
    pl = LE.pool(wide=True)
    neg = [{d: v for d, v in LE.paging.pod_requests(s, pl.pod["neg1"]).items() if v < 0} for s in pl.snaps]
    assert neg[0] == {} and list(neg[1]) == [pl.dim("memory")[1]] and pl.dim("memory")[0] == 1, neg
    assert "neg1" not in pl.placement


def test_the_battery_shows_every_outcome_kind(replayed):
    seen = set()
    for life in replayed.values():
        if len(life.mirror.snaps) > 1:
            seen |= _paged_gang_headroom_kinds(life)
            continue
        q = life.q
        for _, b in life.held:
            for eq in (False, True):
                verdict, _, active, insufficient = S.summary_fields(b["admit", eq][1])
                seen |= {"pod admitted"} if (verdict == 0).any() else set()
                seen |= {"pod active"} if ((verdict == 1) & (active > 0)).any() else set()
                seen |= {"pod insufficient"} if ((verdict == 1) & (insufficient > 0)).any() else set()
                seen |= {"pod error"} if (verdict == 2).any() else set()
                _, sm, admitted = b["admit_gangs", eq]
                for g in range(len(admitted)):
                    v = sm[q.gang_off[g]:q.gang_off[g + 1]] & np.uint64(3)
                    if admitted[g] and len(v) > 1:
                        seen.add("gang admitted")
                    if not admitted[g] and (v == 0).any():
                        seen.add("gang rolled back")
                for kind in ("headroom", "headroom_gangs"):
                    c = b[kind, LE.CAP, eq][0]
                    seen |= {f"{kind} 0"} if (c == 0).any() else set()
                    seen |= {f"{kind} inner"} if ((c > 0) & (c < LE.CAP)).any() else set()
                    seen |= {f"{kind} cap"} if (c == LE.CAP).any() else set()
                first, copies, limiting = b["headroom_forecast", LE.CAP, eq]
                seen |= {"headroom_forecast 0"} if (copies == 0).any() else set()
                seen |= {"headroom_forecast inner"} if ((copies > 0) & (copies < LE.CAP)).any() else set()
                seen |= {"headroom_forecast cap"} if (copies == LE.CAP).any() else set()
                seen |= {"headroom_forecast first 0"} if (first == 0).any() else set()
                seen |= {"headroom_forecast first inner"} if (first > 0).any() else set()
                seen |= {"headroom_forecast first none"} if (first == -1).any() else set()
                for c, l in zip(copies, limiting):
                    if len(set(c)) > 1:
                        seen.add("headroom_forecast copies differ between two instants")
                    if len(set(l[l >= 0])) > 1:
                        seen.add("headroom_forecast limiting row differs between two instants")
                for kind in ("preempt", "preempt_gangs"):
                    for rep in (False, True):
                        k = b[kind, rep, eq][0]
                        seen |= {f"{kind} 0"} if (k == 0).any() else set()
                        seen |= {f"{kind} inner"} if (k > 0).any() else set()
                        seen |= {f"{kind} none"} if (k == -1).any() else set()
                    plain, walked = b[kind, False, eq][1], b[kind, True, eq][1]
                    if plain.sum() > walked.sum():
                        seen.add(f"{kind} reprieve puts a victim back")
                for kind in ("forecast", "forecast_gangs"):
                    if any(FR.flips(row) for row in b[kind, eq][1]):
                        seen.add(f"{kind} flips")
    want = {"pod admitted", "pod active", "pod insufficient", "pod error", "gang admitted", "gang rolled back"}
    want |= {f"{k} {x}" for k in ("headroom", "headroom_gangs") for x in ("0", "inner", "cap")}
    want |= {f"{k} {x}" for k in ("preempt", "preempt_gangs") for x in ("0", "inner", "none", "reprieve puts a victim back")}
    want |= {"forecast flips", "forecast_gangs flips"}
    want |= {f"headroom_forecast {x}" for x in ("0", "inner", "cap", "first 0", "first inner", "first none",
                                                "copies differ between two instants", "limiting row differs between two instants")}
    want |= {f"paged headroom_gangs {x}" for x in ("0", "inner", "cap", "page 1 decides an inner answer", "the decider changes page")}
    assert want <= seen, sorted(want - seen)


@pytest.mark.parametrize("name", list(ALL_LIVES))
def test_the_mirror_equals_one_built_from_scratch(name, replayed):
    life = replayed[name]
    old = life.mirror
    pod_name = {v: k for k, v in life.pl.pod.items()}
    thr_name = {v: k for k, v in life.pl.thr.items()}
    new = LE.Mirror(life.pl)
    new.n_thr, new.n_pods = old.n_thr, old.n_pods
    held = [t for t in range(old.n_thr) if old.tstate[t] >= 0]
    new.put_throttles(held, [thr_name[int(old.tstate[t])] for t in held])
    new.put_namespaces(range(len(old.nstate)), old.nstate)
    live = [r for r in range(old.n_pods) if old.state[r] >= 0]
    new.put_pods(live, [pod_name[int(old.state[r])] for r in live], [old.pod_ns.get(r) for r in live])
    for a, b in zip(old.snaps, new.snaps):  # the stored status and the reservations are the life's own: taken over as they are
        for f in ("thr_used", "thr_calc", "thr_reserved", "thr_thrl_flag", "thr_thrl_has", "thr_status_msgs_fp"):
            setattr(b, f, getattr(a, f))
        b.thr_flags[:] |= a.thr_flags & np.uint32(LE.STATUS_BITS)
        fa, fb = LE.load_fields(a), LE.load_fields(b)
        assert fa.keys() == fb.keys()
        for f in fa:
            assert fa[f] == fb[f], f"{name}: field {f}"


@pytest.mark.parametrize("case", LE.REFUSALS)
def test_the_refused_batches_break_one_rule_each(case):
    pl = LE.pool()
    b, rows, code = LE.refused_pod_batch(pl, case)
    base = pl.snaps[0]
    d = pl.dim("cpu")[1]
    neg = int(b.ctr_req[0, d])
    assert neg < 0 and -neg > int(np.abs(base.ctr_req).max()) and neg & 1, "entry 0: negative, larger than any request, odd"
    assert 0 <= rows[0] < LE.P_CAP and b.pod_ns[0] < base.n_ns and b.pod_label_off[1] <= base.L
    broken = {"row-outside-capacity": rows[1] >= LE.P_CAP, "namespace-id-outside-capacity": b.pod_ns[1] >= base.n_ns + 1,
              "more-labels-than-kept": int(b.pod_label_off[2]) - int(b.pod_label_off[1]) > max(base.L, 1),
              "request-beyond-2^60": int(np.abs(b.ctr_req[1]).max()) > 1 << 60}
    assert [k for k, v in broken.items() if v] == [case]
    assert code == (-4 if case == "request-beyond-2^60" else -2)
