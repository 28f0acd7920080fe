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
    deciding (throttle, page) pair that moves to the other page; a paged headroom forecast that differs from page 0's alone and
    one whose `first` lies inside the instants;
  * the named steps of the life ``page_one_decides`` each move the web gang's paged headroom entry;
  * the mirror after each life equals a mirror built in one go from the same final placement, in every field a load reads;
  * the refused batches are refused for the stated reason alone, behind a negative, larger, odd request;
  * the stretched row layouts (lived_engine.Layout) are faithful — models and oracle on the STRETCHED mirror, answers mapped back by
    the methods the Stretched engines use, equal the compact mirror's byte for byte at every hold — and cover what they are for:
    both chunks of the matrix row, a list order that differs from the row order, ties between far rows, a row count that crosses 1024."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest

import forecast_reference as FR
import lived_engine as LE
from kube_throttler_amd import paging
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


def _paged_headroom_forecast_kinds(life):
    """The outcome kinds of the paged headroom forecast over one wide life: an answer that differs from what page 0 alone would
    give (a name of a later page decides copies or limiting row at some instant), and a `first` inside the instants."""
    seen = set()
    assert [step for step, _ in life.alone_forecast] == [step for step, _ in life.held]
    for (_, b), (_, alone) in zip(life.held, life.alone_forecast):
        for eq in (False, True):
            ans = b["headroom_forecast", LE.CAP, eq]
            if isinstance(ans[0], str):
                continue
            if not LE.same(ans, alone[eq]):
                seen.add("paged headroom_forecast differs from page 0's alone")
            if (ans[0] > 0).any():
                seen.add("paged headroom_forecast first inner")
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
            seen |= _paged_gang_headroom_kinds(life) | _paged_headroom_forecast_kinds(life)
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
    want |= {"paged headroom_forecast differs from page 0's alone", "paged headroom_forecast first inner"}
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


# ---- the stretched layouts ---------------------------------------------------------------------------------------------------
FILLER_LIVES = ("selector_and_row_events",)  # the lives whose `fillers` variant is replayed here (the others: too slow, see below)
STRETCHED = [(name, layout, variant) for name in ALL_LIVES for layout in LE.TMAPS for variant in LE.VARIANTS
             if variant == "holes" or name in FILLER_LIVES]
_RUNS = {}


def _stretched_run(name, layout, variant, oracle_mod):
    """One life replayed with a Layout: per hold the models' battery and the oracle's dry reconcile on the stretched mirror (mapped
    back) next to the compact mirror's, and the stretched snapshots themselves."""
    key = (name, layout, variant)
    if key not in _RUNS:
        lay = LE.Layout(layout, variant)
        life = LE.Life(oracle_mod, gpu=False, wide=name in LE.WIDE_LIVES, layout=lay)
        holds = []

        def watch(life, step):
            got, snaps = LE.stretched_model_battery(life.mirror, life.q, lay, oracle_mod)
            reconciles = []
            for m, s in zip(life.mirror.snaps, snaps):
                rows = LE.responsible(m)
                reconciles.append((LE.reconcile_answer(oracle_mod, s, lay.thr(rows)), LE.reconcile_answer(oracle_mod, m, rows)))
            holds.append(SimpleNamespace(step=step, got=got, want=life.held[-1][1], reconciles=reconciles, snaps=snaps,
                                         q=lay.questions(life.q), lay=lay))

        life.watch = watch
        ALL_LIVES[name](life)
        assert len(holds) == len(life.held) >= 5
        _RUNS[key] = holds
    return _RUNS[key]


@pytest.mark.parametrize("name,layout,variant", STRETCHED, ids=["-".join(x) for x in STRETCHED])
def test_the_stretched_mirror_answers_as_the_compact_one(name, layout, variant, oracle_mod):
    """Faithfulness of the harness, before it is trusted on a GPU: at every hold of every life the oracle's reconcile, check and
    admit and the ``paging.*_of`` models on the stretched mirror (T up to 1100 rows, P up to 4160), mapped back, equal the same on
    the compact mirror — integers and bytes.  The status matrices' columns outside the map are all zero (Layout.status asserts it).
    With `fillers` a hold costs about 12 s here (``preempt_context`` walks 2000 filler pods x 500 filler throttles in Python), so
    that variant replays ``selector_and_row_events`` alone — the life that appends, deletes and re-tenants throttle rows; every
    other life is dropped from `fillers` HERE (all of LIVES and WIDE_LIVES but that one), and every life runs on `holes`."""
    holds = _stretched_run(name, layout, variant, oracle_mod)
    for h in holds:
        LE.assert_same(h.got, h.want, f"{name} on {h.lay}: '{h.step}': the stretched mirror's battery against the compact one's")
        assert set(h.got) == set(h.want)
        for k, (got, want) in enumerate(h.reconciles):
            assert LE.same(got, want), f"{name} on {h.lay}: '{h.step}': the oracle's reconcile of page {k}"


def _without_row(snaps, t):
    out = []
    for s in snaps:
        c = copy.copy(s)
        c._keep = None
        c.thr_flags = s.thr_flags.copy()
        c.thr_flags[t] = 0
        out.append(c)
    return out


def _ties(h, kind, eq=False):
    """The ties among one hold's answers of ``kind``: (copies, limiting row L, the other row) where the models answer the same
    number of copies with throttle row L taken away, and name a row at least a lane above L instead — physical rows."""
    ans = h.got[kind, LE.CAP, eq]
    if isinstance(ans[0], str):
        return []
    lim = np.asarray(ans[2] if kind == "headroom_forecast" else ans[1])
    cop = np.asarray(ans[1] if kind == "headroom_forecast" else ans[0])
    out, ctxs = [], {}
    n = len(h.q.gang_off) - 1 if kind == "headroom_gangs" else len(h.q.pods)
    for i in range(n):
        for l in sorted(set(int(x) for x in np.atleast_1d(lim[i]) if x >= 0)):
            L = int(h.lay.tmap[l])
            snaps = _without_row(h.snaps, L)
            if kind == "headroom":
                c2, l2 = paging.headroom_of([SimpleNamespace(snapshot=s) for s in snaps], int(h.q.pods[i]), LE.CAP, eq)
                pairs = [(int(cop[i]), c2, l2)]
            elif kind == "headroom_gangs":
                c2, l2, _ = paging.paged_headroom_gangs_of(snaps, h.q.members(i), LE.CAP, eq) if len(snaps) > 1 else \
                    paging.headroom_gangs_of(snaps[0], h.q.members(i), LE.CAP, eq)
                pairs = [(int(cop[i]), c2, l2)]
            else:
                if L not in ctxs:
                    ctxs[L] = paging.paged_preempt_context(snaps, LE.NOW) if len(snaps) > 1 else paging.preempt_context(snaps[0], LE.NOW)
                _, c2, l2 = paging.paged_headroom_forecast_of(snaps, int(h.q.pods[i]), LE.INSTANTS, LE.CAP, LE.WANT, eq, ctx=ctxs[L]) \
                    if len(snaps) > 1 else paging.headroom_forecast_of(snaps[0], int(h.q.pods[i]), LE.INSTANTS, LE.CAP, LE.WANT, eq, ctx=ctxs[L])
                pairs = [(int(c), int(a), int(b)) for c, x, a, b in zip(cop[i], lim[i], c2, l2) if x == l]
            out += [(c, L, int(b)) for c, a, b in pairs if a == c and b >= L + LE.LANE]
    return out


def _list_order_differs(rows):
    """Within one chunk of the matrix row: two of these rows in one 16-byte lane and one in a higher lane — the affected-throttle
    list, filled round by round over the lanes, then reads low, HIGH, low."""
    rows = np.asarray(rows, np.int64)
    for c in set(rows // LE.CHUNK):
        lanes = sorted(rows[rows // LE.CHUNK == c] // LE.LANE)
        for a, b in zip(lanes[:-1], lanes[1:]):
            if a == b and lanes[-1] > a:
                return True
    return False


@pytest.mark.parametrize("layout", list(LE.TMAPS))
def test_what_the_layouts_cover(layout, oracle_mod):
    """Know what the stretched lives reach (on the stretched mirror, `holes`; the fillers affect no question pod): a question pod
    with live affecting throttles in both chunks of the matrix row; one whose affecting rows make the list order differ from the
    row order; for headroom, gang headroom and headroom forecast an answer where two affecting rows at least 16 rows apart allow
    the same number of copies and the lower one is reported — an inner number of copies among them; a gang over two tiles of pod
    rows; and on `grow` a life whose row count is at or below 1024 at one hold and above it at a later one."""
    both = order = 0
    crossed, ties, inner = [], {}, {}
    kinds = ("headroom", "headroom_gangs", "headroom_forecast")
    for name in sorted(ALL_LIVES, key=lambda n: n != "rows_appended"):  # (the life made for ties first: the search stops early)
        holds = _stretched_run(name, layout, "holes", oracle_mod)
        counts = [h.snaps[0].n_thr for h in holds]
        if any(a <= LE.CHUNK < b for i, a in enumerate(counts) for b in counts[i + 1:]):
            crossed.append(name)
        for h in holds:
            for p in sorted(set(int(x) for x in h.q.pods) | set(int(x) for x in h.q.gang_rows)):
                if not int(h.snaps[0].pod_flags[p]) & S.POD_VALID:
                    continue
                err, rows = paging.affected_throttles(h.snaps[0], p)
                rows = np.asarray(rows, np.int64)
                both += bool(len(rows) and rows.min() < LE.CHUNK <= rows.max())
                order += _list_order_differs(rows)
            for kind in kinds:
                if not inner.get(kind):
                    found = _ties(h, kind)
                    ties[kind] = ties.get(kind, 0) + len(found)
                    inner[kind] = inner.get(kind, 0) + sum(0 < c < LE.CAP for c, _, _ in found)
                    if found:
                        print(f"{layout}: {name}: '{h.step}': {kind} ties (copies, limiting row, the other row): {found[:4]}")
        q = holds[0].q
        for g in range(len(q.gang_off) - 1):
            if len(q.members(g)) > 1:
                assert len(set(int(r) // LE.TILE for r in q.members(g))) >= 2, f"gang {g} lies in one tile of pod rows"
    print(f"{layout}: {both} (hold, pod) pairs with affecting rows in both chunks, {order} whose list order differs from the row order, "
          f"ties {ties} (inner {inner}), row count crosses 1024 in {crossed}")
    assert both >= 20 and order >= 20
    for kind in kinds:
        assert ties[kind] >= 1 and inner[kind] >= 1, f"{kind}: {ties[kind]} ties, {inner[kind]} at an inner number of copies"
    if layout == "grow":
        assert "rows_appended" in crossed and "selector_and_row_events" in crossed, crossed
