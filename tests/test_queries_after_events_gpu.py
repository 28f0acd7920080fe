"""The admission queries on an engine that has lived through events.

Every other GPU file of the query family loads an engine with Engine.for_snapshot, asks once and closes it.  Here each test is one
short life of tests/lived_engine.py: an engine created EMPTY with spare capacity, fed by events (pods, throttles, reservations,
stored status, Namespace objects), reconciled, and after every further event held (``Life.hold``) to
  * a twin loaded fresh from the mirror at that moment — every array of the whole battery bit for bit (which side moved?),
  * the host models ``paging.*_of`` and the oracle on the mirror (who is right?),
  * itself: a second run of the battery equals the first (queries are dry).
The battery is check, dry admit, dry admit_gangs, headroom, headroom_gangs, headroom_forecast, preempt and preempt_gangs with and
without reprieve, forecast, forecast_gangs, override_instants and fetch_reserved, for both ``on_equal`` values; on two pages the
paged entry points, the paged gang headroom and the paged headroom forecast among them.  tests/test_lived_engine_cpu.py shows
on the models alone that every event of every life moves an answer and that the lives show every kind of outcome.  No tolerance.

``test_a_life_on_a_stretched_layout`` runs every life once more on engines of 1100 throttle rows and 4160 pod rows, its rows spread
by a lived_engine.Layout over both chunks of the matrix row and over 65 tiles of pod rows (`straddle`, `grow`), the rows in between
empty (`holes`) or holding records that affect nothing (`fillers`); there Life.hold also compares the physical status matrices of
live engine and twin over all 1100 columns and asserts that the columns outside the layout are zero."""
import numpy as np
import pytest

import lived_engine as LE
from kube_throttler_amd import engine as E
from kube_throttler_amd import snapshot as S

pytestmark = pytest.mark.gpu
NOW = LE.NOW


def live(script, oracle_mod, wide=False):
    life = LE.Life(oracle_mod, gpu=True, wide=wide)
    try:
        script(life)
        return [name for name, _ in life.held]
    finally:
        life.close()


def test_pod_events(oracle_mod):
    assert len(live(LE.life_pod_events, oracle_mod)) == 8


def test_threshold_and_override_events(oracle_mod):
    """upload_spec_tables without a recompile: compiles() stays (asserted inside the life after every event), the stored status is
    the old one until the last step's reconcile."""
    assert len(live(LE.life_threshold_and_override_events, oracle_mod)) == 6


def test_selector_and_row_events(oracle_mod):
    """A recompile with device-newer status, a throttle row beyond thr_rows_hi, a freed and a reused row: compiles() rises by one
    per event (asserted inside the life)."""
    assert len(live(LE.life_selector_and_row_events, oracle_mod)) == 7


def test_reservations_survive(oracle_mod):
    """fetch_reserved is part of the battery: it equals the mirror at every step."""
    assert len(live(LE.life_reservations_survive, oracle_mod)) == 6


def test_rows_appended(oracle_mod):
    """Second copies of limiting throttles in appended rows: ties, the lower row of a tie deleted and back."""
    assert len(live(LE.life_rows_appended, oracle_mod)) == 6


def test_two_pages_live(oracle_mod):
    assert len(live(LE.life_two_pages, oracle_mod, wide=True)) == 7


def test_page_one_decides_live(oracle_mod):
    """The web gang's paged headroom is decided by names of the last page: a reserved row, a threshold and a member's request of
    page 1 move it, and the deciding (throttle, page) pair goes to page 0 and back (tests/test_lived_engine_cpu.py asserts all of
    that on the models; here the live page engines are held to twin and models at every step)."""
    assert len(live(LE.life_page_one_decides, oracle_mod, wide=True)) == 7


def test_a_negative_request_on_page_one(oracle_mod):
    """Only page 1's engine has been fed a negative request.  kt_paged_headroom_gangs answers KT_ERR_UNSUPPORTED when ANY page has:
    on live and twin while the pod is there, on the live engines alone once it has gone; every other paged answer equals twin and
    models throughout.  Page 0's engine alone still serves its own gang headroom."""
    life = LE.Life(oracle_mod, gpu=True, wide=True)
    try:
        LE.life_negative_on_page_one(life)
        assert len(life.held) == 5
        q = life.q
        with pytest.raises(E.EngineError) as err:
            E.paged_headroom_gangs(life.engines, q.gang_rows, q.gang_off, LE.CAP)
        assert err.value.code == -7, err.value
        got = LE._answer(lambda: life.engines[0].headroom_gangs(q.gang_rows, q.gang_off, cap=LE.CAP))
        assert LE.same(got, life.alone[-1][1][False]), f"page 0's engine alone: {got}"
        with pytest.raises(E.EngineError) as err:
            life.engines[1].headroom_gangs(q.gang_rows, q.gang_off, cap=LE.CAP)
        assert err.value.code == -7 and "has been fed a negative request" in str(err.value), err.value
    finally:
        life.close()


def test_namespace_labels(oracle_mod):
    """Label swaps of Namespace objects reach the ClusterThrottles' namespaceSelector: one compile per gap with events, none in a
    gap without (asserted inside the life), a batch of two rows, a batch that names a row twice."""
    assert len(live(LE.life_namespace_labels, oracle_mod)) == 7


def test_namespace_deleted_and_back(oracle_mod):
    """kt_delete_namespaces, kt_upsert_namespaces with ns_valid = 0 and kt_upsert_namespace with exists = 0 reach the same state;
    the object's return gives the battery of the start back byte for byte (asserted inside the life)."""
    assert len(live(LE.life_namespace_deleted_and_back, oracle_mod)) == 8


def test_namespace_arrives_after_its_pods(oracle_mod):
    """An object for the row that had none, and a pod in a namespace row beyond what the program was compiled for."""
    assert len(live(LE.life_namespace_arrives_after_its_pods, oracle_mod)) == 6


def test_namespace_events_among_the_others(oracle_mod):
    """Behind reconcile(apply) (device-newer status), behind committed admissions (fetch_reserved is in the battery), beside pod
    events of the same namespace in both orders, in front of a threshold-only throttle event."""
    assert len(live(LE.life_namespace_events_among_the_others, oracle_mod)) == 7


@pytest.mark.parametrize("script,steps", [(LE.life_namespace_labels, 7), (LE.life_namespace_deleted_and_back, 8)],
                         ids=["labels", "deleted_and_back"])
def test_namespace_events_on_two_pages(script, steps, oracle_mod):
    """Every event reaches both pages' engines; paged_reconcile and the paged battery follow."""
    assert len(live(script, oracle_mod, wide=True)) == steps


STEPS = {"pod_events": 8, "threshold_and_override_events": 6, "selector_and_row_events": 7, "reservations_survive": 6,
         "negative_came_and_went": 5, "rows_appended": 6, "namespace_labels": 7, "namespace_deleted_and_back": 8,
         "namespace_arrives_after_its_pods": 6, "namespace_events_among_the_others": 7, "two_pages": 7, "page_one_decides": 7,
         "negative_on_page_one": 5, "namespace_labels_wide": 7, "namespace_deleted_and_back_wide": 8}
STRETCHED = [(name, layout, variant) for name in list(LE.LIVES) + list(LE.WIDE_LIVES) for layout in LE.TMAPS for variant in LE.VARIANTS]


@pytest.mark.parametrize("name,layout,variant", STRETCHED, ids=["-".join(x) for x in STRETCHED])
def test_a_life_on_a_stretched_layout(name, layout, variant, oracle_mod):
    """The same life, event for event and hold for hold, on Stretched engines: `straddle` puts the twelve throttles on both sides
    of row 1023/1024 and two of one pod's into one lane below a third, `grow` lets the first appended row carry the live engine's
    row count across 1024 behind answered queries; the pods lie on the edges of tiles 0, 1, 2, 32, 64 and 65.  What the life
    asserts about compiles() holds here too; kernel names and packed_words() belong to the compact cluster and are not asked."""
    wide = name in LE.WIDE_LIVES
    life = LE.Life(oracle_mod, gpu=True, wide=wide, layout=LE.Layout(layout, variant))
    try:
        (LE.WIDE_LIVES if wide else LE.LIVES)[name](life)
        assert len(life.held) == len(life.live_held) == STEPS[name]
        counts = [e.raw.throttle_rows() for e in life.engines]
        assert all(LE.CHUNK <= c <= LE.T_PHYS for c in counts), counts
    finally:
        life.close()


def _fingerprint(eng):
    return eng.kernel_name(E.KERNEL_AGGREGATE), eng.packed_words()


@pytest.mark.parametrize("case", LE.REFUSALS)
def test_a_refused_batch_leaves_the_engine_as_it_was(case, oracle_mod):
    """kt_upsert_pods refuses a batch whose SECOND pod breaks a rule; the first carries a negative request, larger than any the
    engine holds, with new odd low bits.  Nothing of it may stay: not the "a negative request was fed" mark (headroom_gangs would
    answer KT_ERR_UNSUPPORTED and the aggregate would leave the packed fold for good), not the bounds the pack plan is made from."""
    life = LE.Life(oracle_mod, gpu=True)
    try:
        LE.start(life)
        eng = life.eng
        before = life.live_held[-1][1]
        fold = _fingerprint(eng)
        counters = eng.compiles(), eng.view_builds()
        batch, rows, code = LE.refused_pod_batch(life.pl, case)
        with pytest.raises(E.EngineError) as err:
            eng.upsert_pods(batch, rows=rows)
        assert err.value.code == code, err.value
        assert (eng.compiles(), eng.view_builds()) == counters
        after = life.hold(f"a refused batch: {case}")
        LE.assert_same(before, after, "the battery before and after the refused batch")
        for cap in LE.CAPS:
            for eq in (False, True):
                assert not isinstance(after["headroom_gangs", cap, eq][0], str), "headroom_gangs is still served"
        life.reconcile()
        assert _fingerprint(eng) == fold, "the aggregate's kernel and its packed fold after the next reconcile"
        assert (eng.compiles(), eng.view_builds()) == counters
        LE.assert_same(before, life.hold("... and a reconcile behind it"), "the battery behind the next reconcile")
    finally:
        life.close()


@pytest.mark.parametrize("call", ["set_reserved", "set_status"])
def test_a_refused_status_batch_leaves_the_engine_as_it_was(call, oracle_mod):
    """kt_set_reserved / kt_set_status refuse an amount beyond 2^60 (kt_upsert_throttles validates its whole batch before it stores
    a row; these two stored row by row): a good row in front of the refused one must not stay changed."""
    life = LE.Life(oracle_mod, gpu=True)
    try:
        LE.start(life)
        eng = life.eng
        before = life.live_held[-1][1]
        D = life.mirror.snap.D
        rows = np.array([2, 5], np.int32)
        bad = S.Amounts(2, D)
        bad.set_row(0, {0: 7}, 1)
        bad.set_row(1, {0: 1 << 61}, 1)
        with pytest.raises(E.EngineError) as err:
            if call == "set_reserved":
                eng.set_reserved(rows, bad)
            else:
                eng.set_status(rows, bad, S.Amounts(2, D), [0, 0], [0, 0], [0, 0], [0, 0])
        assert err.value.code == -4, err.value
        LE.assert_same(before, life.hold(f"a refused {call}"), f"the battery before and after the refused {call}")
        life.set_reserved(3, ["1jx-p"])  # the next accepted call uploads the host's tables: nothing of the refused batch is among them
        life.hold("... and an accepted set_reserved of another row behind it")
    finally:
        life.close()


@pytest.mark.parametrize("call", ["delete_namespaces", "upsert_namespaces"])
def test_a_refused_namespace_batch_leaves_the_engine_as_it_was(call, oracle_mod):
    """The batch is [ns1, which holds counted pods; a row outside the capacity].  The refused call compiles nothing, so the battery
    cannot show what it left on the host: the decisive step is the recompile an UNRELATED selector-changing throttle event forces
    afterwards.  (kt_delete_namespaces stored row by row while it validated: the live engine lost ns1 there.)"""
    life = LE.Life(oracle_mod, gpu=True)
    try:
        LE.start(life)
        eng = life.eng
        before = life.live_held[-1][1]
        counters = eng.compiles(), eng.view_builds()
        rows = np.array([1, LE.NS_CAP], np.int32)
        with pytest.raises(E.EngineError) as err:
            if call == "delete_namespaces":
                eng.delete_namespaces(rows)
            else:  # (the good entry carries labels that would change answers: no ClusterThrottle admits env=dev)
                eng.upsert_namespaces(life.mirror.namespace_batch(["ns1@dev", "ns0"]), rows=rows)
        assert err.value.code == -2, err.value
        assert (eng.compiles(), eng.view_builds()) == counters
        after = life.hold(f"a refused {call}")
        LE.assert_same(before, after, f"the battery before and after the refused {call}")
        assert (eng.compiles(), eng.view_builds()) == counters
        t = life.pl.initial.index("ns2/t-web")
        life.upsert_throttles([t], ["ns2/t-web@db"])
        life.hold("... and an unrelated selector-changing throttle event behind it: the program is compiled from the host's state")
        assert eng.compiles() == counters[0] + 1
    finally:
        life.close()


def test_a_negative_request_that_came_and_went(oracle_mod):
    """While the pod is there headroom_gangs is KT_ERR_UNSUPPORTED on the live engine and on the twin, everything else equals twin
    and models.  Afterwards the live engine still refuses — kt_engine.h: "has been fed" — while the twin serves it, and every other
    answer of the live engine equals the twin's although the twin folds packed and the live engine plain."""
    life = LE.Life(oracle_mod, gpu=True)
    try:
        LE.life_negative_came_and_went(life)
        with pytest.raises(E.EngineError) as err:
            life.eng.headroom_gangs(life.q.gang_rows, life.q.gang_off, cap=LE.CAP)
        assert err.value.code == -7 and "has been fed a negative request" in str(err.value), err.value
        assert life.eng.packed_words() == 0, "the live engine folds plain"
        tw = life.twin()[0]
        try:
            tw.reconcile(NOW, apply=False)
            assert tw.packed_words() > 0, "the twin folds packed"
        finally:
            tw.close()
    finally:
        life.close()


def _code(f):
    try:
        f()
    except E.EngineError as err:
        return err.code
    return 0


def test_pending_results_across_a_namespace_event(oracle_mod):
    """kt_engine.h: a result that is pending when a namespace event arrives is not touched by it — "its fetch returns either the
    exact answer of the state at its launch or KT_ERR_NOT_READY, never anything else".  A check, a reconcile report, a forecast
    and a headroom forecast are each launched in front of a namespace event that moves their answer, and fetched behind it."""
    life = LE.Life(oracle_mod, gpu=True)
    try:
        LE.start(life)
        eng, q = life.eng, life.q
        at_start = life.live_held[-1][1]
        n, k = len(q.pods), len(LE.INSTANTS)
        outcome = {}

        def fetched(what, fetch, is_exact):
            try:
                got = fetch()
            except E.EngineError as err:
                assert err.code == -5, f"{what}: {err}"
                outcome[what] = "KT_ERR_NOT_READY"
                return
            assert is_exact(got), f"{what}: neither the answer of the state at launch nor KT_ERR_NOT_READY: {got}"
            outcome[what] = "the answer of the state at launch"

        eng.check_launch(n, q.pods, want_status=True)
        life.upsert_namespaces([1], ["ns1@dev"])
        fetched("check", lambda: eng.check_fetch(n, want_status=True), lambda got: LE.same(LE._answer(lambda: got), at_start["check", False]))
        moved = life.hold("ns1 becomes dev behind a pending check")
        assert LE.differences(moved, at_start, [("check", False)]), "the event moves the check's answer"

        rows = LE.responsible(life.mirror.snap)
        want = oracle_mod.Oracle(life.mirror.snap).reconcile(NOW, rows=rows)  # the report of the state at launch: ns1 is dev
        eng.reconcile_launch(NOW, apply=False)
        life.upsert_namespaces([1], ["ns1"])
        after = oracle_mod.Oracle(life.mirror.snap).reconcile(NOW, rows=rows)
        assert not np.array_equal(want.used.count, after.used.count), "the event moves the report"

        def report_is_exact(got):
            LE.assert_reconcile_equal(LE._rows_of(got, rows, life.mirror.snap.D), want, len(rows))
            return True

        fetched("reconcile report", eng.reconcile_fetch, report_is_exact)
        LE.assert_same(at_start, life.hold("ns1 is prod again behind a pending reconcile report"), "the battery of the start")

        eng.forecast_launch(q.pods, LE.INSTANTS)
        life.delete_namespaces([1])
        fetched("forecast", lambda: eng.forecast_fetch(n, k), lambda got: LE.same(LE._answer(lambda: got), at_start["forecast", False]))
        gone = life.hold("ns1 is deleted behind a pending forecast")
        assert LE.differences(gone, at_start, [("forecast", False)])

        key = ("headroom_forecast", LE.CAP, False)
        eng.headroom_forecast_launch(q.pods, LE.INSTANTS, LE.CAP, want=LE.WANT)
        life.upsert_namespaces([1], ["ns1"])
        fetched("headroom forecast", lambda: eng.headroom_forecast_fetch(n, k), lambda got: LE.same(LE._answer(lambda: got), gone[key]))
        back = life.hold("ns1 returns behind a pending headroom forecast")
        assert LE.differences(back, gone, [key]), "the event moves the headroom forecast's answer"
        LE.assert_same(at_start, back, "the battery of the start")
        print("pending across a namespace event:", outcome)
    finally:
        life.close()


def test_pending_results_across_queries(oracle_mod):
    """What kt_engine.h promises about results that are pending while another query is launched, on an engine that has had events:
    a pending forecast and a pending preempt result are independent; a preempt's dry finalize drops a pending reconcile report; the
    one headroom slot and the one preempt slot answer KT_ERR_NOT_READY to the other kind's fetch; a pending kt_check_launch is
    dropped by every query that uses the check slot; result buffers regrow under an unfetched smaller launch.  The headroom
    forecast is the forecast result's third kind."""
    life = LE.Life(oracle_mod, gpu=True)
    try:
        LE.start(life)
        life.upsert_pods([life.row("0jy-r")], ["0jx-r"])
        want = life.hold("an upsert before the slots are looked at")
        eng, q = life.eng, life.q
        ng, n, m, k = len(q.gang_off) - 1, len(q.pods), len(q.cands), len(LE.INSTANTS)
        same = lambda got, key: LE.same(LE._answer(lambda: got), want[key])
        # a forecast launched and not yet fetched is still fetchable, and correct, behind a preempt launch — and the other way round
        eng.forecast_launch(q.pods, LE.INSTANTS)
        eng.preempt_launch(q.pods, q.cands, NOW)
        assert same(eng.forecast_fetch(n, k), ("forecast", False)) and same(eng.preempt_fetch(n, m), ("preempt", False, False))
        eng.preempt_launch(q.pods, q.cands, NOW)
        eng.forecast_launch(q.pods, LE.INSTANTS)
        assert same(eng.preempt_fetch(n, m), ("preempt", False, False)) and same(eng.forecast_fetch(n, k), ("forecast", False))
        # a pending reconcile report is gone behind a preempt (its dry finalize wrote the result buffers)
        eng.reconcile_launch(NOW, apply=False)
        eng.preempt(q.pods, q.cands, NOW)
        assert _code(lambda: eng.reconcile_fetch()) == -5
        # one headroom slot, one preempt slot, one forecast slot: the other kind's fetch is not ready
        eng.headroom_launch(n, q.pods, LE.CAP)
        assert _code(lambda: eng.headroom_gangs_fetch(ng)) == -5
        assert same(eng.headroom_fetch(n), ("headroom", LE.CAP, False))
        eng.headroom_gangs_launch(q.gang_rows, q.gang_off, LE.CAP)
        assert _code(lambda: eng.headroom_fetch(n)) == -5
        assert same(eng.headroom_gangs_fetch(ng), ("headroom_gangs", LE.CAP, False))
        eng.preempt_launch(q.pods, q.cands, NOW)
        assert _code(lambda: eng.preempt_gangs_fetch(ng, m)) == -5
        eng.preempt_gangs_launch(q.gang_rows, q.gang_off, q.cands, NOW)
        assert _code(lambda: eng.preempt_fetch(n, m)) == -5
        assert same(eng.preempt_gangs_fetch(ng, m), ("preempt_gangs", False, False))
        eng.forecast_launch(q.pods, LE.INSTANTS)
        assert _code(lambda: eng.forecast_gangs_fetch(ng, k)) == -5
        eng.forecast_gangs_launch(q.gang_rows, q.gang_off, LE.INSTANTS)
        assert _code(lambda: eng.forecast_fetch(n, k)) == -5
        assert same(eng.forecast_gangs_fetch(ng, k), ("forecast_gangs", False))
        # the headroom forecast is the forecast result's third kind
        hf = ("headroom_forecast", LE.CAP, False)
        hf_launch = lambda: eng.headroom_forecast_launch(q.pods, LE.INSTANTS, LE.CAP, want=LE.WANT)
        hf_launch()
        assert _code(lambda: eng.forecast_fetch(n, k)) == -5 and _code(lambda: eng.forecast_gangs_fetch(ng, k)) == -5
        assert same(eng.headroom_forecast_fetch(n, k), hf)
        eng.forecast_launch(q.pods, LE.INSTANTS)
        assert _code(lambda: eng.headroom_forecast_fetch(n, k)) == -5
        assert same(eng.forecast_fetch(n, k), ("forecast", False))
        eng.forecast_gangs_launch(q.gang_rows, q.gang_off, LE.INSTANTS)
        assert _code(lambda: eng.headroom_forecast_fetch(n, k)) == -5
        assert same(eng.forecast_gangs_fetch(ng, k), ("forecast_gangs", False))
        # ... a pending preempt result of either kind stays fetchable behind it, and it behind a preempt launch
        eng.preempt_launch(q.pods, q.cands, NOW)
        hf_launch()
        assert same(eng.preempt_fetch(n, m), ("preempt", False, False)) and same(eng.headroom_forecast_fetch(n, k), hf)
        eng.preempt_gangs_launch(q.gang_rows, q.gang_off, q.cands, NOW)
        hf_launch()
        assert same(eng.preempt_gangs_fetch(ng, m), ("preempt_gangs", False, False)) and same(eng.headroom_forecast_fetch(n, k), hf)
        hf_launch()
        eng.preempt_launch(q.pods, q.cands, NOW)
        assert same(eng.headroom_forecast_fetch(n, k), hf) and same(eng.preempt_fetch(n, m), ("preempt", False, False))
        hf_launch()
        eng.preempt_gangs_launch(q.gang_rows, q.gang_off, q.cands, NOW)
        assert same(eng.headroom_forecast_fetch(n, k), hf) and same(eng.preempt_gangs_fetch(ng, m), ("preempt_gangs", False, False))
        # ... and its dry finalize drops a pending reconcile report
        eng.reconcile_launch(NOW, apply=False)
        eng.headroom_forecast(q.pods, LE.INSTANTS, cap=LE.CAP, want=LE.WANT)
        assert _code(lambda: eng.reconcile_fetch()) == -5
        # a pending kt_check_launch (with the status matrix: not the few-pod path) is gone behind every query that uses the slot
        for ask in (lambda: eng.headroom(rows=q.pods, cap=LE.CAP), lambda: eng.headroom_gangs(q.gang_rows, q.gang_off, cap=LE.CAP),
                    lambda: eng.preempt(q.pods, q.cands, NOW), lambda: eng.preempt_gangs(q.gang_rows, q.gang_off, q.cands, NOW),
                    lambda: eng.forecast(q.pods, LE.INSTANTS), lambda: eng.forecast_gangs(q.gang_rows, q.gang_off, LE.INSTANTS),
                    lambda: eng.headroom_forecast(q.pods, LE.INSTANTS, cap=LE.CAP, want=LE.WANT)):
            eng.check_launch(len(q.gang_rows), q.gang_rows, want_status=True)
            ask()
            assert _code(lambda: eng.check_fetch(len(q.gang_rows), want_status=True)) == -5
        # ... and replaced behind an admission, whose results ARE read with kt_check_fetch
        eng.check_launch(len(q.gang_rows), q.gang_rows, on_equal=True, want_status=True)
        eng.admit(rows=q.gang_rows)
        assert same(eng.check_fetch(len(q.gang_rows), want_status=True), ("admit", False))
        # result buffers regrow under a smaller launch that was never fetched
        eng.forecast_launch(q.pods[:1], LE.INSTANTS[:2])
        eng.forecast_launch(q.pods, LE.INSTANTS)
        assert same(eng.forecast_fetch(n, k), ("forecast", False))
        eng.forecast_gangs_launch(q.members(0), [0, 1], LE.INSTANTS[:2])
        eng.forecast_gangs_launch(q.gang_rows, q.gang_off, LE.INSTANTS)
        assert same(eng.forecast_gangs_fetch(ng, k), ("forecast_gangs", False))
        eng.preempt_launch(q.pods[:1], q.cands[:2], NOW)
        eng.preempt_reprieve_launch(q.pods, q.cands, NOW)
        assert same(eng.preempt_fetch(n, m), ("preempt", True, False))
        eng.preempt_gangs_launch(q.members(0), [0, 1], q.cands[:2], NOW)
        eng.preempt_gangs_reprieve_launch(q.gang_rows, q.gang_off, q.cands, NOW)
        assert same(eng.preempt_gangs_fetch(ng, m), ("preempt_gangs", True, False))
        eng.headroom_launch(1, q.pods[:1], LE.CAP)
        eng.headroom_launch(n, q.pods, LE.CAP)
        assert same(eng.headroom_fetch(n), ("headroom", LE.CAP, False))
        eng.headroom_gangs_launch(q.members(0), [0, 1], LE.CAP)
        eng.headroom_gangs_launch(q.gang_rows, q.gang_off, LE.CAP)
        assert same(eng.headroom_gangs_fetch(ng), ("headroom_gangs", LE.CAP, False))
        # ... the headroom forecast's too: 1 pod x 2 instants, never fetched, then every pod x 70 instants (from position 64 on a
        # lane owns a second cell of a pod's row of the copies buffer, which the kernel also uses as scratch)
        last = LE.INSTANTS[-1]
        long = list(LE.INSTANTS) + [(int(last[0]) + 3600 * (i + 1), i) for i in range(70 - k)]
        assert len(long) == 70 and [(int(a), int(b)) for a, b in long] == sorted({(int(a), int(b)) for a, b in long})
        snap = life.mirror.snap
        ctx = LE.paging.preempt_context(snap, NOW)
        a = [LE.paging.headroom_forecast_of(snap, p, long, LE.CAP, LE.WANT, False, ctx=ctx) for p in q.pods]
        model = (np.array([x[0] for x in a], np.int64), np.array([x[1] for x in a], np.int64).reshape(n, 70),
                 np.array([x[2] for x in a], np.int32).reshape(n, 70))
        eng.headroom_forecast_launch(q.pods[:1], LE.INSTANTS[:2], LE.CAP, want=LE.WANT)
        eng.headroom_forecast_launch(q.pods, long, LE.CAP, want=LE.WANT)
        got = LE._answer(lambda: eng.headroom_forecast_fetch(n, 70))
        assert LE.same(got, model), f"70 instants behind an unfetched 1 x 2 launch:\n  {got}\n  {model}"
        assert LE.same(tuple(x[:, :k] if x.ndim == 2 else x for x in got[1:]), tuple(want[hf][1:])), "... its first instants are the battery's"
        life.hold("behind all of it the battery is what it was")
    finally:
        life.close()
