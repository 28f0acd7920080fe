"""The text of every refusal of the admission queries (csrc/kt_engine_queries.cpp), as kt_last_error hands it to the plugin's logs.

The per-query tests pin each refusal's code and order; this module pins the words.  ``walk()`` provokes, per entry point, the
refusals those tests provoke — on the smallest cluster they use: two pages, three pods, three throttle rows — and records
(case, return code, the engine the message was recorded on, the message).  The result is compared with
tests/golden/query_refusal_messages.json, which was recorded from the library as it was before the queries' host code was folded
into shared helpers and is never rewritten by a test run (``PYTHONPATH=. python tests/test_query_refusal_messages_gpu.py``, from
the repository root, writes it).

Every case is a refusal on the host or a plain successful call.  Which engine holds a message is found by leaving a mark — the
text of a refused kt_fetch_reserved — on every engine of the call first: the one whose text is no longer the mark."""
import json
import os

import numpy as np
import pytest

import forecast_reference as FR
import preempt_reference as PR
from kube_throttler_amd import engine as E

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query_refusal_messages.json")
NOW = PR.NOW
LATER = (NOW[0] + 60, 0)
INST = [NOW, LATER]
MARK = "throttle row -1"
M, OFF, CANDS = [0, 1], [0, 2], [2]  # two pending pods as one gang, the running pod as the candidate
T_BIG = 1030
BIG = 2**31 // T_BIG + 1             # so many rows x T_BIG throttle rows are beyond 2^31 matrix bytes
MANY = 2**16 + 1                     # so many rows (or gangs of one) x 2^15 instants are beyond 2^31 verdict bytes


def _seconds(m):
    return [(NOW[0] + k, 0) for k in range(m)]


def _mark(e):
    try:
        e.fetch_reserved(rows=[-1])
    except E.EngineError:
        pass


def _last(e):
    return E.lib().kt_last_error(e._h).decode()


class Log:
    def __init__(self, names):
        self.names = names  # id(engine) -> name
        self.entries = {}

    def __call__(self, entry_point, case, engines, fn):
        """Run fn over ``engines`` (one engine, or the pages in order) -> its code, and where which message was left."""
        engines = engines if isinstance(engines, (list, tuple)) else [engines]
        for e in engines:
            _mark(e)
        try:
            r = fn()
            code = r if isinstance(r, int) else 0
        except E.EngineError as x:
            code = x.code
        left = [[self.names[id(e)], _last(e)] for e in {id(e): e for e in engines}.values() if _last(e) != MARK]
        self.entries.setdefault(entry_point, []).append({"case": case, "code": code, "messages": left})


def _engine_cases(log, ep, call, page1, engs, inc, paged):
    """The refusals about an engine that the preempt and forecast families share: ``call(pages)`` is a valid query over the
    engines ``pages`` (one engine for the single-engine entry points)."""
    pages = (lambda last: [engs[0], last]) if paged else (lambda last: [last])
    log(ep, "incremental engine", pages(inc), lambda: call(pages(inc)))
    page1.set_exchange_world(2)
    log(ep, "exchange world 2", pages(page1), lambda: call(pages(page1)))
    page1.set_exchange_world(1)
    page1.set_wide_sums(1)
    log(ep, "wide sums found by the probe", pages(page1), lambda: call(pages(page1)))
    log(ep, "wide sums known", pages(page1), lambda: call(pages(page1)))
    page1.set_wide_sums(0)
    log(ep, "ok", pages(page1), lambda: call(pages(page1)))


def walk():
    flags = [PR.PENDING, PR.PENDING, PR.COUNTED]
    tiny = lambda reqs, **kw: PR.tiny(reqs, {0: 10}, flags=flags, D=1, **kw)
    snaps = [tiny([{0: 3}, {0: 3}, {0: 4}], T=3, row=2), tiny([{0: 2}, {0: 2}, {0: 5}], T=3, row=2)]
    engs = [E.Engine.for_snapshot(s) for s in snaps]
    other = E.Engine.for_snapshot(tiny([{0: 1}] * 3, T=2, row=1))
    inc = E.Engine.for_snapshot(snaps[1], kernel_variant=E.VARIANT_INDEXED | E.VARIANT_INCREMENTAL)
    neg = E.Engine.for_snapshot(tiny([{0: 3}, {0: -3}, {0: 4}], T=3, row=2))
    wide = E.Engine.for_snapshot(snaps[1])
    fresh = E.Engine.for_snapshot(snaps[0])
    big = [E.Engine.for_snapshot(FR._run({0: 10}, T=T_BIG, row=T_BIG - 1)) for _ in range(2)]
    everyone = {"page0": engs[0], "page1": engs[1], "other": other, "inc": inc, "neg": neg, "wide": wide, "fresh": fresh,
                "big0": big[0], "big1": big[1]}
    log = Log({id(e): k for k, e in everyone.items()})
    L = E.lib()
    hs = (E.C.c_void_p * 2)(*[e._h for e in engs])
    ptr = lambda a: a.ctypes.data
    one, two = np.array([0], np.int64), np.array([2], np.int64)
    big_rows, big_off = np.zeros(BIG, np.int64), np.arange(BIG + 1, dtype=np.int64)
    many_rows, many_off = np.zeros(MANY, np.int64), np.arange(MANY + 1, dtype=np.int64)
    e0 = engs[0]
    try:
        wide.set_wide_sums(1)
        wide.reconcile(NOW, apply=False)

        # ---- kt_headroom_launch / kt_paged_headroom
        ep = "kt_headroom_launch"
        log(ep, "cap 0", e0, lambda: e0.headroom_launch(2, M, cap=0))
        log(ep, "cap beyond the maximum", e0, lambda: e0.headroom_launch(2, M, cap=1 << 31))
        log(ep, "pod row out of range", e0, lambda: e0.headroom_launch(2, [0, 99], cap=4))
        log(ep, "wide used", wide, lambda: wide.headroom_launch(2, M, cap=4))
        log(ep, "matrix beyond 2^31", big[0], lambda: big[0].headroom_launch(BIG, big_rows, cap=4))
        log(ep, "ok", e0, lambda: e0.headroom_launch(2, M, cap=4))
        ep = "kt_paged_headroom"
        ph = lambda pages, rows=M, cap=4: E.paged_headroom(pages, rows, cap)
        log(ep, "cap 0", engs, lambda: ph(engs, cap=0))
        log(ep, "pod row out of range", engs, lambda: ph(engs, [0, 99]))
        log(ep, "negative pod row", engs, lambda: ph(engs, [-1]))
        log(ep, "another throttle-row count", [e0, other], lambda: ph([e0, other]))
        log(ep, "an engine twice", [e0, e0], lambda: ph([e0, e0]))
        log(ep, "wide used on page 1", [e0, wide], lambda: ph([e0, wide]))
        log(ep, "matrix beyond 2^31", big, lambda: ph(big, big_rows))
        log(ep, "ok", engs, lambda: ph(engs))

        # ---- kt_headroom_gangs_launch / kt_paged_headroom_gangs
        ep = "kt_headroom_gangs_launch"
        hg = lambda e, rows=M, off=OFF, cap=4: e.headroom_gangs_launch(rows, off, cap=cap)
        log(ep, "gang_off[0] != 0", e0, lambda: hg(e0, off=[1, 2]))
        log(ep, "an empty gang", e0, lambda: hg(e0, off=[0, 0, 2]))
        log(ep, "a pod twice in one gang", e0, lambda: hg(e0, [0, 1, 0], [0, 3]))
        log(ep, "twice is asked before the range", e0, lambda: hg(e0, [0, 99, 99], [0, 3]))
        log(ep, "pod row out of range", e0, lambda: hg(e0, [0, 99]))
        log(ep, "cap 0", e0, lambda: hg(e0, cap=0))
        log(ep, "matrix beyond 2^31", big[0], lambda: hg(big[0], big_rows, big_off))
        log(ep, "wide used", wide, lambda: hg(wide))
        log(ep, "negative request", neg, lambda: hg(neg))
        log(ep, "ok", e0, lambda: hg(e0))
        ep = "kt_paged_headroom_gangs"
        phg = lambda pages, rows=M, off=OFF, cap=4: E.paged_headroom_gangs(pages, rows, off, cap)
        log(ep, "pod_rows missing", engs, lambda: L.kt_paged_headroom_gangs(hs, 2, 2, None, 1, ptr(np.array(OFF, np.int64)), 0, 4, None, None, None))
        log(ep, "gang_off[0] != 0", engs, lambda: phg(engs, off=[1, 2]))
        log(ep, "a pod twice in one gang", engs, lambda: phg(engs, [0, 1, 0], [0, 3]))
        log(ep, "cap 0", engs, lambda: phg(engs, cap=0))
        log(ep, "pod row out of range", engs, lambda: phg(engs, [0, 99]))
        log(ep, "another throttle-row count", [e0, other], lambda: phg([e0, other]))
        log(ep, "an engine twice", [e0, e0], lambda: phg([e0, e0]))
        log(ep, "matrix beyond 2^31", big, lambda: phg(big, big_rows, big_off))
        log(ep, "wide used on page 1", [e0, wide], lambda: phg([e0, wide]))
        log(ep, "negative request on page 1", [e0, neg], lambda: phg([e0, neg], [0], [0, 1]))
        log(ep, "ok", engs, lambda: phg(engs))

        # ---- kt_preempt_launch and its reprieve twin / kt_paged_preempt
        for ep, reprieve in (("kt_preempt_launch", False), ("kt_preempt_reprieve_launch", True)):
            pl = lambda e, rows=[0], cands=CANDS, r=reprieve: (e.preempt_reprieve_launch if r else e.preempt_launch)(rows, cands, NOW)
            log(ep, "preemptor row out of range", e0, lambda: pl(e0, [99]))
            log(ep, "candidate row out of range", e0, lambda: pl(e0, [0], [99]))
            log(ep, "a candidate twice", e0, lambda: pl(e0, [0], [2, 1, 2]))
            log(ep, "a preemptor and a candidate", e0, lambda: pl(e0, [0, 2], [2]))
            log(ep, "matrix beyond 2^31", big[0], lambda: pl(big[0], big_rows, []))
            _engine_cases(log, ep, lambda pages: pl(pages[0]), engs[0], engs, inc, paged=False)
        ep = "kt_paged_preempt"
        pp = lambda pages, rows=[0], cands=CANDS, **kw: E.paged_preempt(pages, rows, cands, NOW, **kw)
        log(ep, "unknown flags", engs, lambda: L.kt_paged_preempt(hs, 2, 1, ptr(one), 1, ptr(two), NOW[0], NOW[1], 0, 0x4, None, None))
        log(ep, "cand_rows missing", engs, lambda: L.kt_paged_preempt(hs, 2, 1, ptr(one), 1, None, NOW[0], NOW[1], 0, 0, None, None))
        log(ep, "preemptor row out of range", engs, lambda: pp(engs, [99]))
        log(ep, "candidate row out of range", engs, lambda: pp(engs, [0], [99]))
        log(ep, "another throttle-row count", [e0, other], lambda: pp([e0, other]))
        log(ep, "an engine twice", [e0, e0], lambda: pp([e0, e0]))
        log(ep, "matrix beyond 2^31", big, lambda: pp(big, big_rows, []))
        log(ep, "a candidate twice", engs, lambda: pp(engs, [0], [2, 1, 2]))
        log(ep, "a preemptor and a candidate", engs, lambda: pp(engs, [0, 2], [2]))
        _engine_cases(log, ep, lambda pages: pp(pages), engs[1], engs, inc, paged=True)
        log(ep, "ok with reprieve", engs, lambda: pp(engs, reprieve=True))

        # ---- kt_preempt_gangs_launch and its reprieve twin / kt_paged_preempt_gangs
        for ep, reprieve in (("kt_preempt_gangs_launch", False), ("kt_preempt_gangs_reprieve_launch", True)):
            pg = lambda e, rows=M, off=OFF, cands=CANDS, r=reprieve: (e.preempt_gangs_reprieve_launch if r else e.preempt_gangs_launch)(rows, off, cands, NOW)
            log(ep, "gang_off[n_gangs] != n", e0, lambda: pg(e0, off=[0, 1]))
            log(ep, "member row out of range", e0, lambda: pg(e0, [0, 99]))
            log(ep, "candidate row out of range", e0, lambda: pg(e0, cands=[99]))
            log(ep, "a candidate twice", e0, lambda: pg(e0, [0], [0, 1], [2, 1, 2]))
            log(ep, "a member and a candidate", e0, lambda: pg(e0, [0, 2], [0, 2], [2]))
            log(ep, "a pod twice in one gang", e0, lambda: pg(e0, [0, 1, 0], [0, 3]))
            log(ep, "matrix beyond 2^31", big[0], lambda: pg(big[0], big_rows, big_off, []))
            _engine_cases(log, ep, lambda pages: pg(pages[0]), engs[0], engs, inc, paged=False)
        ep = "kt_paged_preempt_gangs"
        ppg = lambda pages, rows=M, off=OFF, cands=CANDS, **kw: E.paged_preempt_gangs(pages, rows, off, cands, NOW, **kw)
        off1 = np.array([0, 1], np.int64)
        log(ep, "unknown flags", engs, lambda: L.kt_paged_preempt_gangs(hs, 2, 1, ptr(one), 1, ptr(off1), 1, ptr(two), NOW[0], NOW[1], 0, 0x4, None, None, None))
        log(ep, "gang_off[n_gangs] != n", engs, lambda: ppg(engs, off=[0, 1]))
        log(ep, "cand_rows missing", engs, lambda: L.kt_paged_preempt_gangs(hs, 2, 1, ptr(one), 1, ptr(off1), 1, None, NOW[0], NOW[1], 0, 0, None, None, None))
        log(ep, "member row out of range", engs, lambda: ppg(engs, [0, 99]))
        log(ep, "candidate row out of range", engs, lambda: ppg(engs, cands=[99]))
        log(ep, "another throttle-row count", [e0, other], lambda: ppg([e0, other]))
        log(ep, "an engine twice", [e0, e0], lambda: ppg([e0, e0]))
        log(ep, "a candidate twice", engs, lambda: ppg(engs, [0], [0, 1], [2, 1, 2]))
        log(ep, "a member and a candidate", engs, lambda: ppg(engs, [0, 2], [0, 2], [2]))
        log(ep, "a pod twice in one gang", engs, lambda: ppg(engs, [0, 1, 0], [0, 3]))
        log(ep, "matrix beyond 2^31", big, lambda: ppg(big, big_rows, big_off, []))
        _engine_cases(log, ep, lambda pages: ppg(pages), engs[1], engs, inc, paged=True)
        log(ep, "ok with reprieve", engs, lambda: ppg(engs, reprieve=True))

        # ---- kt_forecast_launch / kt_paged_forecast, kt_headroom_forecast_launch
        def instants_cases(ep, engines, call):
            log(ep, "no instants", engines, lambda: call([]))
            log(ep, "instants not strictly ascending", engines, lambda: call([NOW, NOW]))
            log(ep, "instants descending in the nanoseconds", engines, lambda: call([(NOW[0], 5), (NOW[0], 4)]))
            log(ep, "inst_ns beyond a second", engines, lambda: call([(NOW[0], 1_000_000_000)]))
            log(ep, "inst_ns negative", engines, lambda: call([(NOW[0], -1)]))

        ep = "kt_forecast_launch"
        fl = lambda e, rows=M, inst=INST: e.forecast_launch(rows, inst)
        instants_cases(ep, e0, lambda inst: fl(e0, inst=inst))
        log(ep, "pod row out of range", e0, lambda: fl(e0, [0, 99]))
        log(ep, "matrix beyond 2^31", big[0], lambda: fl(big[0], big_rows, [NOW]))
        log(ep, "verdicts beyond 2^31", e0, lambda: fl(e0, many_rows, _seconds(2**15)))
        _engine_cases(log, ep, lambda pages: fl(pages[0]), engs[0], engs, inc, paged=False)
        ep = "kt_paged_forecast"
        pf = lambda pages, rows=M, inst=INST: E.paged_forecast(pages, rows, inst)
        instants_cases(ep, engs, lambda inst: pf(engs, inst=inst))
        log(ep, "pod row out of range", engs, lambda: pf(engs, [0, 99]))
        log(ep, "another throttle-row count", [e0, other], lambda: pf([e0, other]))
        log(ep, "an engine twice", [e0, e0], lambda: pf([e0, e0]))
        log(ep, "matrix beyond 2^31", big, lambda: pf(big, big_rows, [NOW]))
        log(ep, "verdicts beyond 2^31", engs, lambda: pf(engs, many_rows, _seconds(2**15)))
        _engine_cases(log, ep, lambda pages: pf(pages), engs[1], engs, inc, paged=True)
        ep = "kt_headroom_forecast_launch"
        hf = lambda e, rows=M, inst=INST, cap=4, want=1: e.headroom_forecast_launch(rows, inst, cap, want)
        instants_cases(ep, e0, lambda inst: hf(e0, inst=inst))
        log(ep, "cap 0", e0, lambda: hf(e0, cap=0))
        log(ep, "want 0", e0, lambda: hf(e0, want=0))
        log(ep, "want beyond cap", e0, lambda: hf(e0, want=5))
        log(ep, "pod row out of range", e0, lambda: hf(e0, [0, 99]))
        log(ep, "matrix beyond 2^31", big[0], lambda: hf(big[0], big_rows, [NOW]))
        log(ep, "results beyond 2^31", e0, lambda: hf(e0, many_rows, _seconds(2**15)))
        _engine_cases(log, ep, lambda pages: hf(pages[0]), engs[0], engs, inc, paged=False)

        # ---- kt_forecast_gangs_launch / kt_paged_forecast_gangs
        ep = "kt_forecast_gangs_launch"
        fg = lambda e, rows=M, off=OFF, inst=INST: e.forecast_gangs_launch(rows, off, inst)
        instants_cases(ep, e0, lambda inst: fg(e0, inst=inst))
        log(ep, "the instants come before a broken gang_off", e0, lambda: fg(e0, off=[0, 1], inst=[LATER, NOW]))
        log(ep, "descending gang_off", e0, lambda: fg(e0, off=[0, 2, 1]))
        log(ep, "a pod twice in one gang", e0, lambda: fg(e0, [0, 1, 0], [0, 3]))
        log(ep, "twice is asked before the range", e0, lambda: fg(e0, [0, 99, 99], [0, 3]))
        log(ep, "pod row out of range", e0, lambda: fg(e0, [0, 99]))
        log(ep, "matrix beyond 2^31", big[0], lambda: fg(big[0], big_rows, big_off, [NOW]))
        log(ep, "verdicts beyond 2^31", e0, lambda: fg(e0, many_rows, many_off, _seconds(2**15)))
        _engine_cases(log, ep, lambda pages: fg(pages[0]), engs[0], engs, inc, paged=False)
        ep = "kt_paged_forecast_gangs"
        pfg = lambda pages, rows=M, off=OFF, inst=INST: E.paged_forecast_gangs(pages, rows, off, inst)
        instants_cases(ep, engs, lambda inst: pfg(engs, inst=inst))
        log(ep, "the instants come before a broken gang_off", engs, lambda: pfg(engs, off=[0, 1], inst=[LATER, NOW]))
        log(ep, "descending gang_off", engs, lambda: pfg(engs, off=[0, 2, 1]))
        log(ep, "a pod twice in one gang", engs, lambda: pfg(engs, [0, 1, 0], [0, 3]))
        log(ep, "twice is asked before the range", engs, lambda: pfg(engs, [0, 99, 99], [0, 3]))
        log(ep, "pod row out of range", engs, lambda: pfg(engs, [0, 99]))
        log(ep, "another throttle-row count", [e0, other], lambda: pfg([e0, other]))
        log(ep, "an engine twice", [e0, e0], lambda: pfg([e0, e0]))
        log(ep, "matrix beyond 2^31", big, lambda: pfg(big, big_rows, big_off, [NOW]))
        log(ep, "verdicts beyond 2^31", engs, lambda: pfg(engs, many_rows, many_off, _seconds(2**15)))
        _engine_cases(log, ep, lambda pages: pfg(pages), engs[1], engs, inc, paged=True)

        # ---- the six fetches: before any launch, and n beyond the last launch
        f = fresh
        fetches = [
            ("kt_headroom_fetch", lambda n: f.headroom_fetch(n), lambda: f.headroom_launch(2, M, cap=4)),
            ("kt_headroom_gangs_fetch", lambda n: f.headroom_gangs_fetch(n), lambda: f.headroom_gangs_launch(M, OFF, cap=4)),
            ("kt_preempt_fetch", lambda n: f.preempt_fetch(n, 1), lambda: f.preempt_launch(M, CANDS, NOW)),
            ("kt_preempt_gangs_fetch", lambda n: f.preempt_gangs_fetch(n, 1), lambda: f.preempt_gangs_launch(M, OFF, CANDS, NOW)),
            ("kt_forecast_fetch", lambda n: f.forecast_fetch(n, 2), lambda: f.forecast_launch(M, INST)),
            ("kt_forecast_gangs_fetch", lambda n: f.forecast_gangs_fetch(n, 2), lambda: f.forecast_gangs_launch(M, OFF, INST)),
            ("kt_headroom_forecast_fetch", lambda n: f.headroom_forecast_fetch(n, 2), lambda: f.headroom_forecast_launch(M, INST, 4)),
        ]
        for ep, fetch, launch in fetches:
            log(ep, "fetch before launch", f, lambda: fetch(1))
        for ep, fetch, launch in fetches:
            launch()
            log(ep, "n beyond the last launch", f, lambda: fetch(3))
            log(ep, "negative n", f, lambda: fetch(-1))
            log(ep, "ok", f, lambda: fetch(1))
        # a pending result of the other kind is not this fetch's
        f.headroom_gangs_launch(M, OFF, cap=4)
        log("kt_headroom_fetch", "a gang result is pending", f, lambda: f.headroom_fetch(1))
        f.preempt_gangs_launch(M, OFF, CANDS, NOW)
        log("kt_preempt_fetch", "a gang result is pending", f, lambda: f.preempt_fetch(1, 1))
        f.headroom_forecast_launch(M, INST, 4)
        log("kt_forecast_fetch", "a headroom forecast is pending", f, lambda: f.forecast_fetch(1, 2))
        log("kt_forecast_gangs_fetch", "a headroom forecast is pending", f, lambda: f.forecast_gangs_fetch(1, 2))
    finally:
        for e in everyone.values():
            e.close()
    return log.entries


@pytest.fixture(scope="module")
def walked():
    return walk()


WANT = {}
if os.path.exists(GOLDEN):  # (absent only while it is being recorded)
    with open(GOLDEN) as _f:
        WANT = json.load(_f)


def test_the_walk_covers_what_the_golden_covers(walked):
    assert sorted(walked) == sorted(WANT)


@pytest.mark.parametrize("entry_point", sorted(WANT))
def test_codes_and_messages_are_the_recorded_ones(walked, entry_point):
    got, want = walked[entry_point], WANT[entry_point]
    assert [g["case"] for g in got] == [w["case"] for w in want]
    for g, w in zip(got, want):
        assert g == w, f"{entry_point}, {g['case']}: {g} != {w}"


if __name__ == "__main__":
    entries = walk()
    with open(GOLDEN, "w") as out:
        json.dump(entries, out, indent=1, sort_keys=True)
        out.write("\n")
    print(f"{sum(len(v) for v in entries.values())} cases of {len(entries)} entry points -> {GOLDEN}")
