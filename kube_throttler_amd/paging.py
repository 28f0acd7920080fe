"""More resource names than one engine has dimensions (KT_MAX_DIMS = 16): pages.

The reference sums and compares ANY resource name (pkg/resourcelist/resourcelist.go:27-54, resource_amount.go:127-159).
``ClusterState.build_pages()`` builds the same cluster once per page of <= 16 names; one engine evaluates each page and
this module combines the results.  The combination is exact, not a heuristic: every step of ``CheckThrottledFor``
(throttle_types.go:128-153) is ``count part  OR  exists a resource name ...`` — the count part depends on no resource
name, so every page computes it alike, and the name part of the whole cluster is the OR of the pages' name parts.  Hence
    exceeds      <=> some page says exceeds
    active       <=> no page says exceeds, some page says active
    insufficient <=> no page says exceeds or active, some page says insufficient
and a pod-level Error (selector / namespace) shows in every page.  ``used``, ``calculatedThreshold`` and ``throttled`` of
a reconcile are per resource name — each name comes from the page that owns it — while pod counts, the pod flag and the
next-override instant are the same in every page; ``calculatedThreshold`` counts as replaced when any page replaced it.
"""
from __future__ import annotations

import numpy as np

from . import engine as E
from . import snapshot as S

# CheckThrottleStatus precedence of throttle_types.go:128-153 (first hit wins): exceeds > active > insufficient
_RANK = np.zeros(256, dtype=np.uint8)
_RANK[S.NOT_AFFECTED], _RANK[S.NOT_THROTTLED], _RANK[S.INSUFFICIENT], _RANK[S.ACTIVE], _RANK[S.EXCEEDS] = 0, 1, 2, 3, 4
_RANK[255] = 5  # pod-level error
_CODE = np.array([S.NOT_AFFECTED, S.NOT_THROTTLED, S.INSUFFICIENT, S.ACTIVE, S.EXCEEDS, 255], dtype=np.uint8)


def combine_status(matrices) -> np.ndarray:
    """Status matrices [n][T] of the pages -> the cluster's."""
    rank = _RANK[np.asarray(matrices[0])]
    for m in matrices[1:]:
        rank = np.maximum(rank, _RANK[np.asarray(m)])
    return _CODE[rank]


def verdicts(status: np.ndarray) -> np.ndarray:
    """PreFilter verdict per pod from its status row (plugin.go:177-214): error, block, or allow."""
    err = (status == 255).any(axis=1)
    blocked = ((status == S.EXCEEDS) | (status == S.ACTIVE) | (status == S.INSUFFICIENT)).any(axis=1)
    return np.where(err, S.VERDICT_ERROR, np.where(blocked, S.VERDICT_BLOCK, S.VERDICT_ALLOW)).astype(np.uint8)


def combine_reconcile(pages, results) -> list:
    """Per throttle row one dict: used / calc (resourceCounts?, resourceRequests by name), throttled (pod flag + by name),
    calc_updated, error — from the pages' reconcile results (rows aligned: every page holds every throttle)."""
    T = len(pages[0].thr_names)
    out = []
    for i in range(T):
        used, calc, thr_by_name = {}, {}, {}
        for b, r in zip(pages, results):
            for dst, tab in ((used, r.used), (calc, r.calc)):
                d = b.amount_to_dict(tab, i)
                if "resourceCounts" in d:
                    dst["resourceCounts"] = d["resourceCounts"]
                if "resourceRequests" in d:
                    dst.setdefault("resourceRequests", {}).update(d["resourceRequests"])
            for name, dim in b.dims.items():
                if int(r.thrl_has[i]) >> dim & 1:
                    thr_by_name[name] = bool(int(r.thrl_flag[i]) >> dim & 1)
        out.append({"used": used, "calc": calc, "throttled": (bool(results[0].thrl_pod[i]), thr_by_name),
                    "calc_updated": any(bool(r.calc_updated[i]) for r in results),
                    "error": any(bool(r.error[i]) for r in results)})
    return out


def status_manifest(pages, results, i, now_text: str, previous: dict | None = None) -> dict:
    """``status`` of throttle row ``i`` after a paged reconcile, as UpdateStatus would write it (see
    BuiltState.status_manifest): the resource names of all pages in one document."""
    docs = [b.status_manifest(r, i, now_text, previous=None) for b, r in zip(pages, results)]
    st = dict(previous or {})
    used = {}
    for d in docs:
        if "resourceCounts" in d["used"]:
            used["resourceCounts"] = d["used"]["resourceCounts"]
        if "resourceRequests" in d["used"]:
            used.setdefault("resourceRequests", {}).update(d["used"]["resourceRequests"])
    st["used"] = used
    if any(bool(r.calc_updated[i]) for r in results):  # replaced as a whole: every page contributes its names
        thr = {}
        for b, r in zip(pages, results):
            a = b.amount_to_manifest(r.calc, i)
            if "resourceCounts" in a:
                thr["resourceCounts"] = a["resourceCounts"]
            if "resourceRequests" in a:
                thr.setdefault("resourceRequests", {}).update(a["resourceRequests"])
        st["calculatedThreshold"] = {"threshold": thr, "calculatedAt": now_text, "messages": list(pages[0].thr_messages[i])}
    else:
        st.setdefault("calculatedThreshold", {})
    throttled = {"resourceCounts": docs[0]["throttled"]["resourceCounts"], "resourceRequests": {}}
    for d in docs:
        throttled["resourceRequests"].update(d["throttled"]["resourceRequests"])
    st["throttled"] = throttled
    return st


# ---- headroom: how many copies of a pod the throttles still admit (kt_paged_headroom), restated over the pages' snapshots
def _pool_arrays(pool):
    return pool.arrays() if hasattr(pool, "arrays") else (pool.op, pool.key, pool.val_off, pool.val)


def _selector_matches(pool, r0, r1, keys, pairs) -> bool:
    """labels.Requirement.Matches over requirements [r0, r1) of a pool (the conjunction; an empty selector matches)."""
    op, key, val_off, val = _pool_arrays(pool)
    for r in range(r0, r1):
        has = int(key[r]) in keys
        hit = has and any(int(v) in pairs for v in val[int(val_off[r]):int(val_off[r + 1])])
        o = int(op[r])
        if not {S.OP_IN: hit, S.OP_NOT_IN: not hit, S.OP_EXISTS: has, S.OP_DOES_NOT_EXIST: not has}.get(o, False):
            return False
    return True


def affected_throttles(snap, p):
    """(error, ascending throttle rows) — the throttles PreFilter evaluates for pod row ``p``: affectedThrottles
    (throttle_controller.go:248-269), then affectedClusterThrottles (clusterthrottle_controller.go:272-298: the namespace
    object must exist); a selector that does not convert, reached before a term matched, is an error (plugin.go:154-168)."""
    ns = int(snap.pod_ns[p])
    l0, l1 = int(snap.pod_label_off[p]), int(snap.pod_label_off[p + 1])
    keys = {int(k) for k in snap.pod_label_key[l0:l1]}
    pairs = {int(k) for k in snap.pod_label_pair[l0:l1]}
    need = S.THR_VALID | S.THR_RESPONSIBLE
    ns_ok = ns < snap.n_ns and bool(snap.ns_valid[ns])
    if ns_ok:
        n0, n1 = int(snap.ns_label_off[ns]), int(snap.ns_label_off[ns + 1])
        ns_keys = {int(k) for k in snap.ns_label_key[n0:n1]}
        ns_pairs = {int(k) for k in snap.ns_label_pair[n0:n1]}
    out = []
    for cluster in (False, True):
        if cluster and not ns_ok:
            return True, []
        for t in range(snap.n_thr):
            f = int(snap.thr_flags[t])
            if (f & need) != need or bool(f & S.THR_CLUSTER) != cluster or (not cluster and int(snap.thr_ns[t]) != ns):
                continue
            for g in range(int(snap.thr_term_off[t]), int(snap.thr_term_off[t + 1])):
                tf = int(snap.term_flags[g])
                if cluster and ((tf & S.TERM_NS_SEL_INVALID) or not _selector_matches(
                        snap.nreq, int(snap.term_nreq_off[g]), int(snap.term_nreq_off[g + 1]), ns_keys, ns_pairs)):
                    continue  # (the namespace side swallows a conversion error: clusterthrottle_selector.go:63-69)
                if tf & S.TERM_POD_SEL_INVALID:
                    return True, []
                if _selector_matches(snap.preq, int(snap.term_preq_off[g]), int(snap.term_preq_off[g + 1]), keys, pairs):
                    out.append(t)
                    break
    return False, sorted(out)


def pod_requests(snap, p):
    """ResourceAmountOfPod's requests of pod row ``p`` over the snapshot's names (resourcelist.go:27-46): max(init containers)
    against sum(containers), plus overhead -> {dim: value}; a name is present when any of them names it."""
    init, run = {}, {}
    for c in range(int(snap.pod_ctr_off[p]), int(snap.pod_ctr_off[p + 1])):
        for d in range(snap.D):
            if int(snap.ctr_present[c]) >> d & 1:
                v = int(snap.ctr_req[c, d])
                if snap.ctr_init[c]:
                    init[d] = max(init[d], v) if d in init else v
                else:
                    run[d] = run.get(d, 0) + v
    for d, v in init.items():
        run[d] = max(run[d], v) if d in run else v
    if int(snap.pod_ovh_present[p]) >> 31:
        for d in range(snap.D):
            if int(snap.pod_ovh_present[p]) >> d & 1:
                run[d] = run.get(d, 0) + int(snap.pod_ovh[p, d])
    return run


def _copies_of_amount(v, brings, th_has, tv, uv, rv, present0, flagged, eq3, eq, cap) -> int:
    """The leading copies of a run of identical pods that ONE amount of one throttle lets through (a resource name with
    request ``v``, or the pod count with ``v`` = 1): copy j is checked against used + reserved + j * v by the four steps of
    CheckThrottledFor (throttle_types.go:128-153), and from copy 1 on the amount is present because the pod brought it in."""
    va = v if brings else 0

    def passes(j):
        if flagged:  # step 2
            return False
        if not th_has:
            return True
        if v > tv:  # step 1
            return False
        s = uv + rv + j * va
        if (present0 or (j > 0 and brings)) and (s >= tv if eq3 else s > tv):  # step 3
            return False
        return not (s + v >= tv if eq else s + v > tv)  # step 4

    if not passes(0):
        return 0
    if not th_has or va <= 0:  # the sums do not grow: copies 1.. fare as copy 1 does, or better
        return cap if passes(1) else 1
    # the sums grow: step 4 of a copy implies its step 3, the copies that pass are those with s + (j + 1) v < (<=) tv
    return max(0, min(cap, (tv - uv - rv - (1 if eq else 0)) // v))


def headroom_of(pages, pod_row, cap, on_equal=False):
    """kt_paged_headroom for one pod, in closed form over the page bundles' snapshots (no GPU): the number of leading
    Success verdicts a dry-run admission of ``[pod] * cap`` returns — the minimum over the affecting throttles, and there over
    the pod count and every requested resource name of every page, of the copies that amount alone lets through — and the
    lowest throttle row that stops the next copy (-1 when all ``cap`` are admitted) -> (copies, limiting)."""
    snap0 = pages[0].snapshot
    p = int(pod_row)
    if not (0 <= p < snap0.n_pods) or not int(snap0.pod_flags[p]) & S.POD_VALID:
        return 0, -1
    err, affected = affected_throttles(snap0, p)
    if err:
        return 0, -1
    eq = bool(on_equal)
    reqs = [pod_requests(b.snapshot, p) for b in pages]
    best, limiting = cap, -1
    for t in affected:
        f = int(snap0.thr_flags[t])
        eq3 = eq if f & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
        th = snap0.thr_calc if f & S.THR_CALC_AT_NONZERO else snap0.thr_spec
        u_hc, r_hc = bool(snap0.thr_used.has_count[t]), bool(snap0.thr_reserved.has_count[t])
        h = _copies_of_amount(1, True, bool(th.has_count[t]), int(th.count[t]), int(snap0.thr_used.count[t]) if u_hc else 0,
                              int(snap0.thr_reserved.count[t]) if r_hc else 0, u_hc or r_hc, bool(f & S.THR_THROTTLED_POD), eq3, eq, cap)
        for b, req in zip(pages, reqs):
            s = b.snapshot
            th = s.thr_calc if int(s.thr_flags[t]) & S.THR_CALC_AT_NONZERO else s.thr_spec
            for d, v in req.items():
                if v == 0:
                    continue  # a name the pod does not request (rq.IsZero(), resource_amount.go:46-65)
                bit = lambda w: bool(int(w) >> d & 1)
                u_p, r_p = bit(s.thr_used.present[t]), bit(s.thr_reserved.present[t])
                h = min(h, _copies_of_amount(v, True, bit(th.present[t]), int(th.v[t, d]), int(s.thr_used.v[t, d]) if u_p else 0,
                                             int(s.thr_reserved.v[t, d]) if r_p else 0, u_p or r_p,
                                             bit(int(s.thr_thrl_flag[t]) & int(s.thr_thrl_has[t])), eq3, eq, cap))
        if h < best:
            best, limiting = h, t
    return best, limiting


# ---- preempt: the shortest victim prefix that lets a blocked pod through (kt_preempt_launch), in closed form on a Snapshot ----
_COUNTABLE = S.POD_VALID | S.POD_SCHED_MATCH | S.POD_SCHEDULED


def _throttle_walk(snap, t, p):
    """(matched, error) of throttle row ``t``'s selector on pod row ``p``: terms in order, the first match wins, a podSelector
    that does not convert and is reached before a match is an error (throttle_selector.go:30-54,
    clusterthrottle_selector.go:44-87)."""
    f = int(snap.thr_flags[t])
    need = S.THR_VALID | S.THR_RESPONSIBLE
    if (f & need) != need:
        return False, False
    ns = int(snap.pod_ns[p])
    cluster = bool(f & S.THR_CLUSTER)
    if cluster:
        if not (ns < snap.n_ns and bool(snap.ns_valid[ns])):
            return False, False
        n0, n1 = int(snap.ns_label_off[ns]), int(snap.ns_label_off[ns + 1])
        ns_keys = {int(k) for k in snap.ns_label_key[n0:n1]}
        ns_pairs = {int(k) for k in snap.ns_label_pair[n0:n1]}
    elif int(snap.thr_ns[t]) != ns:
        return False, False
    l0, l1 = int(snap.pod_label_off[p]), int(snap.pod_label_off[p + 1])
    keys = {int(k) for k in snap.pod_label_key[l0:l1]}
    pairs = {int(k) for k in snap.pod_label_pair[l0:l1]}
    for g in range(int(snap.thr_term_off[t]), int(snap.thr_term_off[t + 1])):
        tf = int(snap.term_flags[g])
        if cluster and ((tf & S.TERM_NS_SEL_INVALID) or not _selector_matches(
                snap.nreq, int(snap.term_nreq_off[g]), int(snap.term_nreq_off[g + 1]), ns_keys, ns_pairs)):
            continue
        if tf & S.TERM_POD_SEL_INVALID:
            return False, True
        if _selector_matches(snap.preq, int(snap.term_preq_off[g]), int(snap.term_preq_off[g + 1]), keys, pairs):
            return True, False
    return False, False


def _calculated_threshold(snap, t, now):
    """CalculateThreshold(now) of throttle row ``t`` (throttle_types.go:65-106): the first active override wins per resource
    name and for the pod count, and the merged override REPLACES spec.threshold -> ({dim: value}, count or None, parse error)."""
    now = (int(now[0]), int(now[1]))
    names, count, active, any_err = {}, None, False, False
    for o in range(int(snap.thr_ovr_off[t]), int(snap.thr_ovr_off[t + 1])):
        if int(snap.ovr_flags[o]) & S.OVR_PARSE_ERROR:
            any_err = True
            continue
        begin = (int(snap.ovr_begin_s[o]), int(snap.ovr_begin_ns[o]))
        end = (int(snap.ovr_end_s[o]), int(snap.ovr_end_ns[o]))
        if not (begin <= now and (end == (S.ZERO_TIME_S, 0) or now <= end)):
            continue
        active = True
        if count is None and snap.ovr_thr.has_count[o]:
            count = int(snap.ovr_thr.count[o])
        for d in range(snap.D):
            if int(snap.ovr_thr.present[o]) >> d & 1 and d not in names:
                names[d] = int(snap.ovr_thr.v[o, d])
    if not active:
        names = {d: int(snap.thr_spec.v[t, d]) for d in range(snap.D) if int(snap.thr_spec.present[t]) >> d & 1}
        count = int(snap.thr_spec.count[t]) if snap.thr_spec.has_count[t] else None
    return names, count, any_err


def _amount_dict(tab, t, D):
    return {d: int(tab.v[t, d]) for d in range(D) if int(tab.present[t]) >> d & 1}, (int(tab.count[t]) if tab.has_count[t] else None)


def preempt_context(snap, now):
    """What every preemptor of one kt_preempt_launch shares: per throttle row the sums of a fresh aggregate (values and
    contributor counts per name, counted pods), whether its reconcile is an error, and the thresholds a check reads behind the
    reconcile at ``now``; per pod row the throttles that match it."""
    D, T = snap.D, snap.n_thr
    match = {}  # pod row -> [throttle rows whose selector matches it]
    thr = [dict(val={}, cnt={}, pods=0, error=False) for _ in range(T)]
    for p in range(snap.n_pods):
        fl = int(snap.pod_flags[p])
        if not fl & S.POD_VALID:
            continue
        req = pod_requests(snap, p)
        rows = []
        for t in range(T):
            m, err = _throttle_walk(snap, t, p)
            if (fl & _COUNTABLE) == _COUNTABLE and err:
                thr[t]["error"] = True
            if m:
                rows.append(t)
                if (fl & _COUNTABLE) == _COUNTABLE and not fl & S.POD_FINISHED:
                    thr[t]["pods"] += 1
                    for d, v in req.items():
                        thr[t]["val"][d] = thr[t]["val"].get(d, 0) + v
                        thr[t]["cnt"][d] = thr[t]["cnt"].get(d, 0) + 1
        match[p] = rows
    for t in range(T):
        f = int(snap.thr_flags[t])
        calc, calc_count, any_err = _calculated_threshold(snap, t, now)
        stored, stored_count = _amount_dict(snap.thr_calc, t, D)
        fp = int(snap.thr_spec_msgs_fp[t]) if any_err else 0
        replace = (calc, calc_count) != (stored, stored_count) or int(snap.thr_status_msgs_fp[t]) != fp
        # threshold := status.calculatedThreshold once calculatedAt is set (the reconcile sets it when it replaces), else spec
        use_calc = bool(f & S.THR_CALC_AT_NONZERO) or replace
        thr[t]["calc"], thr[t]["calc_count"] = calc, calc_count
        thr[t]["th"], thr[t]["th_count"] = (calc, calc_count) if use_calc else _amount_dict(snap.thr_spec, t, D)
    return dict(match=match, thr=thr)


def _amount_fails(vp, th, flagged, u_present, uv, r_present, rv, eq3, eq) -> bool:
    """One amount of one throttle for the pod (a requested resource name, or the pod count with vp = 1): does one of the four
    CheckThrottledFor steps (throttle_types.go:128-153) stop it.  ``th`` None: the threshold does not name the amount."""
    if flagged:  # step 2
        return True
    if th is None:
        return False
    if vp > th:  # step 1
        return True
    s = (uv if u_present else 0) + (rv if r_present else 0)
    if (u_present or r_present) and (s >= th if eq3 else s > th):  # step 3
        return True
    return s + vp >= th if eq else s + vp > th  # step 4


def preempt_of(snap, pod_row, cand_rows, now, on_equal=False, ctx=None, reprieve=False):
    """kt_preempt_launch for one preemptor, in closed form on a Snapshot (no GPU) -> (prefix, victims [len(cand_rows)]).
    prefix: the smallest k for which PreFilter(pod) is Success once the candidates ``cand_rows[:k]`` are gone and every
    responsible throttle has been reconciled at ``now`` (reserved amounts unchanged; a throttle whose reconcile is an error keeps
    its stored status); 0: the pod already passes against a fresh reconcile; -1: no prefix helps.  The list is cut before the
    first candidate whose own PreFilter is an error or whose row is invalid.  victims[j] = 1 iff j < prefix, the candidate is
    counted and a throttle that affects the pod matches it.  Deleting a prefix lowers every `used` by a prefix sum; a name stays
    present only while a remaining counted pod carries it, the pod count only while a pod is counted.
    ``reprieve`` (kt_preempt_reprieve_launch): the masked victims are then put back one by one, the last first, and each stays back
    as long as the pod still passes every affecting throttle; victims is what remains."""
    ctx = preempt_context(snap, now) if ctx is None else ctx
    p, cands, eq = int(pod_row), [int(c) for c in cand_rows], bool(on_equal)
    m = len(cands)
    none = (-1, [0] * m)
    if not (0 <= p < snap.n_pods) or not int(snap.pod_flags[p]) & S.POD_VALID:
        return none
    err, affected = affected_throttles(snap, p)
    if err:
        return none
    m_eff = m
    for j, c in enumerate(cands):
        if not (0 <= c < snap.n_pods) or not int(snap.pod_flags[c]) & S.POD_VALID or affected_throttles(snap, c)[0]:
            m_eff = j
            break
    counted = lambda c: (int(snap.pod_flags[c]) & (_COUNTABLE | S.POD_FINISHED)) == _COUNTABLE
    req = {d: v for d, v in pod_requests(snap, p).items() if v != 0}
    creq = [pod_requests(snap, c) if counted(c) else {} for c in cands[:m_eff]]
    contributes = [[counted(c) and t in ctx["match"].get(c, ()) for c in cands[:m_eff]] for t in affected]
    fails = [False] * (m_eff + 1)  # fails[k]: some (throttle, amount) stops the pod in S_k
    for ti, t in enumerate(affected):
        th = ctx["thr"][t]
        f = int(snap.thr_flags[t])
        eq3 = eq if f & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
        res, res_count = _amount_dict(snap.thr_reserved, t, snap.D)
        if th["error"]:  # the stored status stays, in every S_k: the STORED calculatedThreshold once calculatedAt is set, else spec
            used, used_count = _amount_dict(snap.thr_used, t, snap.D)
            sth, sth_count = _amount_dict(snap.thr_calc if f & S.THR_CALC_AT_NONZERO else snap.thr_spec, t, snap.D)
            flg = int(snap.thr_thrl_flag[t]) & int(snap.thr_thrl_has[t])
            bad = _amount_fails(1, sth_count, bool(f & S.THR_THROTTLED_POD), used_count is not None, used_count or 0,
                                res_count is not None, res_count or 0, eq3, eq)
            for d, v in req.items():
                bad = bad or _amount_fails(v, sth.get(d), bool(flg >> d & 1), d in used, used.get(d, 0), d in res, res.get(d, 0), eq3, eq)
            if bad:
                return none
            continue
        val, cnt, pods = dict(th["val"]), dict(th["cnt"]), th["pods"]
        for k in range(m_eff + 1):
            if k > 0 and contributes[ti][k - 1]:
                pods -= 1
                for d, v in creq[k - 1].items():
                    val[d] -= v
                    cnt[d] -= 1
            u_hc = pods > 0
            cc = th["calc_count"]
            bad = _amount_fails(1, th["th_count"], cc is not None and u_hc and pods >= cc, u_hc, pods, res_count is not None, res_count or 0, eq3, eq)
            for d, v in req.items():
                u_pr = cnt.get(d, 0) > 0
                cv = th["calc"].get(d)
                bad = bad or _amount_fails(v, th["th"].get(d), cv is not None and u_pr and val[d] >= cv, u_pr, val.get(d, 0), d in res,
                                           res.get(d, 0), eq3, eq)
            fails[k] = fails[k] or bad
    prefix = next((k for k in range(m_eff + 1) if not fails[k]), -1)
    victims = [0] * m
    for j in range(max(prefix, 0)):
        victims[j] = int(any(contributes[ti][j] for ti in range(len(affected))))
    if reprieve and prefix > 0:
        _reprieve(snap, ctx, affected, contributes, creq, req, eq, prefix, victims)
    return prefix, victims


def _reprieve(snap, ctx, affected, contributes, creq, req, eq, prefix, victims):
    """The reprieve walk on the sums of ``preempt_context``: per reconciled affecting throttle the `used` of the state without the
    masked victims; position prefix - 1 first, a victim is put back where every throttle that matches it still lets the pod
    through with its amounts added (the others do not change: they pass already).  ``victims`` is rewritten in place."""
    live = []  # [throttle row, its index in `contributes`, values, contributor counts, counted pods]
    for ti, t in enumerate(affected):
        th = ctx["thr"][t]
        if th["error"]:  # keeps its stored status whoever is deleted: it passed, or the prefix would not be positive
            continue
        val, cnt, pods = dict(th["val"]), dict(th["cnt"]), th["pods"]
        for j in range(prefix):
            if victims[j] and contributes[ti][j]:
                pods -= 1
                for d, v in creq[j].items():
                    val[d] -= v
                    cnt[d] -= 1
        live.append([t, ti, val, cnt, pods])
    for j in range(prefix - 1, -1, -1):
        if not victims[j]:
            continue
        back = []
        for entry in live:
            t, ti, val, cnt, pods = entry
            if not contributes[ti][j]:
                continue
            val, cnt, pods = dict(val), dict(cnt), pods + 1
            for d, v in creq[j].items():
                val[d] = val.get(d, 0) + v
                cnt[d] = cnt.get(d, 0) + 1
            th = ctx["thr"][t]
            eq3 = eq if int(snap.thr_flags[t]) & S.THR_CLUSTER else True
            res, res_count = _amount_dict(snap.thr_reserved, t, snap.D)
            cc = th["calc_count"]
            bad = _amount_fails(1, th["th_count"], cc is not None and pods >= cc, True, pods, res_count is not None, res_count or 0, eq3, eq)
            for d, v in req.items():
                u_pr = cnt.get(d, 0) > 0
                cv = th["calc"].get(d)
                bad = bad or _amount_fails(v, th["th"].get(d), cv is not None and u_pr and val.get(d, 0) >= cv, u_pr, val.get(d, 0), d in res,
                                           res.get(d, 0), eq3, eq)
            if bad:
                break
            back.append((entry, val, cnt, pods))
        else:
            victims[j] = 0
            for entry, val, cnt, pods in back:
                entry[2:] = [val, cnt, pods]


# ---- preempt, for gangs: the shortest victim prefix that lets a whole gang in (kt_preempt_gangs_launch), in closed form ----
# ---- preempt over pages (kt_paged_preempt): the closed form over a list of page snapshots ----
def paged_preempt_context(snaps, now):
    """``preempt_context`` of every page, and per throttle row the two facts that hold for the throttle AS A WHOLE:
    ``error`` — its reconcile is an error on some page: it keeps its stored status on every page — and ``use_calc`` —
    status.calculatedThreshold is compared and replaced as a whole (throttle_controller.go:116-133), so the check reads the
    calculated threshold on EVERY page iff on SOME page calculatedAt is set or the reconcile at ``now`` replaces it, and
    spec.threshold on every page otherwise.  ``th`` / ``calc`` are keyed by (page, dim); the pod-count parts are page 0's."""
    ctxs = [preempt_context(s, now) for s in snaps]
    thr = []
    for t in range(snaps[0].n_thr):
        error = any(c["thr"][t]["error"] for c in ctxs)
        use_calc, calcs = False, []
        for s, c in zip(snaps, ctxs):
            calc, calc_count, any_err = _calculated_threshold(s, t, now)
            stored, stored_count = _amount_dict(s.thr_calc, t, s.D)
            fp = int(s.thr_spec_msgs_fp[t]) if any_err else 0
            replace = not c["thr"][t]["error"] and ((calc, calc_count) != (stored, stored_count) or int(s.thr_status_msgs_fp[t]) != fp)
            use_calc = use_calc or bool(int(s.thr_flags[t]) & S.THR_CALC_AT_NONZERO) or replace
            calcs.append((calc, calc_count))
        th, cv, val, cnt = {}, {}, {}, {}
        for k, (s, c) in enumerate(zip(snaps, ctxs)):
            names = calcs[k][0] if use_calc else _amount_dict(s.thr_spec, t, s.D)[0]
            th.update({(k, d): v for d, v in names.items()})
            cv.update({(k, d): v for d, v in calcs[k][0].items()})
            val.update({(k, d): v for d, v in c["thr"][t]["val"].items()})
            cnt.update({(k, d): v for d, v in c["thr"][t]["cnt"].items()})
        th_count = calcs[0][1] if use_calc else _amount_dict(snaps[0].thr_spec, t, snaps[0].D)[1]
        thr.append(dict(error=error, use_calc=use_calc, th=th, th_count=th_count, calc=cv, calc_count=calcs[0][1], val=val, cnt=cnt,
                        pods=ctxs[0]["thr"][t]["pods"]))
    return dict(match=ctxs[0]["match"], thr=thr)


def _paged_amounts(snaps, tab_name, t):
    """A stored amount table's row ``t`` over the pages -> ({(page, dim): value}, page 0's count or None)."""
    names = {}
    for k, s in enumerate(snaps):
        names.update({(k, d): v for d, v in _amount_dict(getattr(s, tab_name), t, s.D)[0].items()})
    return names, _amount_dict(getattr(snaps[0], tab_name), t, snaps[0].D)[1]


def paged_preempt_of(snaps, pod_row, cand_rows, now, on_equal=False, reprieve=False, ctx=None):
    """kt_paged_preempt for one preemptor, in closed form over the page snapshots (no GPU) -> (prefix, victims [len(cand_rows)]):
    ``preempt_of`` on the cluster of all names.  Which pods are counted, which throttles match which pod, the error rows and the
    list cut are page 0's (the selector side is the same in every page); the pod count is judged once; a (throttle, k) pair
    fails iff the count part or some page's name part fails.  The whole-threshold rule: a throttle reads the calculated
    threshold on every page iff some page has calculatedAt set or replaces it at ``now``.  The whole-error rule: a throttle whose
    reconcile is an error on some page keeps its stored status on every page.  With one page this is ``preempt_of``.
    ``reprieve``: the walk of kt_preempt_reprieve_launch with the same joint judge — a victim is put back only if the pod still
    passes every page with it back."""
    snap0 = snaps[0]
    ctx = paged_preempt_context(snaps, now) if ctx is None else ctx
    p, cands, eq = int(pod_row), [int(c) for c in cand_rows], bool(on_equal)
    m = len(cands)
    none = (-1, [0] * m)
    if not (0 <= p < snap0.n_pods) or not int(snap0.pod_flags[p]) & S.POD_VALID:
        return none
    err, affected = affected_throttles(snap0, p)
    if err:
        return none
    m_eff = m
    for j, c in enumerate(cands):
        if not (0 <= c < snap0.n_pods) or not int(snap0.pod_flags[c]) & S.POD_VALID or affected_throttles(snap0, c)[0]:
            m_eff = j
            break
    counted = lambda c: (int(snap0.pod_flags[c]) & (_COUNTABLE | S.POD_FINISHED)) == _COUNTABLE

    def requests(c):
        return {(k, d): v for k, s in enumerate(snaps) for d, v in pod_requests(s, c).items()}

    req = {kd: v for kd, v in requests(p).items() if v != 0}
    creq = [requests(c) if counted(c) else {} for c in cands[:m_eff]]
    contributes = [[counted(c) and t in ctx["match"].get(c, ()) for c in cands[:m_eff]] for t in affected]

    def judge(t, val, cnt, pods):
        th = ctx["thr"][t]
        eq3 = eq if int(snap0.thr_flags[t]) & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
        res, res_count = _paged_amounts(snaps, "thr_reserved", t)
        u_hc, cc = pods > 0, th["calc_count"]
        bad = _amount_fails(1, th["th_count"], cc is not None and u_hc and pods >= cc, u_hc, pods, res_count is not None, res_count or 0, eq3, eq)
        for kd, v in req.items():
            u_pr = cnt.get(kd, 0) > 0
            cv = th["calc"].get(kd)
            bad = bad or _amount_fails(v, th["th"].get(kd), cv is not None and u_pr and val.get(kd, 0) >= cv, u_pr, val.get(kd, 0), kd in res,
                                       res.get(kd, 0), eq3, eq)
        return bad

    def moved(state, j, sign):
        val, cnt, pods = dict(state[0]), dict(state[1]), state[2] + sign
        for kd, v in creq[j].items():
            val[kd] = val.get(kd, 0) + sign * v
            cnt[kd] = cnt.get(kd, 0) + sign
        return [val, cnt, pods]

    fails = [False] * (m_eff + 1)  # fails[k]: some (throttle, amount) of some page stops the pod in S_k
    for ti, t in enumerate(affected):
        th = ctx["thr"][t]
        if th["error"]:  # the stored status stays on every page, in every S_k
            f = int(snap0.thr_flags[t])
            eq3 = eq if f & S.THR_CLUSTER else True
            res, res_count = _paged_amounts(snaps, "thr_reserved", t)
            used, used_count = _paged_amounts(snaps, "thr_used", t)
            sth, sth_count = _paged_amounts(snaps, "thr_calc" if th["use_calc"] else "thr_spec", t)
            bad = _amount_fails(1, sth_count, bool(f & S.THR_THROTTLED_POD), used_count is not None, used_count or 0,
                                res_count is not None, res_count or 0, eq3, eq)
            for (k, d), v in req.items():
                flg = int(snaps[k].thr_thrl_flag[t]) & int(snaps[k].thr_thrl_has[t])
                bad = bad or _amount_fails(v, sth.get((k, d)), bool(flg >> d & 1), (k, d) in used, used.get((k, d), 0), (k, d) in res,
                                           res.get((k, d), 0), eq3, eq)
            if bad:
                return none
            continue
        state = [th["val"], th["cnt"], th["pods"]]
        for k in range(m_eff + 1):
            if k > 0 and contributes[ti][k - 1]:
                state = moved(state, k - 1, -1)
            fails[k] = fails[k] or judge(t, *state)
    prefix = next((k for k in range(m_eff + 1) if not fails[k]), -1)
    victims = [0] * m
    for j in range(max(prefix, 0)):
        victims[j] = int(any(contributes[ti][j] for ti in range(len(affected))))
    if reprieve and prefix > 0:
        live = []  # [index in `contributes`, throttle row, state] of the reconciled affecting throttles, in S(the masked victims)
        for ti, t in enumerate(affected):
            th = ctx["thr"][t]
            if th["error"]:
                continue
            state = [th["val"], th["cnt"], th["pods"]]
            for j in range(prefix):
                if victims[j] and contributes[ti][j]:
                    state = moved(state, j, -1)
            live.append([ti, t, state])
        for j in range(prefix - 1, -1, -1):
            if not victims[j]:
                continue
            back = [(entry, moved(entry[2], j, 1)) for entry in live if contributes[entry[0]][j]]
            if any(judge(entry[1], *state) for entry, state in back):
                continue  # some page of some throttle stops the pod with c_j back: it stays a victim
            victims[j] = 0
            for entry, state in back:
                entry[2] = state
    return prefix, victims


def _gang_first_stopped(members, hit, reqs, thr_amounts, used, res, res_count, eq3, eq):
    """One throttle against one state of its `used`: the position of the first member it affects (``hit``) and stops, every
    earlier member it affects having reserved (None: it stops nobody).  ``thr_amounts``: (threshold names, threshold count);
    ``used``: (count flagged, count present, count, {name: (flagged, present, value)})."""
    (th, th_count), (c_flag, u_hc, u_c, names) = thr_amounts, used
    rv, rp, rc, r_hc = dict(res), set(res), res_count or 0, res_count is not None
    for j in range(len(members)):
        if not hit[j]:
            continue
        bad = _amount_fails(1, th_count, c_flag, u_hc, u_c, r_hc, rc, eq3, eq)
        for d, v in reqs[j].items():
            if v == 0:
                continue
            flagged, u_pr, uv = names.get(d, (False, False, 0))
            bad = bad or _amount_fails(v, th.get(d), flagged, u_pr, uv, d in rp, rv.get(d, 0), eq3, eq)
        if bad:
            return j
        for d, v in reqs[j].items():  # Reserve: every name the pod carries becomes present, zero-valued ones included
            rv[d] = rv.get(d, 0) + v
            rp.add(d)
        rc, r_hc = rc + 1, True
    return None


def _gang_reprieve(snap, ctx, members, union, affected, contributes, creq, reqs, eq, prefix, victims):
    """The reprieve walk for a gang on the sums of ``preempt_context`` — ``_reprieve`` with ``_gang_first_stopped`` as the judge: per
    reconciled throttle of the union the `used` of the state without the masked victims; position prefix - 1 first, a victim is put
    back where every throttle that matches it still admits the members in order, under the reserved prefix, with its amounts added
    (the others do not change: they pass already).  ``victims`` is rewritten in place."""
    live = []  # [throttle row, its index in `contributes`, values, contributor counts, counted pods]
    for ti, t in enumerate(union):
        th = ctx["thr"][t]
        if th["error"]:  # keeps its stored status whoever is deleted: it passed, or the prefix would not be positive
            continue
        val, cnt, pods = dict(th["val"]), dict(th["cnt"]), th["pods"]
        for j in range(prefix):
            if victims[j] and contributes[ti][j]:
                pods -= 1
                for d, v in creq[j].items():
                    val[d] -= v
                    cnt[d] -= 1
        live.append([t, ti, val, cnt, pods])
    for j in range(prefix - 1, -1, -1):
        if not victims[j]:
            continue
        back = []
        for entry in live:
            t, ti, val, cnt, pods = entry
            if not contributes[ti][j]:
                continue
            val, cnt, pods = dict(val), dict(cnt), pods + 1
            for d, v in creq[j].items():
                val[d] = val.get(d, 0) + v
                cnt[d] = cnt.get(d, 0) + 1
            th = ctx["thr"][t]
            eq3 = eq if int(snap.thr_flags[t]) & S.THR_CLUSTER else True
            res, res_count = _amount_dict(snap.thr_reserved, t, snap.D)
            cc = th["calc_count"]
            names = {}
            for d in range(snap.D):
                u_pr, cv = cnt.get(d, 0) > 0, th["calc"].get(d)
                names[d] = (cv is not None and u_pr and val.get(d, 0) >= cv, u_pr, val.get(d, 0))
            first = _gang_first_stopped(members, [t in a for a in affected], reqs, (th["th"], th["th_count"]),
                                        (cc is not None and pods > 0 and pods >= cc, pods > 0, pods, names), res, res_count, eq3, eq)
            if first is not None:
                break
            back.append((entry, val, cnt, pods))
        else:
            victims[j] = 0
            for entry, val, cnt, pods in back:
                entry[2:] = [val, cnt, pods]


def preempt_gangs_of(snap, member_rows, cand_rows, now, on_equal=False, ctx=None, reprieve=False):
    """kt_preempt_gangs_launch for one gang, in closed form on a Snapshot (no GPU) -> (prefix, victims [len(cand_rows)], blocker).
    prefix: the smallest k for which an in-order admission of ``member_rows`` — PreFilter, and on Success Reserve on every
    throttle that affects the member — admits every member once the candidates ``cand_rows[:k]`` are gone and every responsible
    throttle has been reconciled at ``now``; -1: no prefix does, a member's PreFilter is an Error or its row is invalid.
    victims[j] = 1 iff j < prefix, the candidate is counted and a throttle that affects some member matches it.  blocker: the
    position in ``member_rows`` of the first member that is not Success with nothing deleted (-1 when prefix == 0).
    Per throttle the members meet `used` lowered by a prefix sum over the candidates and `reserved` raised by a prefix sum over
    the earlier members it affects: both are formed directly, nothing is admitted step by step across throttles.
    ``reprieve`` (kt_preempt_gangs_reprieve_launch): the masked victims are then put back one by one, the last first, and each
    stays back as long as the in-order admission still admits every member; victims is what remains."""
    ctx = preempt_context(snap, now) if ctx is None else ctx
    members, cands, eq = [int(p) for p in member_rows], [int(c) for c in cand_rows], bool(on_equal)
    m, g = len(cands), len(members)
    affected, bad_at = [], None  # per member its affecting throttles; the first member that is invalid or an Error
    for j, p in enumerate(members):
        valid = 0 <= p < snap.n_pods and bool(int(snap.pod_flags[p]) & S.POD_VALID)
        err, rows = affected_throttles(snap, p) if valid else (True, [])
        if (err or not valid) and bad_at is None:
            bad_at = j
        affected.append(set(rows))
    m_eff = m
    for j, c in enumerate(cands):
        if not (0 <= c < snap.n_pods) or not int(snap.pod_flags[c]) & S.POD_VALID or affected_throttles(snap, c)[0]:
            m_eff = j
            break
    counted = lambda c: (int(snap.pod_flags[c]) & (_COUNTABLE | S.POD_FINISHED)) == _COUNTABLE
    reqs = [pod_requests(snap, p) if 0 <= p < snap.n_pods else {} for p in members]
    creq = [pod_requests(snap, c) if counted(c) else {} for c in cands[:m_eff]]
    union = sorted(set().union(*affected)) if affected else []
    contributes = [[counted(c) and t in ctx["match"].get(c, ()) for c in cands[:m_eff]] for t in union]
    fails = [False] * (m_eff + 1)  # fails[k]: some (member, throttle, amount) stops the gang in S_k
    never = bad_at is not None
    block0 = g if bad_at is None else bad_at
    for ti, t in enumerate(union):
        th = ctx["thr"][t]
        f = int(snap.thr_flags[t])
        eq3 = eq if f & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
        res, res_count = _amount_dict(snap.thr_reserved, t, snap.D)
        hit = [t in a for a in affected]
        if th["error"]:  # the stored status stays, in every S_k
            used, used_count = _amount_dict(snap.thr_used, t, snap.D)
            sth = _amount_dict(snap.thr_calc if f & S.THR_CALC_AT_NONZERO else snap.thr_spec, t, snap.D)
            flg = int(snap.thr_thrl_flag[t]) & int(snap.thr_thrl_has[t])
            names = {d: (bool(flg >> d & 1), d in used, used.get(d, 0)) for d in range(snap.D)}
            first = _gang_first_stopped(members, hit, reqs, sth, (bool(f & S.THR_THROTTLED_POD), used_count is not None, used_count or 0, names),
                                        res, res_count, eq3, eq)
            if first is not None:
                never, block0 = True, min(block0, first)
            continue
        val, cnt, pods = dict(th["val"]), dict(th["cnt"]), th["pods"]
        for k in range(m_eff + 1):
            if k > 0 and contributes[ti][k - 1]:
                pods -= 1
                for d, v in creq[k - 1].items():
                    val[d] -= v
                    cnt[d] -= 1
            cc = th["calc_count"]
            names = {}
            for d in range(snap.D):
                u_pr, cv = cnt.get(d, 0) > 0, th["calc"].get(d)
                names[d] = (cv is not None and u_pr and val.get(d, 0) >= cv, u_pr, val.get(d, 0))
            first = _gang_first_stopped(members, hit, reqs, (th["th"], th["th_count"]),
                                        (cc is not None and pods > 0 and pods >= cc, pods > 0, pods, names), res, res_count, eq3, eq)
            if first is not None:
                fails[k] = True
                if k == 0:
                    block0 = min(block0, first)
    prefix = -1 if never else next((k for k in range(m_eff + 1) if not fails[k]), -1)
    victims = [0] * m
    for j in range(max(prefix, 0)):
        victims[j] = int(any(contributes[ti][j] for ti in range(len(union))))
    if reprieve and prefix > 0:
        _gang_reprieve(snap, ctx, members, union, affected, contributes, creq, reqs, eq, prefix, victims)
    return prefix, victims, (-1 if prefix == 0 or block0 >= g else block0)


# ---- preempt, for elastic gangs (kt_preempt_gangs_elastic_launch): member-major, on the sums of ``preempt_context`` ----
def preempt_gangs_elastic_of(snap, member_rows, min_members, required, cand_rows, now, on_equal=False, ctx=None, reprieve=False):
    """kt_preempt_gangs_elastic_launch for one gang on a Snapshot (no GPU) -> (prefix, victims [len(cand_rows)], members, blocker).
    In every state the members are walked in order: a member that succeeds reserves on every throttle that affects it, one that
    fails reserves nowhere, every member is evaluated, one whose PreFilter is an Error or whose row is invalid never succeeds; the
    state passes iff at least ``min_members`` members succeed and every ``required`` one (bools per member, None: none) does.
    prefix: the smallest k whose S_k passes (-1: none, or members that never succeed put the rule out of reach) — every k up to it
    is walked, the verdict is not monotone in k.  victims[j] = 1 iff j < prefix, the candidate is counted and a throttle that
    affects some member matches it.  members: the successes in the final state (S_0 where there is no prefix).  blocker: -1 iff
    prefix == 0, else the position in ``member_rows`` of the first required member that does not succeed in S_0, else of the first
    member that does not.  The state per throttle of the union is what ``preempt_gangs_of`` forms — `used` lowered candidate by
    candidate, exact presence — but the reservations are formed member by member, across throttles.
    ``reprieve`` (KT_PREEMPT_REPRIEVE): the masked victims are put back one by one, the last first, and each stays back iff the
    state still passes; victims and members are what remains."""
    ctx = preempt_context(snap, now) if ctx is None else ctx
    members, cands, eq = [int(p) for p in member_rows], [int(c) for c in cand_rows], bool(on_equal)
    m, g, quorum = len(cands), len(members), int(min_members)
    required = [bool(x) for x in required] if required is not None else [False] * g
    affected, never = [], []
    for p in members:
        valid = 0 <= p < snap.n_pods and bool(int(snap.pod_flags[p]) & S.POD_VALID)
        err, rows = affected_throttles(snap, p) if valid else (True, [])
        never.append(err or not valid)
        affected.append(rows)
    m_eff = m
    for j, c in enumerate(cands):
        if not (0 <= c < snap.n_pods) or not int(snap.pod_flags[c]) & S.POD_VALID or affected_throttles(snap, c)[0]:
            m_eff = j
            break
    counted = lambda c: (int(snap.pod_flags[c]) & (_COUNTABLE | S.POD_FINISHED)) == _COUNTABLE
    reqs = [pod_requests(snap, p) if 0 <= p < snap.n_pods else {} for p in members]
    creq = [pod_requests(snap, c) if counted(c) else {} for c in cands[:m_eff]]
    union = sorted(set().union(*affected)) if affected else []
    hits = [[t for t in union if counted(c) and t in ctx["match"].get(c, ())] for c in cands[:m_eff]]
    # the state: per reconciled throttle of the union [values, contributor counts, counted pods]; an error throttle keeps its stored status
    state = {t: [dict(ctx["thr"][t]["val"]), dict(ctx["thr"][t]["cnt"]), ctx["thr"][t]["pods"]] for t in union if not ctx["thr"][t]["error"]}

    def move(j, sign):
        for t in hits[j]:
            if t in state:
                val, cnt, _ = state[t]
                state[t][2] += sign
                for d, v in creq[j].items():
                    val[d] = val.get(d, 0) + sign * v
                    cnt[d] = cnt.get(d, 0) + sign

    def walk():
        res = {t: list(_amount_dict(snap.thr_reserved, t, snap.D)) for t in union}  # the stored rows: [{name: value}, count or None]
        ok = []
        for j in range(g):
            bad = never[j]
            for t in ([] if bad else affected[j]):
                th, f = ctx["thr"][t], int(snap.thr_flags[t])
                eq3 = eq if f & S.THR_CLUSTER else True
                rv, rc = res[t]
                if t in state:
                    val, cnt, pods = state[t]
                    cc = th["calc_count"]
                    bad = bad or _amount_fails(1, th["th_count"], cc is not None and pods > 0 and pods >= cc, pods > 0, pods, rc is not None, rc or 0, eq3, eq)
                    for d, v in reqs[j].items():
                        u_pr, cv = cnt.get(d, 0) > 0, th["calc"].get(d)
                        bad = bad or (v != 0 and _amount_fails(v, th["th"].get(d), cv is not None and u_pr and val.get(d, 0) >= cv, u_pr, val.get(d, 0),
                                                               d in rv, rv.get(d, 0), eq3, eq))
                else:
                    used, used_count = _amount_dict(snap.thr_used, t, snap.D)
                    sth, sth_count = _amount_dict(snap.thr_calc if f & S.THR_CALC_AT_NONZERO else snap.thr_spec, t, snap.D)
                    flg = int(snap.thr_thrl_flag[t]) & int(snap.thr_thrl_has[t])
                    bad = bad or _amount_fails(1, sth_count, bool(f & S.THR_THROTTLED_POD), used_count is not None, used_count or 0, rc is not None,
                                               rc or 0, eq3, eq)
                    for d, v in reqs[j].items():
                        bad = bad or (v != 0 and _amount_fails(v, sth.get(d), bool(flg >> d & 1), d in used, used.get(d, 0), d in rv, rv.get(d, 0), eq3, eq))
            ok.append(not bad)
            if not bad:  # Reserve: every name the pod carries becomes present, zero-valued ones included; count + 1
                for t in affected[j]:
                    for d, v in reqs[j].items():
                        res[t][0][d] = res[t][0].get(d, 0) + v
                    res[t][1] = (res[t][1] or 0) + 1
        return ok

    out_of_reach = any(n and r for n, r in zip(never, required)) or g - sum(never) < quorum
    passes = lambda ok: not out_of_reach and sum(ok) >= quorum and not any(r and not o for r, o in zip(required, ok))
    ok0 = ok = walk()
    prefix = 0 if passes(ok) else -1
    k = 0
    while prefix < 0 and not out_of_reach and k < m_eff:
        k += 1
        if hits[k - 1]:  # (a candidate that touches no throttle of the union: the verdict of k - 1 stands)
            move(k - 1, -1)
            ok = walk()
            if passes(ok):
                prefix = k
    failed = [j for j in range(g) if not ok0[j]]
    blocker = -1 if prefix == 0 else next((j for j in failed if required[j]), failed[0])
    victims = [int(j < prefix and bool(hits[j])) for j in range(m)]
    if prefix < 0:
        return prefix, victims, sum(ok0), blocker
    if reprieve:
        for j in range(prefix - 1, -1, -1):
            if not victims[j]:
                continue
            move(j, 1)
            back = walk()
            if passes(back):
                victims[j], ok = 0, back
            else:
                move(j, -1)
    return prefix, victims, sum(ok), blocker


# ---- preempt, for gangs, over pages (kt_paged_preempt_gangs): the closed form over a list of page snapshots ----
def paged_preempt_gangs_of(snaps, member_rows, cand_rows, now, on_equal=False, reprieve=False, ctx=None):
    """kt_paged_preempt_gangs for one gang, in closed form over the page snapshots (no GPU) -> (prefix, victims [len(cand_rows)],
    blocker): ``preempt_gangs_of`` on the cluster of all names, ``ctx`` is ``paged_preempt_context``'s.  What pages add:
      * which throttles affect which member, which candidates are counted and matched, the error rows, the list cut and "a member
        is an Error or invalid" are page 0's (the selector side is the same in every page);
      * the pod count — the threshold's, `used`'s, the calculated threshold's, the stored and the running reserved count — is
        page 0's and is judged once; a name part is judged on its own page;
      * the gang passes in S_k iff for every throttle of the union the in-order member walk passes the count part and the name
        part of every page; each page carries its own reserved prefix from its stored reserved row, and a member the throttle
        affects adds its value of every name it carries, the presence of all of them (zero-valued ones included) and count + 1;
      * a throttle keeps its stored status on every page iff its reconcile is an error on some page, and reads the calculated
        threshold on every page iff some page has calculatedAt set or replaces it at ``now`` (a stored throttle reads the STORED
        calculated threshold);
      * blocker: the minimum over throttles and pages of the first stopped position with nothing deleted (an Error or invalid
        member counts as stopped), -1 when prefix == 0;
      * victims[j] = 1 iff j < prefix, c_j is counted and a throttle affecting some member matches it.
    Names are keyed (page, dim), so one walk of the members over all keys IS the walk on every page: the first member that some
    page stops is the minimum of the pages' own first stopped members.  ``reprieve``: the walk of
    kt_preempt_gangs_reprieve_launch with that joint judge.  With one snapshot this is ``preempt_gangs_of``."""
    snap0 = snaps[0]
    ctx = paged_preempt_context(snaps, now) if ctx is None else ctx
    members, cands, eq = [int(p) for p in member_rows], [int(c) for c in cand_rows], bool(on_equal)
    m, g = len(cands), len(members)
    affected, bad_at = [], None  # per member its affecting throttles; the first member that is invalid or an Error
    for j, p in enumerate(members):
        valid = 0 <= p < snap0.n_pods and bool(int(snap0.pod_flags[p]) & S.POD_VALID)
        err, rows = affected_throttles(snap0, p) if valid else (True, [])
        if (err or not valid) and bad_at is None:
            bad_at = j
        affected.append(set(rows))
    m_eff = m
    for j, c in enumerate(cands):
        if not (0 <= c < snap0.n_pods) or not int(snap0.pod_flags[c]) & S.POD_VALID or affected_throttles(snap0, c)[0]:
            m_eff = j
            break
    counted = lambda c: (int(snap0.pod_flags[c]) & (_COUNTABLE | S.POD_FINISHED)) == _COUNTABLE

    def requests(c):
        return {(k, d): v for k, s in enumerate(snaps) for d, v in pod_requests(s, c).items()}

    keys = [(k, d) for k, s in enumerate(snaps) for d in range(s.D)]
    reqs = [requests(p) if 0 <= p < snap0.n_pods else {} for p in members]
    creq = [requests(c) if counted(c) else {} for c in cands[:m_eff]]
    union = sorted(set().union(*affected)) if affected else []
    contributes = [[counted(c) and t in ctx["match"].get(c, ()) for c in cands[:m_eff]] for t in union]

    def first_stopped(t, state):
        """the first member throttle ``t`` stops on some page against the reconciled `used` ``state`` = [values, counts, pods]"""
        th = ctx["thr"][t]
        val, cnt, pods = state
        eq3 = eq if int(snap0.thr_flags[t]) & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
        res, res_count = _paged_amounts(snaps, "thr_reserved", t)
        cc, names = th["calc_count"], {}
        for kd in keys:
            u_pr, cv = cnt.get(kd, 0) > 0, th["calc"].get(kd)
            names[kd] = (cv is not None and u_pr and val.get(kd, 0) >= cv, u_pr, val.get(kd, 0))
        return _gang_first_stopped(members, [t in a for a in affected], reqs, (th["th"], th["th_count"]),
                                   (cc is not None and pods > 0 and pods >= cc, pods > 0, pods, names), res, res_count, eq3, eq)

    def moved(state, j, sign):
        val, cnt, pods = dict(state[0]), dict(state[1]), state[2] + sign
        for kd, v in creq[j].items():
            val[kd] = val.get(kd, 0) + sign * v
            cnt[kd] = cnt.get(kd, 0) + sign
        return [val, cnt, pods]

    fails = [False] * (m_eff + 1)  # fails[k]: some (member, throttle, page, amount) stops the gang in S_k
    never = bad_at is not None
    block0 = g if bad_at is None else bad_at
    for ti, t in enumerate(union):
        th = ctx["thr"][t]
        if th["error"]:  # the stored status stays on every page, in every S_k
            f = int(snap0.thr_flags[t])
            eq3 = eq if f & S.THR_CLUSTER else True
            res, res_count = _paged_amounts(snaps, "thr_reserved", t)
            used, used_count = _paged_amounts(snaps, "thr_used", t)
            sth = _paged_amounts(snaps, "thr_calc" if th["use_calc"] else "thr_spec", t)
            names = {}
            for k, d in keys:
                flg = int(snaps[k].thr_thrl_flag[t]) & int(snaps[k].thr_thrl_has[t])
                names[(k, d)] = (bool(flg >> d & 1), (k, d) in used, used.get((k, d), 0))
            first = _gang_first_stopped(members, [t in a for a in affected], reqs, sth,
                                        (bool(f & S.THR_THROTTLED_POD), used_count is not None, used_count or 0, names), res, res_count, eq3, eq)
            if first is not None:
                never, block0 = True, min(block0, first)
            continue
        state = [th["val"], th["cnt"], th["pods"]]
        for k in range(m_eff + 1):
            if k > 0 and contributes[ti][k - 1]:
                state = moved(state, k - 1, -1)
            first = first_stopped(t, state)
            if first is not None:
                fails[k] = True
                if k == 0:
                    block0 = min(block0, first)
    prefix = -1 if never else next((k for k in range(m_eff + 1) if not fails[k]), -1)
    victims = [0] * m
    for j in range(max(prefix, 0)):
        victims[j] = int(any(contributes[ti][j] for ti in range(len(union))))
    if reprieve and prefix > 0:
        live = []  # [index in `contributes`, throttle row, state] of the reconciled throttles of the union, in S(the masked victims)
        for ti, t in enumerate(union):
            th = ctx["thr"][t]
            if th["error"]:  # keeps its stored status whoever is deleted: it passed, or the prefix would not be positive
                continue
            state = [th["val"], th["cnt"], th["pods"]]
            for j in range(prefix):
                if victims[j] and contributes[ti][j]:
                    state = moved(state, j, -1)
            live.append([ti, t, state])
        for j in range(prefix - 1, -1, -1):
            if not victims[j]:
                continue
            back = [(entry, moved(entry[2], j, 1)) for entry in live if contributes[entry[0]][j]]
            if any(first_stopped(entry[1], state) is not None for entry, state in back):
                continue  # some page of some throttle stops a member with c_j back: it stays a victim
            victims[j] = 0
            for entry, state in back:
                entry[2] = state
    return prefix, victims, (-1 if prefix == 0 or block0 >= g else block0)


# ---- forecast: the first instant at which a blocked pod passes (kt_forecast_launch), in closed form on a Snapshot ----
def _instant(t):
    return int(t[0]), int(t[1])


def override_instants_of(snap, from_, until):
    """kt_override_instants on a Snapshot (no GPU): the sorted, distinct instants in (from_, until] at which the
    CalculateThreshold of some valid and responsible throttle can change — every parsed non-zero ``begin`` and, for every parsed
    non-zero ``end``, the instant end + 1 ns: the first at which the override is no longer active (both ends are inclusive).
    Overrides with a parse error contribute nothing -> [(seconds, nanoseconds)]."""
    lo, hi = _instant(from_), _instant(until)
    need = S.THR_VALID | S.THR_RESPONSIBLE
    zero = (S.ZERO_TIME_S, 0)
    out = set()
    for t in range(snap.n_thr):
        if (int(snap.thr_flags[t]) & need) != need:
            continue
        for o in range(int(snap.thr_ovr_off[t]), int(snap.thr_ovr_off[t + 1])):
            if int(snap.ovr_flags[o]) & S.OVR_PARSE_ERROR:
                continue
            begin = (int(snap.ovr_begin_s[o]), int(snap.ovr_begin_ns[o]))
            end = (int(snap.ovr_end_s[o]), int(snap.ovr_end_ns[o]))
            if begin != zero:
                out.add(begin)
            if end != zero:
                out.add((end[0] + 1, 0) if end[1] == 999_999_999 else (end[0], end[1] + 1))
    return sorted(t for t in out if lo < t <= hi)


def forecast_of(snap, pod_row, instants, on_equal=False, ctx=None):
    """kt_forecast_launch for one pod, in closed form on a Snapshot (no GPU) -> (first, verdicts [len(instants)]).
    verdicts[k]: the KT_VERDICT_* of PreFilter(pod) once every valid and responsible throttle has been reconciled at
    ``instants[k]`` on the state as it is now (reserved amounts unchanged; a throttle whose reconcile is an error keeps its stored
    status at every instant); first: the smallest k with Success, or -1.  `used` does not depend on the instant: ``ctx`` is
    ``preempt_context``'s aggregate (any ``now``: only its sums, error marks and match lists are read).  Per throttle and instant:
    CalculateThreshold (the first active override wins per name and for the count), replaced only where it differs from the
    stored calculatedThreshold by value or in its messages, read by the check iff calculatedAt was non-zero or it is replaced."""
    inst = [_instant(t) for t in instants]
    ctx = preempt_context(snap, inst[0]) if ctx is None else ctx
    p, eq, m = int(pod_row), bool(on_equal), len(inst)
    if not (0 <= p < snap.n_pods) or not int(snap.pod_flags[p]) & S.POD_VALID:
        return -1, [S.VERDICT_ERROR] * m
    err, affected = affected_throttles(snap, p)
    if err:
        return -1, [S.VERDICT_ERROR] * m
    req = {d: v for d, v in pod_requests(snap, p).items() if v != 0}
    fails = [False] * m
    for t in affected:
        th = ctx["thr"][t]
        f = int(snap.thr_flags[t])
        eq3 = eq if f & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
        res, res_count = _amount_dict(snap.thr_reserved, t, snap.D)
        if th["error"]:  # the stored status, at every instant
            used, used_count = _amount_dict(snap.thr_used, t, snap.D)
            sth, sth_count = _amount_dict(snap.thr_calc if f & S.THR_CALC_AT_NONZERO else snap.thr_spec, t, snap.D)
            flg = int(snap.thr_thrl_flag[t]) & int(snap.thr_thrl_has[t])
            bad = _amount_fails(1, sth_count, bool(f & S.THR_THROTTLED_POD), used_count is not None, used_count or 0,
                                res_count is not None, res_count or 0, eq3, eq)
            for d, v in req.items():
                bad = bad or _amount_fails(v, sth.get(d), bool(flg >> d & 1), d in used, used.get(d, 0), d in res, res.get(d, 0), eq3, eq)
            if bad:
                fails = [True] * m
                break
            continue
        val, cnt, pods = th["val"], th["cnt"], th["pods"]
        u_hc = pods > 0
        stored = _amount_dict(snap.thr_calc, t, snap.D)
        spec, spec_count = _amount_dict(snap.thr_spec, t, snap.D)
        for k, at in enumerate(inst):
            calc, cc, any_err = _calculated_threshold(snap, t, at)
            fp = int(snap.thr_spec_msgs_fp[t]) if any_err else 0
            replace = (calc, cc) != stored or int(snap.thr_status_msgs_fp[t]) != fp
            rd, rd_count = (calc, cc) if (f & S.THR_CALC_AT_NONZERO) or replace else (spec, spec_count)
            bad = _amount_fails(1, rd_count, cc is not None and u_hc and pods >= cc, u_hc, pods, res_count is not None, res_count or 0, eq3, eq)
            for d, v in req.items():
                u_pr = cnt.get(d, 0) > 0
                cv = calc.get(d)
                bad = bad or _amount_fails(v, rd.get(d), cv is not None and u_pr and val.get(d, 0) >= cv, u_pr, val.get(d, 0), d in res,
                                           res.get(d, 0), eq3, eq)
            fails[k] = fails[k] or bad
    verdicts_ = [S.VERDICT_BLOCK if b else S.VERDICT_ALLOW for b in fails]
    return next((k for k in range(m) if not fails[k]), -1), verdicts_


# ---- headroom forecast (kt_headroom_forecast_launch), in closed form on a Snapshot ----
def headroom_forecast_of(snap, pod_row, instants, cap, want=1, on_equal=False, ctx=None):
    """kt_headroom_forecast_launch for one pod, in closed form on a Snapshot (no GPU) -> (first, copies [len(instants)], limiting
    [len(instants)]).  copies[k]: the leading Success verdicts of a dry admission of ``[pod] * cap`` once every valid and
    responsible throttle has been reconciled at ``instants[k]`` on the state as it is now — per throttle and instant
    ``forecast_of``'s threshold (CalculateThreshold, the replace rule, which threshold the check reads, throttled from the fresh
    sums), per amount ``headroom_of``'s closed form, the minimum over both; limiting[k]: the lowest throttle row that stops the
    next copy, -1 where all ``cap`` are admitted; first: the smallest k with copies[k] >= want, or -1.  A throttle whose reconcile
    is an error is judged from its stored status, at every instant.  ``ctx`` is ``preempt_context``'s aggregate (any ``now``)."""
    inst = [_instant(t) for t in instants]
    ctx = preempt_context(snap, inst[0]) if ctx is None else ctx
    p, eq, m, cap = int(pod_row), bool(on_equal), len(inst), int(cap)
    if not (0 <= p < snap.n_pods) or not int(snap.pod_flags[p]) & S.POD_VALID:
        return -1, [0] * m, [-1] * m
    err, affected = affected_throttles(snap, p)
    if err:
        return -1, [0] * m, [-1] * m
    req = {d: v for d, v in pod_requests(snap, p).items() if v != 0}  # (every name in it is present: the pod brings it)
    best = [(cap, -1)] * m  # (copies, row): affected is ascending, so a strict < keeps the lowest row of a tie
    for t in affected:
        th = ctx["thr"][t]
        f = int(snap.thr_flags[t])
        eq3 = eq if f & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
        res, res_count = _amount_dict(snap.thr_reserved, t, snap.D)
        r_hc = res_count is not None
        if th["error"]:  # the stored status, at every instant
            used, used_count = _amount_dict(snap.thr_used, t, snap.D)
            sth, sth_count = _amount_dict(snap.thr_calc if f & S.THR_CALC_AT_NONZERO else snap.thr_spec, t, snap.D)
            flg = int(snap.thr_thrl_flag[t]) & int(snap.thr_thrl_has[t])
            u_hc = used_count is not None
            h = _copies_of_amount(1, True, sth_count is not None, sth_count or 0, used_count or 0, res_count or 0, u_hc or r_hc,
                                  bool(f & S.THR_THROTTLED_POD), eq3, eq, cap)
            for d, v in req.items():
                h = min(h, _copies_of_amount(v, True, d in sth, sth.get(d, 0), used.get(d, 0), res.get(d, 0), d in used or d in res,
                                             bool(flg >> d & 1), eq3, eq, cap))
            best = [(h, t) if h < b[0] else b for b in best]
            continue
        val, cnt, pods = th["val"], th["cnt"], th["pods"]
        u_hc = pods > 0
        stored = _amount_dict(snap.thr_calc, t, snap.D)
        spec, spec_count = _amount_dict(snap.thr_spec, t, snap.D)
        for k, at in enumerate(inst):
            calc, cc, any_err = _calculated_threshold(snap, t, at)
            fp = int(snap.thr_spec_msgs_fp[t]) if any_err else 0
            replace = (calc, cc) != stored or int(snap.thr_status_msgs_fp[t]) != fp
            rd, rd_count = (calc, cc) if (f & S.THR_CALC_AT_NONZERO) or replace else (spec, spec_count)
            h = _copies_of_amount(1, True, rd_count is not None, rd_count or 0, pods if u_hc else 0, res_count or 0, u_hc or r_hc,
                                  cc is not None and u_hc and pods >= cc, eq3, eq, cap)
            for d, v in req.items():
                u_pr = cnt.get(d, 0) > 0
                uv = val.get(d, 0) if u_pr else 0
                cv = calc.get(d)
                h = min(h, _copies_of_amount(v, True, d in rd, rd.get(d, 0), uv, res.get(d, 0), u_pr or d in res,
                                             cv is not None and u_pr and uv >= cv, eq3, eq, cap))
            if h < best[k][0]:
                best[k] = (h, t)
    copies = [b[0] for b in best]
    return next((k for k in range(m) if copies[k] >= int(want)), -1), copies, [b[1] for b in best]


# ---- forecast, for gangs (kt_forecast_gangs_launch), in closed form on a Snapshot ----
def forecast_gangs_of(snap, member_rows, instants, on_equal=False, ctx=None):
    """kt_forecast_gangs_launch for one gang, in closed form on a Snapshot (no GPU) -> (first, verdicts [len(instants)], blockers
    [len(instants)]).  verdicts[k]: Success iff an in-order admission of ``member_rows`` — PreFilter, and on Success Reserve on
    every throttle that affects the member — admits every member once every valid and responsible throttle has been reconciled at
    ``instants[k]`` on the state as it is now; Error at every instant when a member's PreFilter is an Error or its row is invalid.
    blockers[k]: the position in ``member_rows`` of the first member that is not Success at that instant, -1 where the gang
    passes; first: the smallest k with Success, or -1.  ``forecast_of``'s threshold per throttle and instant, met by the members
    under ``_gang_first_stopped``'s reserved prefix; `used` and the reserved prefix do not depend on the instant.  ``ctx`` is
    ``preempt_context``'s aggregate (any ``now``)."""
    inst = [_instant(t) for t in instants]
    ctx = preempt_context(snap, inst[0]) if ctx is None else ctx
    members, eq, m = [int(p) for p in member_rows], bool(on_equal), len(inst)
    g = len(members)
    affected, bad_at = [], None  # per member its affecting throttles; the first member that is invalid or an Error
    for j, p in enumerate(members):
        valid = 0 <= p < snap.n_pods and bool(int(snap.pod_flags[p]) & S.POD_VALID)
        err, rows = affected_throttles(snap, p) if valid else (True, [])
        if (err or not valid) and bad_at is None:
            bad_at = j
        affected.append(set(rows))
    reqs = [pod_requests(snap, p) if 0 <= p < snap.n_pods else {} for p in members]
    stopped = [g if bad_at is None else bad_at] * m  # per instant the first member some throttle stops (g: none)
    for t in (sorted(set().union(*affected)) if affected else []):
        th = ctx["thr"][t]
        f = int(snap.thr_flags[t])
        eq3 = eq if f & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
        res, res_count = _amount_dict(snap.thr_reserved, t, snap.D)
        hit = [t in a for a in affected]
        if th["error"]:  # the stored status, at every instant
            used, used_count = _amount_dict(snap.thr_used, t, snap.D)
            sth = _amount_dict(snap.thr_calc if f & S.THR_CALC_AT_NONZERO else snap.thr_spec, t, snap.D)
            flg = int(snap.thr_thrl_flag[t]) & int(snap.thr_thrl_has[t])
            names = {d: (bool(flg >> d & 1), d in used, used.get(d, 0)) for d in range(snap.D)}
            j = _gang_first_stopped(members, hit, reqs, sth, (bool(f & S.THR_THROTTLED_POD), used_count is not None, used_count or 0, names),
                                    res, res_count, eq3, eq)
            if j is not None:
                stopped = [min(s, j) for s in stopped]
            continue
        val, cnt, pods = th["val"], th["cnt"], th["pods"]
        stored = _amount_dict(snap.thr_calc, t, snap.D)
        spec = _amount_dict(snap.thr_spec, t, snap.D)
        for k, at in enumerate(inst):
            calc, cc, any_err = _calculated_threshold(snap, t, at)
            fp = int(snap.thr_spec_msgs_fp[t]) if any_err else 0
            replace = (calc, cc) != stored or int(snap.thr_status_msgs_fp[t]) != fp
            rd = (calc, cc) if (f & S.THR_CALC_AT_NONZERO) or replace else spec
            names = {}
            for d in range(snap.D):
                u_pr, cv = cnt.get(d, 0) > 0, calc.get(d)
                names[d] = (cv is not None and u_pr and val.get(d, 0) >= cv, u_pr, val.get(d, 0))
            j = _gang_first_stopped(members, hit, reqs, rd, (cc is not None and pods > 0 and pods >= cc, pods > 0, pods, names), res, res_count,
                                    eq3, eq)
            if j is not None:
                stopped[k] = min(stopped[k], j)
    if bad_at is not None:
        verdicts_ = [S.VERDICT_ERROR] * m
    else:
        verdicts_ = [S.VERDICT_BLOCK if s < g else S.VERDICT_ALLOW for s in stopped]
    first = next((k for k in range(m) if verdicts_[k] == S.VERDICT_ALLOW), -1)
    return first, verdicts_, [s if s < g else -1 for s in stopped]


# ---- headroom, for gangs (kt_headroom_gangs_launch), as the kernel computes it, on a Snapshot ----
_INT64_MAX = (1 << 63) - 1


def headroom_gangs_of(snap, member_rows, cap, on_equal=False):
    """kt_headroom_gangs_launch for one gang, restated on a Snapshot (no GPU) -> (copies, limiting, blocker position inside
    ``member_rows``).  copies: the leading admitted gangs of a dry-run gang admission of ``cap`` consecutive copies of the gang
    against the stored status and reserved amounts.  Copy j meets on throttle t the stored reserved row plus j x A_t (what one
    admitted copy reserves on t: one pod per member t affects, every name such a member carries by value and by presence; from
    copy 1 on the count and those names are present), judged by ``_gang_first_stopped``; per throttle the candidates end at the
    running minimum and where a named amount would leave int64, the first failing one is found by the kernel's 64-ary search,
    and the answer is the lexicographic minimum of (h_t, first stopped member at j = h_t, t).  limiting / blocker: -1 / -1 when
    all ``cap`` copies are admitted.  A member whose PreFilter is an Error or whose row is invalid: 0 copies, the walk of copy 0
    ends in front of it, limiting -1 when it is the blocker itself."""
    members, eq, cap = [int(p) for p in member_rows], bool(on_equal), int(cap)
    affected, bad_at = [], None  # per member its affecting throttles; the first member that is invalid or an Error
    for j, p in enumerate(members):
        valid = 0 <= p < snap.n_pods and bool(int(snap.pod_flags[p]) & S.POD_VALID)
        err, rows = affected_throttles(snap, p) if valid else (True, [])
        if (err or not valid) and bad_at is None:
            bad_at = j
        affected.append(set(rows))
    g = len(members) if bad_at is None else bad_at  # the members that are walked
    members, affected = members[:g], affected[:g]
    reqs = [pod_requests(snap, p) for p in members]
    best = (cap if bad_at is None else 0, g, -1)  # (h, first, t)
    for t in (sorted(set().union(*affected)) if affected else []):
        f = int(snap.thr_flags[t])
        eq3 = eq if f & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
        th = _amount_dict(snap.thr_calc if f & S.THR_CALC_AT_NONZERO else snap.thr_spec, t, snap.D)
        used, used_count = _amount_dict(snap.thr_used, t, snap.D)
        flg = int(snap.thr_thrl_flag[t]) & int(snap.thr_thrl_has[t])
        names = {d: (bool(flg >> d & 1), d in used, used.get(d, 0)) for d in range(snap.D)}
        ustate = (bool(f & S.THR_THROTTLED_POD), used_count is not None, used_count or 0, names)
        res, res_count = _amount_dict(snap.thr_reserved, t, snap.D)
        hit = [t in a for a in affected]
        # A_t: only what the threshold names is summed (the rest is never compared)
        per, per_p, per_c = {}, set(), 0
        for j in range(g):
            if hit[j]:
                per_c += 1
                for d, v in reqs[j].items():
                    per_p.add(d)
                    if d in th[0]:
                        per[d] = min(per.get(d, 0) + v, _INT64_MAX)
        if th[1] is None:
            per_c = 0

        def first_stopped(j):
            r = {d: res.get(d, 0) + j * per.get(d, 0) for d in (set(res) | per_p if j > 0 else set(res))}
            rc = (res_count or 0) + j * per_c if (res_count is not None or j > 0) else None
            s = _gang_first_stopped(members, hit, reqs, th, ustate, r, rc, eq3, eq)
            return g if s is None else s

        # the range: up to the running minimum, and no further than every named amount stays inside int64
        top = best[0] if best[0] < cap else cap - 1
        if bad_at is None:
            if per_c > 0:
                top = min(top, (_INT64_MAX - (res_count or 0)) // per_c)
            for d, a in per.items():
                if a > 0:
                    top = min(top, (_INT64_MAX - res.get(d, 0)) // a)
        lo, known, first = 0, False, g
        while True:  # the 64-ary search for the first candidate in [lo, top] that fails
            hi = top - 1 if known else top
            n = hi - lo + 1
            if n <= 0:
                break
            step = (n + 63) // 64
            probes = [(j, first_stopped(j)) for j in (hi - (63 - lane) * step for lane in range(64)) if j >= lo]
            fail = next((k for k, (_, s) in enumerate(probes) if s < g), None)
            if fail is None:
                lo = hi + 1
                if not known:
                    break
                continue
            (top, first), known = probes[fail], True
            if fail > 0:
                lo = probes[fail - 1][0] + 1
        if known and (top, first) < best[:2]:
            best = (top, first, t)
    h, first, t = best
    if bad_at is not None:
        return 0, (t if first < g else -1), first
    return (cap, -1, -1) if h >= cap else (h, t, first)


# ---- headroom forecast, for gangs (kt_headroom_forecast_gangs_launch), as the kernel computes it, on a Snapshot ----
def headroom_forecast_gangs_of(snap, member_rows, instants, cap, want=1, on_equal=False, ctx=None):
    """kt_headroom_forecast_gangs_launch for one gang, restated on a Snapshot (no GPU) -> (first, copies [len(instants)], limiting
    [len(instants)], blocker positions inside ``member_rows`` [len(instants)]).  copies[k]: ``headroom_gangs_of`` once every valid
    and responsible throttle has been reconciled at ``instants[k]`` on the state as it is now: ``forecast_gangs_of``'s threshold
    and throttled flags per throttle and instant, ``headroom_gangs_of``'s A_t, range and judge per candidate copy, the first
    failing candidate found by bisection per instant, and per instant the lexicographic minimum of (h_t, first stopped member at
    j = h_t, t).  A throttle whose reconcile is an error is judged once from the stored tables.  limiting / blocker: -1 / -1 where
    all ``cap`` copies are admitted; a member whose PreFilter is an Error or whose row is invalid: 0 copies at every instant, the
    walk of copy 0 ends in front of it, limiting -1 where it is the blocker itself.  first: the smallest k with copies[k] >=
    ``want``, or -1.  ``ctx`` is ``preempt_context``'s aggregate (any ``now``)."""
    inst = [_instant(t) for t in instants]
    ctx = preempt_context(snap, inst[0]) if ctx is None else ctx
    members, eq, cap, m = [int(p) for p in member_rows], bool(on_equal), int(cap), len(inst)
    affected, bad_at = [], None  # per member its affecting throttles; the first member that is invalid or an Error
    for j, p in enumerate(members):
        valid = 0 <= p < snap.n_pods and bool(int(snap.pod_flags[p]) & S.POD_VALID)
        err, rows = affected_throttles(snap, p) if valid else (True, [])
        if (err or not valid) and bad_at is None:
            bad_at = j
        affected.append(set(rows))
    g = len(members) if bad_at is None else bad_at  # the members that are walked
    members, affected = members[:g], affected[:g]
    reqs = [pod_requests(snap, p) for p in members]
    start = (cap if bad_at is None else 0, g, -1)  # (h, first, t)
    best, kept = [start] * m, start  # per instant; and over the throttles that keep their stored status

    def judge(hit, th, ustate, res, res_count, eq3, top):
        """(h_t, first stopped member at j = h_t) of one throttle against one threshold and state of `used`, candidates up to
        ``top``; None: it passes there"""
        per, per_p, per_c = {}, set(), 0  # A_t: only what the threshold names is summed (the rest is never compared)
        for j in range(g):
            if hit[j]:
                per_c += 1
                for d, v in reqs[j].items():
                    per_p.add(d)
                    if d in th[0]:
                        per[d] = min(per.get(d, 0) + v, _INT64_MAX)
        if th[1] is None:
            per_c = 0

        def first_stopped(j):
            r = {d: res.get(d, 0) + j * per.get(d, 0) for d in (set(res) | per_p if j > 0 else set(res))}
            rc = (res_count or 0) + j * per_c if (res_count is not None or j > 0) else None
            s = _gang_first_stopped(members, hit, reqs, th, ustate, r, rc, eq3, eq)
            return g if s is None else s

        if bad_at is None:  # no further than every named amount stays inside int64
            if per_c > 0:
                top = min(top, (_INT64_MAX - (res_count or 0)) // per_c)
            for d, a in per.items():
                if a > 0:
                    top = min(top, (_INT64_MAX - res.get(d, 0)) // a)
        first = first_stopped(top)
        if first >= g:
            return None
        lo, hi = 0, top  # hi has been seen to fail, everything below lo passes
        while lo < hi:
            mid = lo + (hi - lo) // 2
            s = first_stopped(mid)
            if s < g:
                hi, first = mid, s
            else:
                lo = mid + 1
        return hi, first

    for t in (sorted(set().union(*affected)) if affected else []):
        th = ctx["thr"][t]
        f = int(snap.thr_flags[t])
        eq3 = eq if f & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
        res, res_count = _amount_dict(snap.thr_reserved, t, snap.D)
        hit = [t in a for a in affected]
        if th["error"]:  # the stored status, at every instant
            used, used_count = _amount_dict(snap.thr_used, t, snap.D)
            sth = _amount_dict(snap.thr_calc if f & S.THR_CALC_AT_NONZERO else snap.thr_spec, t, snap.D)
            flg = int(snap.thr_thrl_flag[t]) & int(snap.thr_thrl_has[t])
            names = {d: (bool(flg >> d & 1), d in used, used.get(d, 0)) for d in range(snap.D)}
            ustate = (bool(f & S.THR_THROTTLED_POD), used_count is not None, used_count or 0, names)
            got = judge(hit, sth, ustate, res, res_count, eq3, kept[0] if kept[0] < cap else cap - 1)
            if got is not None:
                kept = min(kept, got + (t,))
            continue
        val, cnt, pods = th["val"], th["cnt"], th["pods"]
        stored = _amount_dict(snap.thr_calc, t, snap.D)
        spec = _amount_dict(snap.thr_spec, t, snap.D)
        for k, at in enumerate(inst):
            calc, cc, any_err = _calculated_threshold(snap, t, at)
            fp = int(snap.thr_spec_msgs_fp[t]) if any_err else 0
            replace = (calc, cc) != stored or int(snap.thr_status_msgs_fp[t]) != fp
            rd = (calc, cc) if (f & S.THR_CALC_AT_NONZERO) or replace else spec
            names = {}
            for d in range(snap.D):
                u_pr, cv = cnt.get(d, 0) > 0, calc.get(d)
                names[d] = (cv is not None and u_pr and val.get(d, 0) >= cv, u_pr, val.get(d, 0))
            ustate = (cc is not None and pods > 0 and pods >= cc, pods > 0, pods, names)
            got = judge(hit, rd, ustate, res, res_count, eq3, best[k][0] if best[k][0] < cap else cap - 1)
            if got is not None:
                best[k] = min(best[k], got + (t,))
    copies, limiting, blocker = [], [], []
    for k in range(m):
        h, first, t = min(best[k], kept)
        if bad_at is not None:
            copies.append(0), limiting.append(t if first < g else -1), blocker.append(first)
        elif h >= cap:
            copies.append(cap), limiting.append(-1), blocker.append(-1)
        else:
            copies.append(h), limiting.append(t), blocker.append(first)
    return next((k for k in range(m) if copies[k] >= int(want)), -1), copies, limiting, blocker


# ---- forecast over pages (kt_paged_forecast): the closed form over a list of page snapshots ----
def paged_forecast_of(snaps, pod_row, instants, on_equal=False, ctx=None):
    """kt_paged_forecast for one pod, in closed form over the page snapshots (no GPU) -> (first, verdicts [len(instants)]):
    ``forecast_of`` on the cluster of all names.  Which throttles affect the pod, the error rows and the pod count are page 0's
    (the selector side is the same in every page); ``ctx`` is ``paged_preempt_context``'s (any ``now``: only its sums, error
    marks and match lists are read).  Per affecting throttle:
    the whole-error rule — its reconcile is an error on some page: the stored status is read on every page at every instant,
    against the stored calculatedThreshold iff calculatedAt is set on SOME page, else spec.threshold, judged once;
    the whole-threshold rule — status.calculatedThreshold is compared and replaced as a whole (throttle_controller.go:116-133):
    at instant t every page computes CalculateThreshold(t) over its names; the throttle reads the calculated threshold on EVERY
    page iff calculatedAt is set on some page, or on some page the calculated threshold differs by value from the stored one over
    that page's names or the messages differ (page 0 adds the pod count, the same in every page); otherwise spec.threshold on every
    page.  A page that holds nothing the pod asks for still takes part: it can replace the threshold for all the others.
    The pod fails at t iff the count part or some page's name part of the four steps fails.  With one page this is ``forecast_of``."""
    snap0 = snaps[0]
    inst = [_instant(t) for t in instants]
    ctx = paged_preempt_context(snaps, inst[0]) if ctx is None else ctx
    p, eq, m = int(pod_row), bool(on_equal), len(inst)
    if not (0 <= p < snap0.n_pods) or not int(snap0.pod_flags[p]) & S.POD_VALID:
        return -1, [S.VERDICT_ERROR] * m
    err, affected = affected_throttles(snap0, p)
    if err:
        return -1, [S.VERDICT_ERROR] * m
    req = {(k, d): v for k, s in enumerate(snaps) for d, v in pod_requests(s, p).items() if v != 0}
    fails = [False] * m
    for t in affected:
        th = ctx["thr"][t]
        f = int(snap0.thr_flags[t])
        eq3 = eq if f & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
        res, res_count = _paged_amounts(snaps, "thr_reserved", t)
        calc_at_any = any(int(s.thr_flags[t]) & S.THR_CALC_AT_NONZERO for s in snaps)
        if th["error"]:  # the stored status of every page, at every instant
            used, used_count = _paged_amounts(snaps, "thr_used", t)
            sth, sth_count = _paged_amounts(snaps, "thr_calc" if calc_at_any else "thr_spec", t)
            bad = _amount_fails(1, sth_count, bool(f & S.THR_THROTTLED_POD), used_count is not None, used_count or 0,
                                res_count is not None, res_count or 0, eq3, eq)
            for (k, d), v in req.items():
                flg = int(snaps[k].thr_thrl_flag[t]) & int(snaps[k].thr_thrl_has[t])
                bad = bad or _amount_fails(v, sth.get((k, d)), bool(flg >> d & 1), (k, d) in used, used.get((k, d), 0), (k, d) in res,
                                           res.get((k, d), 0), eq3, eq)
            if bad:
                fails = [True] * m
                break
            continue
        val, cnt, pods = th["val"], th["cnt"], th["pods"]
        u_hc = pods > 0
        spec, spec_count = _paged_amounts(snaps, "thr_spec", t)
        for j, at in enumerate(inst):
            calc, cc, differs = {}, None, False
            for k, s in enumerate(snaps):
                names, count, any_err = _calculated_threshold(s, t, at)
                stored, stored_count = _amount_dict(s.thr_calc, t, s.D)
                fp = int(s.thr_spec_msgs_fp[t]) if any_err else 0
                differs = differs or names != stored or int(s.thr_status_msgs_fp[t]) != fp
                if k == 0:  # the count is the same in every page
                    cc = count
                    differs = differs or count != stored_count
                calc.update({(k, d): v for d, v in names.items()})
            rd, rd_count = (calc, cc) if calc_at_any or differs else (spec, spec_count)
            bad = _amount_fails(1, rd_count, cc is not None and u_hc and pods >= cc, u_hc, pods, res_count is not None, res_count or 0, eq3, eq)
            for kd, v in req.items():
                u_pr = cnt.get(kd, 0) > 0
                cv = calc.get(kd)
                bad = bad or _amount_fails(v, rd.get(kd), cv is not None and u_pr and val.get(kd, 0) >= cv, u_pr, val.get(kd, 0), kd in res,
                                           res.get(kd, 0), eq3, eq)
            fails[j] = fails[j] or bad
    verdicts_ = [S.VERDICT_BLOCK if b else S.VERDICT_ALLOW for b in fails]
    return next((k for k in range(m) if not fails[k]), -1), verdicts_


# ---- headroom forecast over pages (kt_paged_headroom_forecast): the closed form over a list of page snapshots ----
def paged_headroom_forecast_of(snaps, pod_row, instants, cap, want=1, on_equal=False, ctx=None):
    """kt_paged_headroom_forecast for one pod, in closed form over the page snapshots (no GPU) -> (first, copies [len(instants)],
    limiting [len(instants)]): ``headroom_forecast_of`` on the cluster of all names.  The page rules are ``paged_forecast_of``'s —
    the affecting throttles, the error rows and the pod count are page 0's; the whole-error rule; the whole-threshold rule, with
    ``differs`` formed over EVERY page — and per amount ``_copies_of_amount`` takes the place of the four steps: the throttle's
    number at an instant is the minimum over the pod count (page 0) and every requested name of every page, each page against its
    own reserved row; the answer is the lexicographic minimum of (copies, throttle row).  ``ctx`` is ``paged_preempt_context``'s
    (any ``now``).  With one page this is ``headroom_forecast_of``."""
    snap0 = snaps[0]
    inst = [_instant(t) for t in instants]
    ctx = paged_preempt_context(snaps, inst[0]) if ctx is None else ctx
    p, eq, m, cap = int(pod_row), bool(on_equal), len(inst), int(cap)
    if not (0 <= p < snap0.n_pods) or not int(snap0.pod_flags[p]) & S.POD_VALID:
        return -1, [0] * m, [-1] * m
    err, affected = affected_throttles(snap0, p)
    if err:
        return -1, [0] * m, [-1] * m
    req = {(k, d): v for k, s in enumerate(snaps) for d, v in pod_requests(s, p).items() if v != 0}  # (the pod brings every one)
    best = [(cap, -1)] * m  # (copies, row): affected is ascending, so a strict < keeps the lowest row of a tie
    for t in affected:
        th = ctx["thr"][t]
        f = int(snap0.thr_flags[t])
        eq3 = eq if f & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
        res, res_count = _paged_amounts(snaps, "thr_reserved", t)
        r_hc = res_count is not None
        calc_at_any = any(int(s.thr_flags[t]) & S.THR_CALC_AT_NONZERO for s in snaps)
        if th["error"]:  # the stored status of every page, at every instant
            used, used_count = _paged_amounts(snaps, "thr_used", t)
            sth, sth_count = _paged_amounts(snaps, "thr_calc" if calc_at_any else "thr_spec", t)
            u_hc = used_count is not None
            h = _copies_of_amount(1, True, sth_count is not None, sth_count or 0, used_count or 0, res_count or 0, u_hc or r_hc,
                                  bool(f & S.THR_THROTTLED_POD), eq3, eq, cap)
            for (k, d), v in req.items():
                flg = int(snaps[k].thr_thrl_flag[t]) & int(snaps[k].thr_thrl_has[t])
                h = min(h, _copies_of_amount(v, True, (k, d) in sth, sth.get((k, d), 0), used.get((k, d), 0), res.get((k, d), 0),
                                             (k, d) in used or (k, d) in res, bool(flg >> d & 1), eq3, eq, cap))
            best = [(h, t) if h < b[0] else b for b in best]
            continue
        val, cnt, pods = th["val"], th["cnt"], th["pods"]
        u_hc = pods > 0
        spec, spec_count = _paged_amounts(snaps, "thr_spec", t)
        for j, at in enumerate(inst):
            calc, cc, differs = {}, None, False
            for k, s in enumerate(snaps):
                names, count, any_err = _calculated_threshold(s, t, at)
                stored, stored_count = _amount_dict(s.thr_calc, t, s.D)
                fp = int(s.thr_spec_msgs_fp[t]) if any_err else 0
                differs = differs or names != stored or int(s.thr_status_msgs_fp[t]) != fp
                if k == 0:  # the count is the same in every page
                    cc = count
                    differs = differs or count != stored_count
                calc.update({(k, d): v for d, v in names.items()})
            rd, rd_count = (calc, cc) if calc_at_any or differs else (spec, spec_count)
            h = _copies_of_amount(1, True, rd_count is not None, rd_count or 0, pods if u_hc else 0, res_count or 0, u_hc or r_hc,
                                  cc is not None and u_hc and pods >= cc, eq3, eq, cap)
            for kd, v in req.items():
                u_pr = cnt.get(kd, 0) > 0
                uv = val.get(kd, 0) if u_pr else 0
                cv = calc.get(kd)
                h = min(h, _copies_of_amount(v, True, kd in rd, rd.get(kd, 0), uv, res.get(kd, 0), u_pr or kd in res,
                                             cv is not None and u_pr and uv >= cv, eq3, eq, cap))
            if h < best[j][0]:
                best[j] = (h, t)
    copies = [b[0] for b in best]
    return next((k for k in range(m) if copies[k] >= int(want)), -1), copies, [b[1] for b in best]


# ---- forecast for gangs over pages (kt_paged_forecast_gangs): the closed form over a list of page snapshots ----
def paged_forecast_gangs_of(snaps, member_rows, instants, on_equal=False, ctx=None):
    """kt_paged_forecast_gangs for one gang, in closed form over the page snapshots (no GPU) -> (first, verdicts [len(instants)],
    blockers [len(instants)]): ``forecast_gangs_of`` on the cluster of all names.  ``paged_forecast_of``'s threshold per throttle and
    instant — the whole-error rule and the whole-threshold rule, `differs` over EVERY page — met by the members under the per-page
    reserved prefix of ``paged_preempt_gangs_of``: names are keyed (page, dim), each page's prefix starts from its own stored
    reserved row, a member the throttle affects adds its value of every name it carries, the presence of all of them and count +
    1, and the pod count (threshold, `used`, reserved) is page 0's, judged once.  Which throttles affect which member and "a member
    is an Error or invalid" are page 0's.  ``ctx`` is ``paged_preempt_context``'s (any ``now``: only its sums and error marks are
    read).  With one snapshot this is ``forecast_gangs_of``; with one member ``paged_forecast_of``."""
    snap0 = snaps[0]
    inst = [_instant(t) for t in instants]
    ctx = paged_preempt_context(snaps, inst[0]) if ctx is None else ctx
    members, eq, m = [int(p) for p in member_rows], bool(on_equal), len(inst)
    g = len(members)
    affected, bad_at = [], None  # per member its affecting throttles; the first member that is invalid or an Error
    for j, p in enumerate(members):
        valid = 0 <= p < snap0.n_pods and bool(int(snap0.pod_flags[p]) & S.POD_VALID)
        err, rows = affected_throttles(snap0, p) if valid else (True, [])
        if (err or not valid) and bad_at is None:
            bad_at = j
        affected.append(set(rows))
    keys = [(k, d) for k, s in enumerate(snaps) for d in range(s.D)]
    reqs = [{(k, d): v for k, s in enumerate(snaps) for d, v in pod_requests(s, p).items()} if 0 <= p < snap0.n_pods else {}
            for p in members]
    stopped = [g if bad_at is None else bad_at] * m  # per instant the first member some throttle stops on some page (g: none)
    for t in (sorted(set().union(*affected)) if affected else []):
        th = ctx["thr"][t]
        f = int(snap0.thr_flags[t])
        eq3 = eq if f & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
        res, res_count = _paged_amounts(snaps, "thr_reserved", t)
        hit = [t in a for a in affected]
        calc_at_any = any(int(s.thr_flags[t]) & S.THR_CALC_AT_NONZERO for s in snaps)
        # the whole-error rule, as the kernel states it: the reconcile is an error on some page, or some page holds the row as not
        # valid and responsible (pages built by hand may disagree; page 0 holds it as both, or it would not affect anybody)
        need = S.THR_VALID | S.THR_RESPONSIBLE
        if th["error"] or any((int(s.thr_flags[t]) & need) != need for s in snaps):  # the stored status of every page, at every instant
            used, used_count = _paged_amounts(snaps, "thr_used", t)
            sth = _paged_amounts(snaps, "thr_calc" if calc_at_any else "thr_spec", t)
            names = {}
            for k, d in keys:
                flg = int(snaps[k].thr_thrl_flag[t]) & int(snaps[k].thr_thrl_has[t])
                names[(k, d)] = (bool(flg >> d & 1), (k, d) in used, used.get((k, d), 0))
            j = _gang_first_stopped(members, hit, reqs, sth, (bool(f & S.THR_THROTTLED_POD), used_count is not None, used_count or 0, names),
                                    res, res_count, eq3, eq)
            if j is not None:
                stopped = [min(s, j) for s in stopped]
            continue
        val, cnt, pods = th["val"], th["cnt"], th["pods"]
        spec = _paged_amounts(snaps, "thr_spec", t)
        for i, at in enumerate(inst):
            calc, cc, differs = {}, None, False
            for k, s in enumerate(snaps):
                page_names, count, any_err = _calculated_threshold(s, t, at)
                stored, stored_count = _amount_dict(s.thr_calc, t, s.D)
                fp = int(s.thr_spec_msgs_fp[t]) if any_err else 0
                differs = differs or page_names != stored or int(s.thr_status_msgs_fp[t]) != fp
                if k == 0:  # the count is the same in every page
                    cc = count
                    differs = differs or count != stored_count
                calc.update({(k, d): v for d, v in page_names.items()})
            rd = (calc, cc) if calc_at_any or differs else spec
            names = {}
            for kd in keys:
                u_pr, cv = cnt.get(kd, 0) > 0, calc.get(kd)
                names[kd] = (cv is not None and u_pr and val.get(kd, 0) >= cv, u_pr, val.get(kd, 0))
            j = _gang_first_stopped(members, hit, reqs, rd, (cc is not None and pods > 0 and pods >= cc, pods > 0, pods, names), res, res_count,
                                    eq3, eq)
            if j is not None:
                stopped[i] = min(stopped[i], j)
    if bad_at is not None:
        verdicts_ = [S.VERDICT_ERROR] * m
    else:
        verdicts_ = [S.VERDICT_BLOCK if s < g else S.VERDICT_ALLOW for s in stopped]
    first = next((k for k in range(m) if verdicts_[k] == S.VERDICT_ALLOW), -1)
    return first, verdicts_, [s if s < g else -1 for s in stopped]


# ---- headroom for gangs over pages (kt_paged_headroom_gangs), as the kernel computes it, over a list of page snapshots ----
def paged_headroom_gangs_of(snaps, member_rows, cap, on_equal=False):
    """kt_paged_headroom_gangs for one gang, restated over the page snapshots (no GPU) -> (copies, limiting, blocker position
    inside ``member_rows``): ``headroom_gangs_of`` on the cluster of all names, held to a dry paged gang admission of ``cap``
    consecutive copies.  Which throttles affect which member and "a member is an Error or invalid" are page 0's.  Every
    (throttle, page) pair is a throttle of its own: the page's own threshold (its stored calculatedAt flag; nothing is
    reconciled), `used`, throttled flags and reserved row, A_t of that page (the values and the presence of the names the
    affected members carry THERE); the pod count — threshold, flag, what a copy adds, the int64 cut — is page 0's, judged once,
    and a page k != 0 none of whose names an affected member requests with a non-zero value is skipped.  The candidates of a pair
    end at the running minimum over the pairs before it and where a named amount of the page would leave int64; the first
    failing one is found by the kernel's 64-ary search, and the answer is the lexicographic minimum of (h, first stopped member
    at j = h, t), throttles ascending and the pages inside a throttle.  With one snapshot this is ``headroom_gangs_of``."""
    snap0 = snaps[0]
    members, eq, cap = [int(p) for p in member_rows], bool(on_equal), int(cap)
    affected, bad_at = [], None  # per member its affecting throttles; the first member that is invalid or an Error
    for j, p in enumerate(members):
        valid = 0 <= p < snap0.n_pods and bool(int(snap0.pod_flags[p]) & S.POD_VALID)
        err, rows = affected_throttles(snap0, p) if valid else (True, [])
        if (err or not valid) and bad_at is None:
            bad_at = j
        affected.append(set(rows))
    g = len(members) if bad_at is None else bad_at  # the members that are walked
    members, affected = members[:g], affected[:g]
    page_reqs = [[pod_requests(s, p) for p in members] for s in snaps]
    best = (cap if bad_at is None else 0, g, -1)  # (h, first, t)
    for t in (sorted(set().union(*affected)) if affected else []):
        hit = [t in a for a in affected]
        for k, s in enumerate(snaps):
            reqs = page_reqs[k]
            if k != 0 and not any(hit[j] and v != 0 for j in range(g) for v in reqs[j].values()):
                continue  # nothing on this page is compared
            f = int(s.thr_flags[t])
            eq3 = eq if f & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
            th = _amount_dict(s.thr_calc if f & S.THR_CALC_AT_NONZERO else s.thr_spec, t, s.D)
            used, used_count = _amount_dict(s.thr_used, t, s.D)
            flg = int(s.thr_thrl_flag[t]) & int(s.thr_thrl_has[t])
            names = {d: (bool(flg >> d & 1), d in used, used.get(d, 0)) for d in range(s.D)}
            res, res_count = _amount_dict(s.thr_reserved, t, s.D)
            if k == 0:
                ustate = (bool(f & S.THR_THROTTLED_POD), used_count is not None, used_count or 0, names)
            else:  # the pod count is page 0's: here the threshold does not name it and its flag is false
                th, ustate = (th[0], None), (False, used_count is not None, used_count or 0, names)
            # A_t of this page: only what the threshold names is summed (the rest is never compared)
            per, per_p, per_c = {}, set(), 0
            for j in range(g):
                if hit[j]:
                    per_c += 1
                    for d, v in reqs[j].items():
                        per_p.add(d)
                        if d in th[0]:
                            per[d] = min(per.get(d, 0) + v, _INT64_MAX)
            if th[1] is None:
                per_c = 0

            def first_stopped(j):
                r = {d: res.get(d, 0) + j * per.get(d, 0) for d in (set(res) | per_p if j > 0 else set(res))}
                rc = (res_count or 0) + j * per_c if (res_count is not None or j > 0) else None
                st = _gang_first_stopped(members, hit, reqs, th, ustate, r, rc, eq3, eq)
                return g if st is None else st

            # the range: up to the running minimum, and no further than every named amount of this page stays inside int64
            top = best[0] if best[0] < cap else cap - 1
            if bad_at is None:
                if per_c > 0:
                    top = min(top, (_INT64_MAX - (res_count or 0)) // per_c)
                for d, a in per.items():
                    if a > 0:
                        top = min(top, (_INT64_MAX - res.get(d, 0)) // a)
            lo, known, first = 0, False, g
            while True:  # the 64-ary search for the first candidate in [lo, top] that fails
                hi = top - 1 if known else top
                n = hi - lo + 1
                if n <= 0:
                    break
                step = (n + 63) // 64
                probes = [(j, first_stopped(j)) for j in (hi - (63 - lane) * step for lane in range(64)) if j >= lo]
                fail = next((i for i, (_, st) in enumerate(probes) if st < g), None)
                if fail is None:
                    lo = hi + 1
                    if not known:
                        break
                    continue
                (top, first), known = probes[fail], True
                if fail > 0:
                    lo = probes[fail - 1][0] + 1
            if known and (top, first) < best[:2]:
                best = (top, first, t)
    h, first, t = best
    if bad_at is not None:
        return 0, (t if first < g else -1), first
    return (cap, -1, -1) if h >= cap else (h, t, first)


# ---- headroom forecast for gangs over pages (kt_paged_headroom_forecast_gangs), as the kernel computes it, over page snapshots ----
def paged_headroom_forecast_gangs_of(snaps, member_rows, instants, cap, want=1, on_equal=False, ctx=None):
    """kt_paged_headroom_forecast_gangs for one gang, restated over the page snapshots (no GPU) -> (first, copies [len(instants)],
    limiting [len(instants)], blocker positions inside ``member_rows`` [len(instants)]): ``headroom_forecast_gangs_of`` on the
    cluster of all names.  ``paged_forecast_gangs_of``'s threshold per throttle and instant — the whole-error rule and the
    whole-threshold rule, `differs` over EVERY page, a throttle that keeps its stored status read against the stored calculated
    threshold where calculatedAt is set on some page and against spec otherwise — with ``paged_headroom_gangs_of``'s copies per
    (throttle, page) pair: the page's own reserved row, A_t of that page, the pod count (threshold, flag, what a copy adds, the
    int64 cut) page 0's and judged once, a page k != 0 none of whose names an affected member requests with a non-zero value
    skipped.  Per pair and instant the candidates end at the running minimum and where a named amount of the page would leave
    int64, the first failing one is found by bisection, and per instant the answer is the lexicographic minimum over the pairs of
    (h, first stopped member at j = h, t).  Which throttles affect which member and "a member is an Error or invalid" are page
    0's.  ``ctx`` is ``paged_preempt_context``'s (any ``now``: only its sums and error marks are read).  With one snapshot this is
    ``headroom_forecast_gangs_of``; with one member its first, copies and limiting are ``paged_headroom_forecast_of``'s."""
    snap0 = snaps[0]
    inst = [_instant(t) for t in instants]
    ctx = paged_preempt_context(snaps, inst[0]) if ctx is None else ctx
    members, eq, cap, m = [int(p) for p in member_rows], bool(on_equal), int(cap), len(inst)
    affected, bad_at = [], None  # per member its affecting throttles; the first member that is invalid or an Error
    for j, p in enumerate(members):
        valid = 0 <= p < snap0.n_pods and bool(int(snap0.pod_flags[p]) & S.POD_VALID)
        err, rows = affected_throttles(snap0, p) if valid else (True, [])
        if (err or not valid) and bad_at is None:
            bad_at = j
        affected.append(set(rows))
    g = len(members) if bad_at is None else bad_at  # the members that are walked
    members, affected = members[:g], affected[:g]
    page_reqs = [[pod_requests(s, p) for p in members] for s in snaps]
    start = (cap if bad_at is None else 0, g, -1)  # (h, first, t)
    best, kept = [start] * m, start  # per instant; and over the pairs that keep their stored status

    def judge(reqs, hit, th, ustate, res, res_count, eq3, top):
        """(h, first stopped member at j = h) of one (throttle, page) pair against one threshold and state of `used`, candidates
        up to ``top``; None: it passes there"""
        per, per_p, per_c = {}, set(), 0  # A_t of the page: only what the threshold names is summed (the rest is never compared)
        for j in range(g):
            if hit[j]:
                per_c += 1
                for d, v in reqs[j].items():
                    per_p.add(d)
                    if d in th[0]:
                        per[d] = min(per.get(d, 0) + v, _INT64_MAX)
        if th[1] is None:
            per_c = 0

        def first_stopped(j):
            r = {d: res.get(d, 0) + j * per.get(d, 0) for d in (set(res) | per_p if j > 0 else set(res))}
            rc = (res_count or 0) + j * per_c if (res_count is not None or j > 0) else None
            s = _gang_first_stopped(members, hit, reqs, th, ustate, r, rc, eq3, eq)
            return g if s is None else s

        if bad_at is None:  # no further than every named amount of this page stays inside int64
            if per_c > 0:
                top = min(top, (_INT64_MAX - (res_count or 0)) // per_c)
            for d, a in per.items():
                if a > 0:
                    top = min(top, (_INT64_MAX - res.get(d, 0)) // a)
        first = first_stopped(top)
        if first >= g:
            return None
        lo, hi = 0, top  # hi has been seen to fail, everything below lo passes
        while lo < hi:
            mid = lo + (hi - lo) // 2
            s = first_stopped(mid)
            if s < g:
                hi, first = mid, s
            else:
                lo = mid + 1
        return hi, first

    for t in (sorted(set().union(*affected)) if affected else []):
        th = ctx["thr"][t]
        hit = [t in a for a in affected]
        calc_at_any = any(int(s.thr_flags[t]) & S.THR_CALC_AT_NONZERO for s in snaps)
        # page 0 carries the pod count; elsewhere a page none of whose names an affected member requests stops nobody
        walked = [k == 0 or any(hit[j] and v != 0 for j in range(g) for v in page_reqs[k][j].values()) for k in range(len(snaps))]
        need = S.THR_VALID | S.THR_RESPONSIBLE
        if th["error"] or any((int(s.thr_flags[t]) & need) != need for s in snaps):  # the stored status of every page, at every instant
            for k, s in enumerate(snaps):
                if not walked[k]:
                    continue
                f = int(s.thr_flags[t])
                eq3 = eq if f & S.THR_CLUSTER else True  # throttle_types.go:143 vs clusterthrottle_types.go:45
                sth = _amount_dict(s.thr_calc if calc_at_any else s.thr_spec, t, s.D)
                used, used_count = _amount_dict(s.thr_used, t, s.D)
                flg = int(s.thr_thrl_flag[t]) & int(s.thr_thrl_has[t])
                names = {d: (bool(flg >> d & 1), d in used, used.get(d, 0)) for d in range(s.D)}
                res, res_count = _amount_dict(s.thr_reserved, t, s.D)
                if k == 0:
                    ustate = (bool(f & S.THR_THROTTLED_POD), used_count is not None, used_count or 0, names)
                else:  # the pod count is page 0's: here the threshold does not name it and its flag is false
                    sth, ustate = (sth[0], None), (False, used_count is not None, used_count or 0, names)
                got = judge(page_reqs[k], hit, sth, ustate, res, res_count, eq3, kept[0] if kept[0] < cap else cap - 1)
                if got is not None:
                    kept = min(kept, got + (t,))
            continue
        val, cnt, pods = th["val"], th["cnt"], th["pods"]
        for i, at in enumerate(inst):
            calcs, differs = [], False
            for k, s in enumerate(snaps):
                page_names, count, any_err = _calculated_threshold(s, t, at)
                stored, stored_count = _amount_dict(s.thr_calc, t, s.D)
                fp = int(s.thr_spec_msgs_fp[t]) if any_err else 0
                differs = differs or page_names != stored or int(s.thr_status_msgs_fp[t]) != fp
                if k == 0:  # the count is the same in every page
                    differs = differs or count != stored_count
                calcs.append((page_names, count))
            reads_calc = calc_at_any or differs
            for k, s in enumerate(snaps):
                if not walked[k]:
                    continue
                f = int(s.thr_flags[t])
                eq3 = eq if f & S.THR_CLUSTER else True
                calc, cc = calcs[k]
                rd = (calc, cc) if reads_calc else _amount_dict(s.thr_spec, t, s.D)
                names = {}
                for d in range(s.D):
                    u_pr, cv, uv = cnt.get((k, d), 0) > 0, calc.get(d), val.get((k, d), 0)
                    names[d] = (cv is not None and u_pr and uv >= cv, u_pr, uv)
                if k == 0:
                    ustate = (cc is not None and pods > 0 and pods >= cc, pods > 0, pods, names)
                else:  # the pod count is page 0's
                    rd, ustate = (rd[0], None), (False, pods > 0, pods, names)
                res, res_count = _amount_dict(s.thr_reserved, t, s.D)
                got = judge(page_reqs[k], hit, rd, ustate, res, res_count, eq3, best[i][0] if best[i][0] < cap else cap - 1)
                if got is not None:
                    best[i] = min(best[i], got + (t,))
    copies, limiting, blocker = [], [], []
    for i in range(m):
        h, first, t = min(best[i], kept)
        if bad_at is not None:
            copies.append(0), limiting.append(t if first < g else -1), blocker.append(first)
        elif h >= cap:
            copies.append(cap), limiting.append(-1), blocker.append(-1)
        else:
            copies.append(h), limiting.append(t), blocker.append(first)
    return next((i for i in range(m) if copies[i] >= int(want)), -1), copies, limiting, blocker


class PagedEngine:
    """One HIP engine per page of a ``ClusterState.build_pages()`` result; reconcile and check run on every page (the
    selector scan is repeated per page: the price of more than 16 resource names) and come back combined."""

    def __init__(self, pages, kernel_variant=E.VARIANT_INDEXED, device=-1):
        self.pages = pages
        self.engines = [E.Engine.for_snapshot(b.snapshot, kernel_variant, device) for b in pages]

    def close(self):
        for e in self.engines:
            e.close()

    def reconcile(self, now, apply=True):
        """-> (combined rows, per-page ReconcileResult list).  The step runs through the library's kt_paged_reconcile (what
        a Go host calls); the rows are put together by resource NAME here, which only the host layer knows."""
        results, replaced_any, error_any = E.paged_reconcile(self.engines, now, apply=apply)
        rows = combine_reconcile(self.pages, results)
        for i, r in enumerate(rows):  # the library's OR over the pages is the same statement
            assert r["calc_updated"] == bool(replaced_any[i]) and r["error"] == bool(error_any[i])
        return rows, results

    def check(self, on_equal=False):
        """-> (status matrix [pods][throttles], verdict per pod) of the whole cluster — combined inside the library
        (kt_paged_check: the C-ABI entry point of this module's combination rule)."""
        n = self.pages[0].snapshot.n_pods
        status, summary = E.paged_check(self.engines, n, on_equal=on_equal)
        v = verdicts(status)
        got = np.where(summary == 2, S.VERDICT_ERROR, np.where((summary & 1) != 0, S.VERDICT_BLOCK, S.VERDICT_ALLOW)).astype(np.uint8)
        assert (got == v).all(), "kt_paged_check: summary words disagree with the combined status rows"
        return status, v

    def admit(self, rows=None, on_equal=False, commit=False):
        """The queue ``rows`` (default: every pod row in order) admitted in order through kt_paged_admit: PreFilter at each
        pod's turn against the reserved amounts the pods before it left, Reserve on Success on every page (``commit`` keeps
        the result) -> (status matrix [n][throttles] at each pod's turn, verdict per pod), combined over the pages."""
        if rows is None:
            rows = np.arange(self.pages[0].snapshot.n_pods, dtype=np.int64)
        status, summary = E.paged_admit(self.engines, rows, on_equal=on_equal, commit=commit)
        v = np.where(summary == 2, S.VERDICT_ERROR, np.where((summary & 1) != 0, S.VERDICT_BLOCK, S.VERDICT_ALLOW)).astype(np.uint8)
        ok = v != S.VERDICT_ERROR  # (an error row keeps page 0's precomputed status row; its summary word says error)
        assert (verdicts(status)[ok] == v[ok]).all(), "kt_paged_admit: summary words disagree with the combined status rows"
        return status, v

    def admit_gangs(self, rows, gang_off, on_equal=False, commit=False):
        """The queue ``rows`` in consecutive gangs ``[gang_off[g], gang_off[g + 1])`` through kt_paged_admit_gangs: every gang is
        admitted as a whole or rolled back on every page before the next one starts -> (status matrix [n][throttles] at each
        pod's turn, verdict per pod, admitted byte per gang), combined over the pages."""
        status, summary, admitted = E.paged_admit_gangs(self.engines, rows, gang_off, on_equal=on_equal, commit=commit)
        v = np.where(summary == 2, S.VERDICT_ERROR, np.where((summary & 1) != 0, S.VERDICT_BLOCK, S.VERDICT_ALLOW)).astype(np.uint8)
        ok = v != S.VERDICT_ERROR  # (an error row keeps page 0's precomputed status row; its summary word says error)
        assert (verdicts(status)[ok] == v[ok]).all(), "kt_paged_admit_gangs: summary words disagree with the combined status rows"
        return status, v, admitted

    def admit_gangs_elastic(self, rows, gang_off, min_members, required=None, on_equal=False, commit=False):
        """The queue ``rows`` in consecutive gangs through kt_paged_admit_gangs_elastic: gang g is kept once at least
        ``min_members[g]`` members succeeded and every ``required`` one did, else rolled back on every page before the next one
        starts -> (status matrix [n][throttles] at each pod's turn, verdict per pod, members that stay reserved per gang: 0 rolled
        back), combined over the pages."""
        status, summary, members = E.paged_admit_gangs_elastic(self.engines, rows, gang_off, min_members, required, on_equal=on_equal,
                                                               commit=commit)
        v = np.where(summary == 2, S.VERDICT_ERROR, np.where((summary & 1) != 0, S.VERDICT_BLOCK, S.VERDICT_ALLOW)).astype(np.uint8)
        ok = v != S.VERDICT_ERROR  # (an error row keeps page 0's precomputed status row; its summary word says error)
        assert (verdicts(status)[ok] == v[ok]).all(), "kt_paged_admit_gangs_elastic: summary words disagree with the combined status rows"
        return status, v, members

    def headroom(self, rows, cap, on_equal=False):
        """How many copies of each pod of ``rows`` the throttles still admit, through kt_paged_headroom: the leading Success
        verdicts of a dry-run admission of ``[pod] * cap`` with every page's names -> (copies [n], limiting throttle row [n],
        -1 when all ``cap`` are admitted).  Nothing is reserved."""
        return E.paged_headroom(self.engines, rows, cap, on_equal=on_equal)

    def headroom_gangs(self, pod_rows, gang_off, cap, on_equal=False, want_limiting=True, want_blocker=True):
        """How many copies of each gang ``pod_rows[gang_off[g]:gang_off[g + 1]]`` the throttles still admit as a whole, over every
        page's names, through kt_paged_headroom_gangs (any number of pages; one page goes through the same call): the leading
        admitted gangs of a dry-run paged gang admission of ``members * cap`` -> (copies [n_gangs], limiting throttle row
        [n_gangs] or None, blocker queue position [n_gangs] or None; -1 / -1 when all ``cap`` copies are admitted).  Nothing is
        reserved on any page."""
        return E.paged_headroom_gangs(self.engines, pod_rows, gang_off, cap, on_equal=on_equal, want_limiting=want_limiting,
                                      want_blocker=want_blocker)

    def preempt(self, pod_rows, cand_rows, now, on_equal=False, reprieve=False, want_victims=True):
        """The shortest victim prefix of the caller-ordered ``cand_rows`` that lets each pod of ``pod_rows`` through, over every
        page's names, through kt_paged_preempt (``reprieve``: the victim mask shrunk to a minimal set by the reprieve walk) ->
        (prefix [n], victims [n][n_cand] or None).  A dry run: nothing stored changes on any page."""
        return E.paged_preempt(self.engines, pod_rows, cand_rows, now, on_equal=on_equal, reprieve=reprieve, want_victims=want_victims)

    def preempt_gangs(self, pod_rows, gang_off, cand_rows, now, on_equal=False, reprieve=False, want_victims=True):
        """The shortest victim prefix of the caller-ordered ``cand_rows`` that lets each gang ``pod_rows[gang_off[g]:gang_off[g + 1]]``
        in as a whole, over every page's names, through kt_paged_preempt_gangs (``reprieve``: the victim mask shrunk to a minimal set
        by the reprieve walk) -> (prefix [n_gangs], victims [n_gangs][n_cand] or None, blocker [n_gangs]).  A dry run: nothing
        stored changes on any page."""
        return E.paged_preempt_gangs(self.engines, pod_rows, gang_off, cand_rows, now, on_equal=on_equal, reprieve=reprieve,
                                     want_victims=want_victims)

    def forecast(self, pod_rows, instants, on_equal=False, want_verdicts=True):
        """The first of the strictly ascending ``instants`` at which each pod of ``pod_rows`` passes PreFilter, over every page's
        names, through kt_paged_forecast -> (first [n], verdicts [n][n_inst] or None).  A dry run: nothing stored changes on any
        page."""
        return E.paged_forecast(self.engines, pod_rows, instants, on_equal=on_equal, want_verdicts=want_verdicts)

    def forecast_gangs(self, pod_rows, gang_off, instants, on_equal=False, want_verdicts=True, want_blocker=True):
        """The first of the strictly ascending ``instants`` at which each gang ``pod_rows[gang_off[g]:gang_off[g + 1]]`` is admitted
        as a whole, over every page's names, through kt_paged_forecast_gangs (any number of pages; one page goes through the same
        call) -> (first [n_gangs], verdicts [n_gangs][n_inst] or None, blocker [n_gangs][n_inst] or None).  A dry run: nothing
        stored changes on any page."""
        return E.paged_forecast_gangs(self.engines, pod_rows, gang_off, instants, on_equal=on_equal, want_verdicts=want_verdicts,
                                      want_blocker=want_blocker)

    def headroom_forecast(self, pod_rows, instants, *, cap, want=1, on_equal=False):
        """How many copies of each pod of ``pod_rows`` the throttles admit at each of the strictly ascending ``instants``, over every
        page's names, through kt_paged_headroom_forecast -> (first [n], copies [n][n_inst], limiting [n][n_inst]): the first
        position with at least ``want`` copies, and per instant the lowest throttle row that stops the next copy.  A dry run:
        nothing stored changes on any page."""
        return E.paged_headroom_forecast(self.engines, pod_rows, instants, cap=cap, want=want, on_equal=on_equal)

    def headroom_forecast_gangs(self, pod_rows, gang_off, instants, *, cap, want=1, on_equal=False, want_copies=True, want_limiting=True,
                                want_blocker=True):
        """How many copies of each gang ``pod_rows[gang_off[g]:gang_off[g + 1]]`` the throttles admit as a whole at each of the
        strictly ascending ``instants``, over every page's names, through kt_paged_headroom_forecast_gangs (any number of pages;
        one page goes through the same call) -> (first [n_gangs], copies [n_gangs][n_inst] or None, limiting [n_gangs][n_inst] or
        None, blocker [n_gangs][n_inst] or None): the first position with at least ``want`` copies, and per instant the lowest
        throttle row that stops the next copy and the queue position of the member it stops.  A dry run: nothing stored changes
        on any page."""
        return E.paged_headroom_forecast_gangs(self.engines, pod_rows, gang_off, instants, cap=cap, want=want, on_equal=on_equal,
                                               want_copies=want_copies, want_limiting=want_limiting, want_blocker=want_blocker)

    def override_instants(self, from_, until, cap=None):
        """kt_override_instants of page 0 -> ([(seconds, nanoseconds)], total): every page holds every override's times and parse
        flags, so the instants are the same on every page."""
        return self.engines[0].override_instants(from_, until, cap)

    def fetch_reserved(self) -> list:
        """Reserved amounts per throttle row, put together by resource NAME from the pages (like combine_reconcile):
        {"resourceCounts": {"pod": n}?, "resourceRequests": {name: Fraction}?}."""
        tabs = [e.fetch_reserved() for e in self.engines]
        out = []
        for i in range(len(self.pages[0].thr_names)):
            row = {}
            for b, tab in zip(self.pages, tabs):
                d = b.amount_to_dict(tab, i)
                if "resourceCounts" in d:
                    row["resourceCounts"] = d["resourceCounts"]
                if "resourceRequests" in d:
                    row.setdefault("resourceRequests", {}).update(d["resourceRequests"])
            out.append(row)
        return out
