"""An engine that has lived through events, and what the query family answers on it (not a test file).

Almost every GPU case of the query family builds its engine with ``Engine.for_snapshot``, asks once and closes it.  The plugin does
the opposite: one engine lives for days, is fed pod, Throttle and reservation events, and is asked in between.  This module holds

  * ``Pool``: one small hand-made cluster (three resource names; ``wide=True``: twenty, so two pages) as a pool of pod KINDS and
    throttle KINDS, the pattern of test_match_codes_gpu.Pool — every variant a life needs (another threshold, a moved override
    window, another selector, another namespace) is a throttle kind of its own, so one label and scale dictionary serves all;
  * ``Mirror``: per page one Snapshot of what a freshly loaded engine would be loaded from, edited in place by every event
    (``state[row] -> pod kind`` and ``tstate[row] -> throttle kind``, -1 for a deleted row; the stored status and the reserved
    amounts live in the snapshot's own arrays); ``n_thr`` and ``n_pods`` stay the highest row ever used + 1; the namespace side is
    ``nstate[row] -> namespace kind`` ("gone": no object) with ``ns_valid`` / ``ns_label_*`` arrays of the mirror's own;
  * ``battery``: everything the query family answers for one fixed question set, for both ``on_equal`` values — the headroom
    forecast (first, copies and limiting at every instant of ``INSTANTS``) and, over pages, the paged gang headroom and the paged
    headroom forecast included;
  * ``model_battery``: the same dictionary from the host models (``paging.*_of``) and the oracle, on the mirror alone;
  * ``Life``: the events, applied to the mirror and — when it has engines — to the live engine(s), and ``hold()``: live against a twin
    loaded fresh from the mirror (which side moved?), live against the models (who is right?), live against itself (queries are dry);
  * the lives, each a function of a Life: tests/test_queries_after_events_gpu.py runs them on the GPU, tests/test_lived_engine_cpu.py
    replays them on the mirror alone and asserts they are not vacuous.

Row layouts.  The compact cluster (T_CAP = 24 throttle rows, P_CAP = 64 pod rows, live rows packed from row 0) stays below every
structure that has bitten these kernels: the affected-throttle list is consumed in chunks of 1024 matrix bytes, 16 per lane, and
is filled round by round over the lanes (so it is not in row order once a lane owns two live rows and a higher lane one); every
per-T buffer of a live engine has to grow when its row count passes 1024; pods lie in tiles of 64 rows.  So every life also
runs, unchanged, on a STRETCHED engine of T_PHYS = 1100 x P_PHYS = 4160 rows: ``Life(..., layout=Layout(name, variant))``.

  * ``Layout``: logical throttle row k lives at physical row tmap[k], logical pod row r at pmap[r], both strictly increasing (the
    lowest row is the lowest row in both numberings; a permuted layout would change the answers).  ``STRADDLE`` puts the twelve
    initial throttles on both sides of row 1023/1024 (0 and 1 in one lane with 16 in the next, 15 and 16 neighbours, 1022..1025,
    c-web and c-x in one lane at 1024 and 1025 below ns1/t-web at 1088, the rest a lane apart in chunk 1, appended rows above);
    ``GROW`` ends them exactly at row 1023, so the first row a life appends (1024, 1025, 1040 ...) carries the live engine's row
    count across 1024 between two answered batteries.  ``PMAP`` puts the pods on the edges of tiles 0, 1, 2, 32, 64 and 65.
  * variants: ``holes`` — the rows outside the maps are never fed; ``fillers`` — every second unmapped throttle row below the last
    of the twelve initial ones holds ``c-filler`` (valid, responsible, selector app=filler: no pod carries it) and every second
    unmapped pod row below the highest mapped one holds a pending pod ``filler`` of ns0 (app=idle: no throttle selects it), so the
    program has several term words and views and tiles hold real records between the life's own.  (The throttle fillers stop at
    the twelfth throttle so that on ``grow`` the rows from 1024 on are unborn in both variants.)
  * ``Stretched`` wraps an E.Engine and ``StretchedPages`` the module-level E.paged_* calls: row arguments are mapped on the way in
    (events, pod_rows, cand_rows, gang members), everything that names a throttle row on the way out (limiting rows, the columns of
    status matrices, the rows of fetch_reserved and of reconcile results); queue, candidate and instant positions stay.  Mirror,
    models and lives stay in logical numbering.  ``stretch_snapshot`` builds what a stretched twin is loaded from.
  * two assertions the translation would otherwise hide: in every status matrix of live engine and twin the physical columns
    outside tmap are all zero (``Layout.status``; the row of a pod whose PreFilter is an Error is KT_STATUS_ERROR in EVERY column,
    by the engine's contract and the oracle's, and is exempt as a whole), and the physical matrices of live engine and twin are
    equal byte for byte over all physical columns (``Life.hold``).
  * ``stretched_model_battery``: the models on the stretched mirror, mapped back by the same Layout methods —
    tests/test_lived_engine_cpu.py holds it to the compact mirror's battery (the harness is faithful) and asserts what the layouts cover.

Every comparison is exact: integers and bytes."""
import copy
from types import SimpleNamespace

import numpy as np

import forecast_reference as FR
from kube_throttler_amd import engine as E
from kube_throttler_amd import paging
from kube_throttler_amd import snapshot as S
from kube_throttler_amd.objects import ClusterState
from test_engine_gpu import _gather_pods, _permute_pods, _with_pods, assert_reconcile_equal, _rows_of

NOW = FR.NOW
INSTANTS = FR.instants_under_test()
B = FR.BOUNDARY_TEXTS
CAP = 24
CAPS = (CAP, E.HEADROOM_MAX_CAP)
WANT = 3  # the headroom forecast's `want`: `first` is the first instant with at least so many copies
P_CAP, T_CAP = 64, 24  # capacities of the live engine: above what the cluster starts with
STATUS_BITS = S.THR_CALC_AT_NONZERO | S.THR_THROTTLED_POD
NS = ("ns0", "ns1", "ns2")
GHOST, SPARE = 3, 4  # namespace rows: the one without an object ("ghost"), and the row the live engine keeps spare
NS_CAP = SPARE + 1   # namespace capacity of the live engine
APPS = {"j": "job", "w": "web", "d": "db"}
EXTRA = [f"example.com/r{k:02d}" for k in range(17)]  # wide=True: 3 + 17 names, two pages


# ---- the pool --------------------------------------------------------------------------------------------------------------
def _pod(name, ns, labels, requests, running=False):
    p = {"kind": "Pod", "metadata": {"name": name, "namespace": ns, "labels": dict(labels)},
         "spec": {"schedulerName": "my-scheduler", "containers": [{"name": "c", "resources": {"requests": dict(requests)}}]},
         "status": {"phase": "Running" if running else "Pending"}}
    if running:
        p["spec"]["nodeName"] = "n1"
    return p


def _thr(name, terms, threshold, ns=None, overrides=None):
    kind = "Throttle" if ns else "ClusterThrottle"
    md = {"name": name}
    if ns:
        md["namespace"] = ns
    sel = []
    for labels in terms:
        t = {"podSelector": {"matchLabels": dict(labels)}}
        if not ns:
            t["namespaceSelector"] = {"matchLabels": {"env": "prod"}}
        sel.append(t)
    spec = {"throttlerName": "kube-throttler", "selector": {"selectorTerms": sel}, "threshold": threshold}
    if overrides:
        spec["temporaryThresholdOverrides"] = overrides
    return {"kind": kind, "metadata": md, "spec": spec}


def _rr(**kw):
    names = {"cpu": "cpu", "mem": "memory", "gpu": "amd.com/gpu"}
    return {"resourceRequests": {names[k]: v for k, v in kw.items()}}


def _cnt(n, **kw):
    out = {"resourceCounts": {"pod": n}}
    if kw:
        out.update(_rr(**kw))
    return out


class Pool:
    """The cluster as kinds: ``pod[name]`` / ``thr[name]`` are rows of the pool's snapshots ``snaps`` (one per page).  With
    ``wide=True`` the names sort into cpu, the GPU name and r00..r13 on page 0, r14..r16 and memory on page 1."""

    def __init__(self, wide=False):
        cs = ClusterState()
        cs.add_namespace("ns0", {"env": "prod", "kubernetes.io/metadata.name": "ns0"})
        cs.add_namespace("ns1", {"env": "prod", "kubernetes.io/metadata.name": "ns1"})
        cs.add_namespace("ns2", {"env": "dev", "kubernetes.io/metadata.name": "ns2"})  # (no ClusterThrottle admits it)
        self.pod, self.thr = {}, {}

        def pod(name, *a, **kw):
            self.pod[name] = len(cs.pods)
            cs.add(_pod(name, *a, **kw))

        def thr(name, *a, **kw):
            self.thr[name] = len(cs.throttles)
            cs.add(_thr(name.split("@")[0], *a, **kw))

        # every (namespace, app, team), pending and running: "0jx-p" is the pending job pod of team x in ns0
        cpu = {"j": 300, "w": 200, "d": 500}
        for n, ns in enumerate(NS):
            for a, app in APPS.items():
                for k, team in enumerate("xy"):
                    for running in (False, True):
                        req = {"cpu": f"{cpu[a] + 100 * k + 100 * running}m", "memory": f"{64 * (n + 1)}Mi"}
                        if a == "d":
                            req["amd.com/gpu"] = "1"
                        if wide and a == "w":  # (the web pods carry the names of the second page too)
                            req.update({name: "1" for name in EXTRA})
                        pod(f"{n}{a}{team}-{'r' if running else 'p'}", ns, {"app": app, "team": team}, req, running)
        pod("none", "ns0", {"app": "none"}, {"cpu": "100m", "memory": "64Mi"})                    # nothing matches it
        pod("zero", "ns1", {"app": "job", "team": "x"}, {"cpu": "100m", "amd.com/gpu": "0"})     # carries a name with value 0
        pod("ghost-p", "ghost", {"app": "job", "team": "x"}, {"cpu": "100m"})                     # no Namespace object: Error
        pod("two", "ns0", {"app": "job", "team": "x", "m": "two"}, {"cpu": "100m", "memory": "64Mi"})  # both terms of t-two
        pod("big", "ns0", {"app": "job", "team": "y"}, {"cpu": "5", "memory": "64Mi"})           # more than t-job admits at all
        pod("small", "ns0", {"app": "job", "team": "y"}, {"cpu": "50m", "memory": "32Mi"})       # (an upsert's other requests)
        pod("neg", "ns0", {"app": "web", "team": "y"}, {"cpu": "300m", "memory": "64Mi"}, True)  # (cpu made negative below)
        pod("0wz-r", "ns0", {"app": "web", "team": "z"}, {"cpu": "100m", "memory": "64Mi"}, True)
        pod("neg1", "ns1", {"app": "web", "team": "y"}, {"cpu": "300m", "memory": "128Mi"}, True)  # (memory made negative below)
        pod("filler", "ns0", {"app": "idle"}, {"cpu": "100m"})                                    # (a stretched layout's filler rows)

        win = lambda b, e, th: [{"begin": B[b], "end": B[e], "threshold": th}]
        x = {name: "3" for name in EXTRA[-4:]} if wide else {}  # (c-web's names of both pages)
        # the twelve throttles the cluster starts with (rows 0..11 of the mirror, in this order)
        thr("ns0/t-job", [{"app": "job"}], _rr(cpu="1", mem="1Gi"), ns="ns0")
        thr("ns0/t-web", [{"app": "web"}], _cnt(2), ns="ns0")
        thr("ns1/t-job", [{"app": "job"}], _rr(cpu="1700m"), ns="ns1")
        thr("ns1/t-team", [{"team": "x"}], _cnt(10), ns="ns1")
        thr("ns2/t-db", [{"app": "db"}], _rr(cpu="2", gpu="2"), ns="ns2")
        thr("c-job", [{"app": "job"}], _cnt(8, cpu="3"))
        thr("c-web", [{"app": "web"}], {"resourceRequests": dict(_rr(cpu="1500m")["resourceRequests"], **x)},
            overrides=win(3, 6, _cnt(20, cpu="10")))
        thr("c-x", [{"team": "x"}], _cnt(7), overrides=win(1, 8, _cnt(40)))
        thr("ns0/t-two", [{"m": "two"}, {"app": "job", "team": "x"}], _cnt(4), ns="ns0")
        thr("ns2/t-web", [{"app": "web"}], _rr(mem="256Mi"), ns="ns2")
        thr("c-db", [{"app": "db"}], _rr(gpu="6"))
        thr("ns1/t-web", [{"app": "web"}], _rr(cpu="900m", mem="1Gi"), ns="ns1")
        self.initial = list(self.thr)
        # variants: the same throttle after an event ("name@what")
        thr("ns1/t-job@tight", [{"app": "job"}], _rr(cpu="1"), ns="ns1")                           # a threshold edit
        thr("ns1/t-web@mem", [{"app": "web"}], _rr(cpu="900m", mem="300Mi"), ns="ns1")             # ... of a name of the last page
        thr("c-web@moved", [{"app": "web"}], {"resourceRequests": dict(_rr(cpu="1500m")["resourceRequests"], **x)},
            overrides=win(2, 4, _cnt(20, cpu="10")))                                                # the window moved
        thr("ns0/t-job@ovr", [{"app": "job"}], _rr(cpu="1", mem="1Gi"), ns="ns0", overrides=win(5, 7, _rr(cpu="4", mem="1Gi")))
        thr("c-x@plain", [{"team": "x"}], _cnt(7))                                                  # its override removed
        thr("ns1/t-job@web", [{"app": "web"}], _rr(cpu="2"), ns="ns1")                             # another selector
        thr("ns1/t-team@ns2", [{"team": "x"}], _cnt(10), ns="ns2")                                 # moved to another namespace
        thr("c-none", [{"app": "none"}], _cnt(0))                                                   # blocks the pod nobody blocked
        thr("c-y", [{"team": "y"}], _cnt(5))                                                        # a freed row's next tenant
        thr("ns2/t-web@db", [{"app": "db"}], _rr(mem="256Mi"), ns="ns2")                           # (an unrelated selector change)
        # the web throttles with room: what the running web pods use stays well below, on the names of both pages (the first of
        # c-web's four names lies on page 0 and leaves more room than the three of the last page)
        room = dict({EXTRA[-4]: "40"}, **{name: "17" for name in EXTRA[-3:]}) if wide else {}
        thr("ns0/t-web@room", [{"app": "web"}], _cnt(20), ns="ns0")
        thr("ns1/t-web@room", [{"app": "web"}], _rr(cpu="10", mem="2Gi"), ns="ns1")
        thr("ns1/t-web@room-mem", [{"app": "web"}], _rr(cpu="10", mem="768Mi"), ns="ns1")          # ... and memory edited
        thr("c-web@room", [{"app": "web"}], {"resourceRequests": dict(_rr(cpu="20")["resourceRequests"], **room)},
            overrides=win(3, 6, _cnt(20, cpu="10")))
        thr("ns1/t-job2", [{"app": "job"}], _rr(cpu="1700m"), ns="ns1")                            # ns1/t-job once more: ties with it
        thr("c-x2", [{"team": "x"}], _cnt(7), overrides=win(1, 8, _cnt(40)))                        # c-x once more
        thr("c-filler", [{"app": "filler"}], _cnt(3))                                               # (a stretched layout's filler rows)
        self.cs = cs
        pages = cs.build_pages()
        assert len(pages) == (2 if wide else 1), len(pages)
        self.snaps = [b.snapshot for b in pages]
        self.dims = [b.dims for b in pages]
        self.scales = [b.scales for b in pages]
        for s, dims in zip(self.snaps, self.dims):
            for kind, name in (("neg", "cpu"), ("neg1", "memory")):  # the pods with a negative request, each on one page alone
                if name in dims:
                    k = int(s.pod_ctr_off[self.pod[kind]])
                    s.ctr_req[k, dims[name]] = -s.ctr_req[k, dims[name]]
        # namespace kinds, per page: the label list the pool gives each row, and the ids of env=prod / env=dev
        self.ns_lists, self.env = [], []
        for s in self.snaps:
            assert s.n_ns == GHOST + 1 and list(s.ns_valid[:s.n_ns]) == [1, 1, 1, 0]
            lists = {name: [(int(s.ns_label_key[i]), int(s.ns_label_pair[i])) for i in range(int(s.ns_label_off[r]), int(s.ns_label_off[r + 1]))]
                     for r, name in enumerate(NS)}
            (key, prod), = set(lists["ns0"]) & set(lists["ns1"])            # the one pair the two prod namespaces share
            (dev,) = [p for k, p in lists["ns2"] if k == key]
            assert dev != prod
            self.ns_lists.append(lists)
            self.env.append((key, {"prod": prod, "dev": dev}))

    def ns_kind(self, kind, page=0):
        """A namespace KIND -> (valid, [(key id, pair id)]): "gone" (no object), "ns1" (the labels the pool gives that row),
        "ns2@prod" / "ns0@dev" (... with the env pair swapped: the pool's dictionary has both ids)."""
        if kind == "gone":
            return 0, []
        name, _, env = kind.partition("@")
        key, pairs = self.env[page]
        return 1, [(k, pairs[env] if env and k == key else p) for k, p in self.ns_lists[page][name]]

    # the pods the cluster starts with: row r holds PLACEMENT[r]
    @property
    def placement(self):
        skip = {"neg", "neg1", "small", "filler"}
        return [name for name in self.pod if name not in skip]

    def dim(self, name):
        """(page, dimension) of a resource name"""
        for k, dims in enumerate(self.dims):
            if name in dims:
                return k, dims[name]
        raise KeyError(name)


_POOLS = {}


def pool(wide=False):
    if wide not in _POOLS:
        _POOLS[wide] = Pool(wide)
    return _POOLS[wide]


# ---- the question set ------------------------------------------------------------------------------------------------------
class Questions:
    """Fixed ROWS (events change what they hold): 8 single pods, 4 gangs of 1, 2, 3 and 5 members, 10 candidates; the wide pool has
    a fifth gang (``WEB_GANG``) of two pending web pods, whose names of the last page decide its headroom once the web throttles
    leave room."""
    WEB_GANG = 4

    def __init__(self, pl):
        r = {name: i for i, name in enumerate(pl.placement)}
        self.row = r
        self.pods = np.array([r[n] for n in ("0jx-p", "0wx-p", "1jy-p", "1wx-p", "none", "ghost-p", "big", "zero")], np.int64)
        gangs = [["2jx-p"],                                        # no throttle reaches it
                 ["1jx-p", "zero"],                                # both meet c-x, which has room for one: rolled back
                 ["1jy-p", "0dy-p", "2jy-p"],                      # members that meet different throttles: admitted
                 ["0jy-p", "1wy-p", "2wy-p", "ghost-p", "1dy-p"]]  # a member in the namespace without an object
        if len(pl.snaps) > 1:
            gangs.append(["1wy-p", "0wy-p"])                       # web pods alone: they carry the names of the last page
        self.gang_rows = np.array([r[n] for g in gangs for n in g], np.int64)
        self.gang_off = np.cumsum([0] + [len(g) for g in gangs]).astype(np.int64)
        self.cands = np.array([r[n] for n in ("1jx-r", "0jy-r", "0jx-r", "0wx-r", "0wy-r", "2dx-r", "1wx-r", "1wy-r", "2wx-r", "0dx-r")],
                              np.int64)

    def members(self, g):
        return self.gang_rows[self.gang_off[g]:self.gang_off[g + 1]]


# ---- the mirror ------------------------------------------------------------------------------------------------------------
THR_SPEC_FIELDS = ("thr_ns", "thr_spec", "thr_spec_msgs_fp", "thr_ovr_off", "ovr_begin_s", "ovr_begin_ns", "ovr_end_s", "ovr_end_ns",
                   "ovr_flags", "ovr_thr", "thr_term_off", "term_flags", "term_preq_off", "term_nreq_off", "preq", "nreq")
NS_FIELDS = ("ns_valid", "ns_label_off", "ns_label_key", "ns_label_pair")
POD_FIELDS = ("n_pods", "pod_ns", "pod_flags", "pod_label_off", "pod_label_key", "pod_label_pair", "pod_ctr_off", "ctr_init",
              "ctr_present", "ctr_req", "pod_ovh_present", "pod_ovh")


class Mirror:
    def __init__(self, pl, pod_capacity=P_CAP, thr_capacity=T_CAP):
        self.pl = pl
        self.P, self.T = pod_capacity, thr_capacity
        self.state = np.full(self.P, -1, np.int64)
        self.tstate = np.full(self.T, -1, np.int64)
        self.n_pods = self.n_thr = 0
        self.snaps = []
        for base in pl.snaps:
            m = copy.copy(base)
            m._keep = None
            # the status side lives here, in arrays of the engine's capacity, and is edited in place
            m.thr_flags = np.zeros(self.T, np.uint32)
            for tab in ("thr_used", "thr_calc", "thr_reserved"):
                setattr(m, tab, S.Amounts(self.T, base.D))
            m.thr_thrl_flag, m.thr_thrl_has = np.zeros(self.T, np.uint32), np.zeros(self.T, np.uint32)
            m.thr_status_msgs_fp = np.zeros(self.T, np.uint64)
            self.snaps.append(m)
        # the namespace side: ``nstate[row] -> namespace kind``; every page gets arrays of its own (the pool's are shared)
        self.nstate = list(NS) + ["gone"]
        self.pod_ns = {}  # pod row -> namespace row, where a pod was fed into another namespace than its kind's
        self._refresh_namespaces()
        for m, base in zip(self.snaps, pl.snaps):
            for f in NS_FIELDS:
                assert np.array_equal(getattr(m, f), getattr(base, f)[:len(getattr(m, f))]), f"the mirror starts as the pool: {f}"

    @property
    def snap(self):
        return self.snaps[0]

    # -- namespaces
    def put_namespaces(self, rows, kinds):
        for r, k in zip(rows, kinds):  # (a row named twice: the last wins)
            self._grow_namespaces(int(r) + 1)
            self.nstate[int(r)] = k
        self._refresh_namespaces()

    def drop_namespaces(self, rows):
        self.put_namespaces(rows, ["gone"] * len(rows))

    def _grow_namespaces(self, n):
        self.nstate += ["gone"] * (n - len(self.nstate))

    def namespace_batch(self, kinds, page=0):
        """A namespaces-only batch of these kinds, in this order (for kt_upsert_namespaces)."""
        base = self.pl.snaps[page]
        b = S.Snapshot(base.D, base.L)
        lists = [self.pl.ns_kind(k, page) for k in kinds]
        b.alloc_namespaces(len(kinds), sum(len(l) for _, l in lists))
        b.alloc_pods(0, 0, 0)
        b.alloc_throttles(0, 0, 0)
        n = 0
        for i, (valid, labels) in enumerate(lists):
            b.ns_valid[i] = valid
            for key, pair in labels:
                b.ns_label_key[n], b.ns_label_pair[n] = key, pair
                n += 1
            b.ns_label_off[i + 1] = n
        return b

    def _refresh_namespaces(self):
        for k, m in enumerate(self.snaps):
            b = self.namespace_batch(self.nstate, k)
            m.n_ns = b.n_ns
            for f in NS_FIELDS:
                setattr(m, f, getattr(b, f))
            m._keep = None

    # -- pods
    def put_pods(self, rows, kinds, ns=None):
        """``ns``: the namespace row each pod is fed with (None: its kind's own)."""
        for i, (r, k) in enumerate(zip(rows, kinds)):  # (a row named twice: the last wins)
            self.state[int(r)] = self.pl.pod[k] if isinstance(k, str) else int(k)
            self.n_pods = max(self.n_pods, int(r) + 1)
            self.pod_ns.pop(int(r), None)
            if ns is not None and ns[i] is not None:
                self.pod_ns[int(r)] = int(ns[i])
                if int(ns[i]) >= len(self.nstate):  # a pod in front of its Namespace object: the row exists, without an object
                    self._grow_namespaces(int(ns[i]) + 1)
                    self._refresh_namespaces()
        self._refresh_pods()

    def drop_pods(self, rows):
        for r in rows:
            self.state[int(r)] = -1
            self.pod_ns.pop(int(r), None)
        self._refresh_pods()

    def _refresh_pods(self):
        for m, base in zip(self.snaps, self.pl.snaps):
            w = _with_pods(base, self.state[:self.n_pods])
            for r, ns in self.pod_ns.items():
                w.pod_ns[r] = ns
            for f in POD_FIELDS:
                setattr(m, f, getattr(w, f))

    # -- throttles
    def put_throttles(self, rows, kinds):
        for t, k in zip(rows, kinds):
            self.tstate[int(t)] = self.pl.thr[k]
            self.n_thr = max(self.n_thr, int(t) + 1)
        self._refresh_throttles()

    def drop_throttles(self, rows):
        for t in rows:
            self.tstate[int(t)] = -1
            self._clear_status(int(t))
        self._refresh_throttles()

    def _clear_status(self, t):
        for m in self.snaps:
            for tab in (m.thr_used, m.thr_calc, m.thr_reserved):
                tab.set_row(t, {}, None)
            m.thr_thrl_flag[t] = m.thr_thrl_has[t] = 0
            m.thr_status_msgs_fp[t] = 0
            m.thr_flags[t] = 0

    def _refresh_throttles(self):
        n = self.n_thr
        held = self.tstate[:n] >= 0
        for m, base in zip(self.snaps, self.pl.snaps):
            tb = base.throttle_batch(np.where(held, self.tstate[:n], 0))
            for f in THR_SPEC_FIELDS:
                setattr(m, f, getattr(tb, f))
            m.n_thr = n
            m.thr_flags[:n] = np.where(held, (tb.thr_flags[:n] & ~np.uint32(STATUS_BITS)) | (m.thr_flags[:n] & np.uint32(STATUS_BITS)), 0)
            m._keep = None

    # -- reserved amounts and stored status
    def set_reserved(self, t, kinds, only_page=None):
        """Throttle row t's reserved amount becomes what these pod kinds ask together (``only_page``: on that page alone)."""
        for k, (m, base) in enumerate(zip(self.snaps, self.pl.snaps)):
            if only_page is not None and k != only_page:
                continue
            vals = {}
            for name in kinds:
                for d, v in paging.pod_requests(base, self.pl.pod[name]).items():
                    vals[d] = vals.get(d, 0) + v
            m.thr_reserved.set_row(t, vals, len(kinds))

    def take_reserved(self, reserved, k=0):
        """The totals an admission model returned become page k's reserved table."""
        m = self.snaps[k]
        n = self.n_thr
        for f in ("v", "present", "count", "has_count"):
            getattr(m.thr_reserved, f)[:n] = getattr(reserved, f)[:n]

    def reserved(self, k=0):
        m, n = self.snaps[k], self.n_thr
        return tuple(np.array(getattr(m.thr_reserved, f)[:n]) for f in ("v", "present", "count", "has_count"))

    def reconcile(self, oracle_mod, now=NOW):
        """The oracle's reconcile of every page becomes the stored status (CodesTwin.step's pattern); a calculated threshold is
        replaced as a whole: where some page replaces it, every page has calculatedAt set.  -> per page (rows, result)"""
        out = []
        for m in self.snaps:
            rows = responsible(m)
            want = oracle_mod.Oracle(m).reconcile(now, rows=rows)
            m.apply_status(want.used, want.calc, want.calc_updated, want.thrl_flag, want.thrl_has, want.thrl_pod, want.error, rows=rows)
            out.append((rows, want))
        if len(self.snaps) > 1:
            any_set = np.zeros(self.n_thr, bool)
            for m in self.snaps:
                any_set |= (m.thr_flags[:self.n_thr] & S.THR_CALC_AT_NONZERO) != 0
            for m in self.snaps:
                m.thr_flags[:self.n_thr] |= np.where(any_set, np.uint32(S.THR_CALC_AT_NONZERO), np.uint32(0))
        return out


def responsible(snap):
    need = S.THR_VALID | S.THR_RESPONSIBLE
    return np.nonzero((snap.thr_flags[:snap.n_thr] & need) == need)[0].astype(np.int32)


def load_fields(snap):
    """The fields a load reads, as comparable values (tables cut to the rows in use)."""
    out = {"D": snap.D, "n_ns": snap.n_ns, "n_pods": snap.n_pods, "n_thr": snap.n_thr}
    n, T = snap.n_pods, snap.n_thr
    nl, nc = int(snap.pod_label_off[n]), int(snap.pod_ctr_off[n])
    no, nt = int(snap.thr_ovr_off[T]), int(snap.thr_term_off[T])
    nn = int(snap.ns_label_off[snap.n_ns])
    cut = {"ns_label_key": nn, "ns_label_pair": nn,"pod_ns": n, "pod_flags": n, "pod_label_off": n + 1, "pod_label_key": nl, "pod_label_pair": nl, "pod_ctr_off": n + 1,
           "ctr_init": nc, "ctr_present": nc, "ctr_req": nc, "pod_ovh_present": n, "pod_ovh": n, "thr_flags": T, "thr_ns": T,
           "thr_thrl_flag": T, "thr_thrl_has": T, "thr_status_msgs_fp": T, "thr_spec_msgs_fp": T, "thr_ovr_off": T + 1,
           "ovr_begin_s": no, "ovr_begin_ns": no, "ovr_end_s": no, "ovr_end_ns": no, "ovr_flags": no, "thr_term_off": T + 1,
           "term_flags": nt, "term_preq_off": nt + 1, "term_nreq_off": nt + 1, "ns_valid": snap.n_ns, "ns_label_off": snap.n_ns + 1}
    for f, k in cut.items():
        out[f] = np.asarray(getattr(snap, f))[:k].tobytes()
    for tab, k in (("thr_spec", T), ("thr_calc", T), ("thr_used", T), ("thr_reserved", T), ("ovr_thr", no)):
        a = getattr(snap, tab)
        out[tab] = tuple(np.asarray(getattr(a, f))[:k].tobytes() for f in ("v", "present", "count", "has_count"))
    for name in ("preq", "nreq"):
        op, key, val_off, val = getattr(snap, name).arrays()
        r = len(getattr(snap, name))
        out[name] = (op[:r].tobytes(), key[:r].tobytes(), val_off[:r + 1].tobytes(), val[:int(val_off[r])].tobytes())
    # a deleted pod row is gated by its flags: what lies behind it is not read
    live = (np.asarray(snap.pod_flags)[:n] & S.POD_VALID) != 0
    out["live_rows"] = live.tobytes()
    return out


# ---- row layouts: the same lives on stretched engines -------------------------------------------------------------------------
T_PHYS, P_PHYS = 1100, 65 * 64  # capacities of a stretched live engine: two chunks of the matrix row, 65 tiles of pod rows
CHUNK, LANE, TILE = 1024, 16, 64  # matrix bytes per chunk of the affected-throttle list, bytes per lane, pod rows per tile
# straddle: the twelve initial throttles lie on both sides of the chunk boundary 1023/1024 — rows 0 and 1 share a lane and 16 is
# the next one (the list reads 0, 16, 1), 15 and 16 are neighbouring lanes, 1022..1025 end chunk 0 and begin chunk 1 (c-job at 1023,
# c-web and c-x in ONE lane at 1024 and 1025), the rest lie in chunk 1 a lane apart; the rows a life adds follow above.
STRADDLE = (0, 1, 15, 16, 1022, 1023, 1024, 1025, 1040, 1056, 1072, 1088, 1089, 1090, 1091, 1092, 1094, 1095, 1097, 1099)
# grow: the twelve initial throttles end exactly at row 1023 (c-web and c-x in one lane at 512 and 513), so the first row a life
# adds carries the live engine's row count across 1024 and every per-T buffer has to grow behind answered queries.
GROW = (0, 1, 15, 16, 40, 511, 512, 513, 600, 1021, 1022, 1023, 1024, 1025, 1040, 1041, 1056, 1057, 1072, 1099)
TMAPS = {"straddle": STRADDLE, "grow": GROW}
# the pod map: both ends of tiles 0 and 1, the tile boundaries at 128, 2048 and 4096, and the last row of the last tile (logical
# row 44: the row life_pod_events appends)
PMAP = (0, 1, 62, 63, 64, 65, 127, 128, 129, 200, 300, 511, 512, 1000, 1023, 1024, 1500, 2047, 2048, 2049, 2500, 3000, 3071, 3072,
        3500, 4000, 4031, 4032, 4094, 4095, 4096, 4097, 4100, 4110, 4120, 4127, 4128, 4130, 4140, 4150, 4151, 4152, 4157, 4158, 4159)
VARIANTS = ("holes", "fillers")


def _gather_throttles(entries, D, L):
    """A throttles-only batch whose row i is throttle row t of snapshot s for entries[i] = (s, t); None: an empty row (flags 0).
    (Snapshot.throttle_batch, over several snapshots.)"""
    b = S.Snapshot(D, L)
    b.alloc_namespaces(0, 0)
    b.alloc_pods(0, 0, 0)
    live = [e for e in entries if e is not None]
    b.alloc_throttles(len(entries), int(sum(int(s.thr_ovr_off[t + 1]) - int(s.thr_ovr_off[t]) for s, t in live)),
                      int(sum(int(s.thr_term_off[t + 1]) - int(s.thr_term_off[t]) for s, t in live)))
    pools = {}
    oo = gg = 0
    for i, e in enumerate(entries):
        if e is not None:
            s, t = e
            if id(s) not in pools:
                pools[id(s)] = [tuple(np.asarray(x) for x in paging._pool_arrays(p)) for p in (s.preq, s.nreq)]
            b.thr_flags[i], b.thr_ns[i] = s.thr_flags[t], s.thr_ns[t]
            for tab in ("thr_spec", "thr_calc", "thr_used", "thr_reserved"):
                for f in ("v", "present", "count", "has_count"):
                    getattr(getattr(b, tab), f)[i] = getattr(getattr(s, tab), f)[t]
            b.thr_thrl_flag[i], b.thr_thrl_has[i] = s.thr_thrl_flag[t], s.thr_thrl_has[t]
            b.thr_status_msgs_fp[i], b.thr_spec_msgs_fp[i] = s.thr_status_msgs_fp[t], s.thr_spec_msgs_fp[t]
            for o in range(int(s.thr_ovr_off[t]), int(s.thr_ovr_off[t + 1])):
                for f in ("ovr_begin_s", "ovr_begin_ns", "ovr_end_s", "ovr_end_ns", "ovr_flags"):
                    getattr(b, f)[oo] = getattr(s, f)[o]
                for f in ("v", "present", "count", "has_count"):
                    getattr(b.ovr_thr, f)[oo] = getattr(s.ovr_thr, f)[o]
                oo += 1
            for g in range(int(s.thr_term_off[t]), int(s.thr_term_off[t + 1])):
                b.term_flags[gg] = s.term_flags[g]
                for dst, offs, (op, key, val_off, val) in zip((b.preq, b.nreq), (s.term_preq_off, s.term_nreq_off), pools[id(s)]):
                    for r in range(int(offs[g]), int(offs[g + 1])):
                        dst.add(int(op[r]), int(key[r]), [int(v) for v in val[int(val_off[r]):int(val_off[r + 1])]])
                gg += 1
                b.term_preq_off[gg], b.term_nreq_off[gg] = len(b.preq), len(b.nreq)
        b.thr_ovr_off[i + 1], b.thr_term_off[i + 1] = oo, gg
    return b


def stretch_snapshot(snap, tmap, pmap, T_phys, P_phys, fillers=None):
    """The snapshot a stretched twin is loaded from: ``snap``'s throttle row k at row tmap[k] and its pod row r at row pmap[r],
    namespaces as they are.  ``fillers``: None (the rows outside the maps are empty), or (snapshot, throttle row, pod row, throttle
    rows to fill, pod rows to fill) — every listed row holds a copy of that throttle / that pod."""
    tmap, pmap = np.asarray(tmap, np.int64), np.asarray(pmap, np.int64)
    thr = [None] * (int(tmap[snap.n_thr - 1]) + 1 if snap.n_thr else 0)
    pods = [None] * (int(pmap[snap.n_pods - 1]) + 1 if snap.n_pods else 0)
    if fillers is not None:
        src, ft, fp, thr_rows, pod_rows = fillers
        thr += [None] * max(0, int(max(thr_rows, default=-1)) + 1 - len(thr))
        pods += [None] * max(0, int(max(pod_rows, default=-1)) + 1 - len(pods))
        for t in thr_rows:
            thr[int(t)] = (src, ft)
        for r in pod_rows:
            pods[int(r)] = (src, fp)
    for k in range(snap.n_thr):
        thr[int(tmap[k])] = (snap, k)
    for r in range(snap.n_pods):
        pods[int(pmap[r])] = (snap, r)
    assert len(thr) <= T_phys and len(pods) <= P_phys
    out = copy.copy(snap)
    out._keep = None
    tb = _gather_throttles(thr, snap.D, snap.L)
    for f in THR_SPEC_FIELDS + ("n_thr", "thr_flags", "thr_calc", "thr_used", "thr_reserved", "thr_thrl_flag", "thr_thrl_has",
                                "thr_status_msgs_fp"):
        setattr(out, f, getattr(tb, f))
    empty = np.array([e is None for e in pods], bool)
    pb = _gather_pods([e or (snap, 0) for e in pods])
    pb.pod_flags[:len(pods)][empty] = 0  # (a row that holds nothing is gated by its flags, as a deleted one is)
    for f in POD_FIELDS:
        setattr(out, f, getattr(pb, f))
    return out


class Layout:
    """Logical throttle row k lives at physical row tmap[k], logical pod row r at pmap[r]; both maps are strictly increasing, so
    "the lowest row" is the same row in both numberings.  Translates rows on the way in and everything that names a throttle row
    on the way out; queue positions, candidate positions and instant positions are left as they are."""

    def __init__(self, name, variant):
        assert variant in VARIANTS
        self.name, self.variant = name, variant
        self.tmap, self.pmap = np.array(TMAPS[name], np.int64), np.array(PMAP, np.int64)
        for m, cap in ((self.tmap, T_PHYS), (self.pmap, P_PHYS)):
            assert (np.diff(m) > 0).all() and m[0] >= 0 and m[-1] < cap
        self.tinv = np.full(T_PHYS, -1, np.int64)
        self.tinv[self.tmap] = np.arange(len(self.tmap))
        self.outside = self.tinv < 0
        self.thr_fillers = self.pod_fillers = np.zeros(0, np.int64)
        if variant == "fillers":
            # every second unmapped row: throttles below the last of the twelve initial ones (on `grow` the rows from 1024 on stay
            # unborn until a life adds one), pods below the highest mapped row
            self.thr_fillers = np.setdiff1d(np.arange(self.tmap[11]), self.tmap)[::2]
            self.pod_fillers = np.setdiff1d(np.arange(self.pmap[-1]), self.pmap)[::2]

    def __repr__(self):
        return f"{self.name}-{self.variant}"

    # -- on the way in
    def thr(self, rows):
        return self.tmap[np.asarray(rows, np.int64)].astype(np.int32)

    def pods(self, rows):
        return self.pmap[np.asarray(rows, np.int64)]

    def questions(self, q):
        out = copy.copy(q)
        out.pods, out.gang_rows, out.cands = self.pods(q.pods), self.pods(q.gang_rows), self.pods(q.cands)
        return out

    def stretch(self, snap, base, pl):
        """``snap`` (a page of the mirror) in physical numbering; ``base``: the pool's snapshot of that page (the fillers' kinds)."""
        fillers = (base, pl.thr["c-filler"], pl.pod["filler"], self.thr_fillers, self.pod_fillers) if self.variant == "fillers" else None
        return stretch_snapshot(snap, self.tmap, self.pmap, T_PHYS, P_PHYS, fillers)

    # -- on the way out
    def logical_rows(self, n_phys):
        """The logical row count of an engine with n_phys rows: the map's entries below it."""
        return int(np.searchsorted(self.tmap, n_phys))

    def limiting(self, l):
        l = np.asarray(l)
        back = np.where(l >= 0, self.tinv[np.maximum(l, 0)], l)
        assert (back[l >= 0] >= 0).all(), f"{self}: a limiting row outside the layout: {l}"
        return back.astype(l.dtype)

    def status(self, st, n):
        """A physical status matrix [pods][physical rows] -> its logical columns [pods][n].  The columns outside the map are all
        zero: asserted here, on the physical matrix, because nobody sees them afterwards."""
        assert st.shape[1] == (int(self.tmap[n - 1]) + 1 if n else 0), f"{self}: {st.shape[1]} physical columns for {n} logical rows"
        whole = (st == S.ERROR).all(axis=1)  # (a pod whose PreFilter is an Error: KT_STATUS_ERROR in EVERY column of its row)
        stray = st[~whole][:, self.outside[:st.shape[1]]]
        assert not stray.any(), f"{self}: status outside the layout's rows at physical columns " \
                                f"{np.nonzero(self.outside[:st.shape[1]])[0][np.nonzero(stray.any(axis=0))[0]]}"
        return np.ascontiguousarray(st[:, self.tmap[:n]])

    def amounts(self, a, n):
        return tuple(np.array(getattr(a, f) if hasattr(a, "v") else a[i])[self.tmap[:n]]
                     for i, f in enumerate(("v", "present", "count", "has_count")))

    def battery(self, b, n):
        """A battery in physical numbering -> in logical numbering (n logical throttle rows)."""
        out = {}
        for k, a in b.items():
            name = k if isinstance(k, str) else k[0]
            if isinstance(a[0], str):
                out[k] = a
            elif name in ("check", "check_status", "admit", "admit_gangs"):
                out[k] = (self.status(a[0], n),) + tuple(a[1:])
            elif name == "headroom":
                out[k] = (a[0], self.limiting(a[1]))
            elif name == "headroom_gangs":
                out[k] = (a[0], self.limiting(a[1]), a[2])
            elif name == "headroom_forecast":
                out[k] = (a[0], a[1], self.limiting(a[2]))
            elif name == "reserved":
                out[k] = self.amounts(a, n)
            else:
                out[k] = a
        return out


class Stretched:
    """An E.Engine of capacity T_PHYS x P_PHYS behind a Layout: the lives feed it and ask it in logical numbering.  Every physical
    status matrix it has returned is kept in ``matrices`` (``take_matrices``): Life.hold compares the live engine's with the
    twin's byte for byte over all physical columns."""
    PLAIN = ("close", "compiles", "view_builds", "upsert_namespaces", "upsert_namespace", "delete_namespaces", "override_instants", "D")

    def __init__(self, raw, lay):
        self.raw, self.lay, self.matrices = raw, lay, []

    def __getattr__(self, name):
        if name in Stretched.PLAIN:  # what names no throttle row and no pod row
            return getattr(self.raw, name)
        raise AttributeError(f"Stretched: {name} is not translated")

    def take_matrices(self):
        out, self.matrices = self.matrices, []
        return out

    def throttle_rows(self):
        return self.lay.logical_rows(self.raw.throttle_rows())

    def _status(self, st):
        self.matrices.append(np.array(st))
        return self.lay.status(st, self.throttle_rows())

    # -- events
    def upsert_pods(self, batch, rows):
        self.raw.upsert_pods(batch, rows=self.lay.pods(rows))

    def delete_pods(self, rows):
        self.raw.delete_pods(self.lay.pods(rows))

    def upsert_throttles(self, batch, rows):
        self.raw.upsert_throttles(batch, rows=self.lay.thr(rows))

    def delete_throttles(self, rows):
        self.raw.delete_throttles(self.lay.thr(rows))

    def set_reserved(self, rows, amounts):
        self.raw.set_reserved(self.lay.thr(rows), amounts)

    def set_status(self, rows, *a, **kw):
        self.raw.set_status(self.lay.thr(rows), *a, **kw)

    def _reconciled(self, got):
        return _rows_of(got, self.lay.tmap[:self.throttle_rows()], self.raw.D)

    def reconcile(self, now, apply=True):
        return self._reconciled(self.raw.reconcile(now, apply=apply))

    def reconcile_rows(self, now, rows, apply=True):
        return self._reconciled(self.raw.reconcile_rows(now, self.lay.thr(rows), apply=apply))

    def fetch_reserved(self):
        n = self.throttle_rows()
        out = S.Amounts(n, self.raw.D)
        for f, x in zip(("v", "present", "count", "has_count"), self.lay.amounts(self.raw.fetch_reserved(), n)):
            getattr(out, f)[:n] = x
        return out

    # -- queries
    def check(self, rows, on_equal=False, want_status=True):
        st, sm = self.raw.check(rows=self.lay.pods(rows), on_equal=on_equal, want_status=want_status)
        return (self._status(st) if want_status else None), sm

    def admit(self, rows, on_equal=False, commit=False):
        st, sm = self.raw.admit(rows=self.lay.pods(rows), on_equal=on_equal, commit=commit)
        return self._status(st), sm

    def admit_gangs(self, rows, gang_off, on_equal=False, commit=False):
        st, sm, admitted = self.raw.admit_gangs(self.lay.pods(rows), gang_off, on_equal=on_equal, commit=commit)
        return self._status(st), sm, admitted

    def headroom(self, rows, cap, on_equal=False):
        copies, limiting = self.raw.headroom(rows=self.lay.pods(rows), cap=cap, on_equal=on_equal)
        return copies, self.lay.limiting(limiting)

    def headroom_gangs(self, pod_rows, gang_off, cap, on_equal=False):
        copies, limiting, blocker = self.raw.headroom_gangs(self.lay.pods(pod_rows), gang_off, cap=cap, on_equal=on_equal)
        return copies, self.lay.limiting(limiting), blocker

    def headroom_forecast(self, pod_rows, instants, cap, want=1, on_equal=False):
        first, copies, limiting = self.raw.headroom_forecast(self.lay.pods(pod_rows), instants, cap=cap, want=want, on_equal=on_equal)
        return first, copies, self.lay.limiting(limiting)

    def preempt(self, pod_rows, cand_rows, now, on_equal=False, reprieve=False):
        return self.raw.preempt(self.lay.pods(pod_rows), self.lay.pods(cand_rows), now, on_equal=on_equal, reprieve=reprieve)

    def preempt_gangs(self, pod_rows, gang_off, cand_rows, now, on_equal=False, reprieve=False):
        return self.raw.preempt_gangs(self.lay.pods(pod_rows), gang_off, self.lay.pods(cand_rows), now, on_equal=on_equal, reprieve=reprieve)

    def forecast(self, pod_rows, instants, on_equal=False):
        return self.raw.forecast(self.lay.pods(pod_rows), instants, on_equal=on_equal)

    def forecast_gangs(self, pod_rows, gang_off, instants, on_equal=False):
        return self.raw.forecast_gangs(self.lay.pods(pod_rows), gang_off, instants, on_equal=on_equal)


class StretchedPages:
    """The module-level E.paged_* calls over Stretched page engines, translated the same way (the physical status matrices are
    kept by the first page's engine)."""

    def __init__(self, engs):
        self.first, self.lay = engs[0], engs[0].lay

    @staticmethod
    def _raw(engs):
        return [e.raw for e in engs]

    def paged_reconcile(self, engs, now, apply=True):
        return E.paged_reconcile(self._raw(engs), now, apply=apply)

    def paged_check(self, engs, n, rows, on_equal=False):
        st, sm = E.paged_check(self._raw(engs), n, rows=self.lay.pods(rows), on_equal=on_equal)
        return self.first._status(st), sm

    def paged_admit(self, engs, rows, on_equal=False, commit=False):
        st, sm = E.paged_admit(self._raw(engs), self.lay.pods(rows), on_equal=on_equal, commit=commit)
        return self.first._status(st), sm

    def paged_admit_gangs(self, engs, rows, gang_off, on_equal=False, commit=False):
        st, sm, admitted = E.paged_admit_gangs(self._raw(engs), self.lay.pods(rows), gang_off, on_equal=on_equal, commit=commit)
        return self.first._status(st), sm, admitted

    def paged_headroom(self, engs, rows, cap, on_equal=False):
        copies, limiting = E.paged_headroom(self._raw(engs), self.lay.pods(rows), cap, on_equal=on_equal)
        return copies, self.lay.limiting(limiting)

    def paged_headroom_gangs(self, engs, pod_rows, gang_off, cap, on_equal=False):
        copies, limiting, blocker = E.paged_headroom_gangs(self._raw(engs), self.lay.pods(pod_rows), gang_off, cap, on_equal=on_equal)
        return copies, self.lay.limiting(limiting), blocker

    def paged_headroom_forecast(self, engs, pod_rows, instants, cap, want=1, on_equal=False):
        first, copies, limiting = E.paged_headroom_forecast(self._raw(engs), self.lay.pods(pod_rows), instants, cap=cap, want=want,
                                                            on_equal=on_equal)
        return first, copies, self.lay.limiting(limiting)

    def paged_preempt(self, engs, pod_rows, cand_rows, now, on_equal=False, reprieve=False):
        return E.paged_preempt(self._raw(engs), self.lay.pods(pod_rows), self.lay.pods(cand_rows), now, on_equal=on_equal, reprieve=reprieve)

    def paged_preempt_gangs(self, engs, pod_rows, gang_off, cand_rows, now, on_equal=False, reprieve=False):
        return E.paged_preempt_gangs(self._raw(engs), self.lay.pods(pod_rows), gang_off, self.lay.pods(cand_rows), now,
                                     on_equal=on_equal, reprieve=reprieve)

    def paged_forecast(self, engs, pod_rows, instants, on_equal=False):
        return E.paged_forecast(self._raw(engs), self.lay.pods(pod_rows), instants, on_equal=on_equal)

    def paged_forecast_gangs(self, engs, pod_rows, gang_off, instants, on_equal=False):
        return E.paged_forecast_gangs(self._raw(engs), self.lay.pods(pod_rows), gang_off, instants, on_equal=on_equal)


def paged_api(engs):
    """The E.paged_* entry points for these page engines: the module itself, or its translation for Stretched ones."""
    return StretchedPages(engs) if isinstance(engs[0], Stretched) else E


# ---- the battery -----------------------------------------------------------------------------------------------------------
def _answer(f):
    """An EngineError is recorded as its code, so a refusal compares like a value."""
    try:
        out = f()
    except E.EngineError as err:
        return ("error", err.code)
    out = out if isinstance(out, tuple) else (out,)
    return tuple(x if isinstance(x, (list, int)) else np.array(x) for x in out)


def _amounts(a, n):
    return tuple(np.array(getattr(a, f)[:n]) for f in ("v", "present", "count", "has_count"))


def battery(eng, q, now=NOW):
    """Everything the query family answers for the question set ``q`` on one engine, or on a list of page engines (the paged entry
    points), for both ``on_equal`` values -> {(query, on_equal): arrays | ("error", code)}."""
    if isinstance(eng, (list, tuple)):
        return _paged_battery(list(eng), q, now)
    out = {}
    for eq in (False, True):
        out["check", eq] = _answer(lambda: eng.check(rows=q.pods, on_equal=eq, want_status=True))
        out["admit", eq] = _answer(lambda: eng.admit(rows=q.gang_rows, on_equal=eq, commit=False))
        out["admit_gangs", eq] = _answer(lambda: eng.admit_gangs(q.gang_rows, q.gang_off, on_equal=eq, commit=False))
        for cap in CAPS:
            out["headroom", cap, eq] = _answer(lambda: eng.headroom(rows=q.pods, cap=cap, on_equal=eq))
            out["headroom_gangs", cap, eq] = _answer(lambda: eng.headroom_gangs(q.gang_rows, q.gang_off, cap=cap, on_equal=eq))
            out["headroom_forecast", cap, eq] = _answer(lambda: eng.headroom_forecast(q.pods, INSTANTS, cap=cap, want=WANT, on_equal=eq))
        for rep in (False, True):
            out["preempt", rep, eq] = _answer(lambda: eng.preempt(q.pods, q.cands, now, on_equal=eq, reprieve=rep))
            out["preempt_gangs", rep, eq] = _answer(lambda: eng.preempt_gangs(q.gang_rows, q.gang_off, q.cands, now, on_equal=eq, reprieve=rep))
        out["forecast", eq] = _answer(lambda: eng.forecast(q.pods, INSTANTS, on_equal=eq))
        out["forecast_gangs", eq] = _answer(lambda: eng.forecast_gangs(q.gang_rows, q.gang_off, INSTANTS, on_equal=eq))
    out["override_instants"] = _answer(lambda: eng.override_instants(NOW, FR.BEYOND))
    out["reserved"] = _answer(lambda: _amounts(eng.fetch_reserved(), eng.throttle_rows()))
    return out


def _paged_battery(engs, q, now):
    P = paged_api(engs)
    out = {}
    for eq in (False, True):
        out["check", eq] = _answer(lambda: P.paged_check(engs, len(q.pods), rows=q.pods, on_equal=eq))
        out["check_status", eq] = out["check", eq][:1]
        out["admit", eq] = _answer(lambda: P.paged_admit(engs, q.gang_rows, on_equal=eq, commit=False))
        out["admit_gangs", eq] = _answer(lambda: P.paged_admit_gangs(engs, q.gang_rows, q.gang_off, on_equal=eq, commit=False))
        for cap in CAPS:
            out["headroom", cap, eq] = _answer(lambda: P.paged_headroom(engs, q.pods, cap, on_equal=eq))
            out["headroom_gangs", cap, eq] = _answer(lambda: P.paged_headroom_gangs(engs, q.gang_rows, q.gang_off, cap, on_equal=eq))
            out["headroom_forecast", cap, eq] = _answer(lambda: P.paged_headroom_forecast(engs, q.pods, INSTANTS, cap=cap, want=WANT, on_equal=eq))
        for rep in (False, True):
            out["preempt", rep, eq] = _answer(lambda: P.paged_preempt(engs, q.pods, q.cands, now, on_equal=eq, reprieve=rep))
            out["preempt_gangs", rep, eq] = _answer(lambda: P.paged_preempt_gangs(engs, q.gang_rows, q.gang_off, q.cands, now, on_equal=eq, reprieve=rep))
        out["forecast", eq] = _answer(lambda: P.paged_forecast(engs, q.pods, INSTANTS, on_equal=eq))
        out["forecast_gangs", eq] = _answer(lambda: P.paged_forecast_gangs(engs, q.gang_rows, q.gang_off, INSTANTS, on_equal=eq))
    for k, e in enumerate(engs):
        out["override_instants", k] = _answer(lambda: e.override_instants(NOW, FR.BEYOND))
        out["reserved", k] = _answer(lambda: _amounts(e.fetch_reserved(), e.throttle_rows()))
    return out


def _model_admit_gangs(snap, q, eq, oracle_mod):
    """test_gang_admit_cpu.model_admit_gangs on a Snapshot: every member takes the oracle's in-order step, also behind one that
    failed; a gang with a member that is not Success gives its reservations back."""
    work = copy.copy(snap)
    work._keep = None
    work.thr_reserved = snap.thr_reserved.copy()
    st_all, sm_all, admitted = [], [], []
    for g in range(len(q.gang_off) - 1):
        st, sm, res = oracle_mod.Oracle(work).admit(rows=q.members(g), on_equal=eq)
        valid = (np.asarray(snap.pod_flags)[q.members(g)] & S.POD_VALID) != 0  # (kt_engine.h: an invalid pod row fails its gang)
        ok = bool(((sm & np.uint64(3)) == 0).all() and valid.all())
        if ok:
            for f in ("v", "present", "count", "has_count"):
                getattr(work.thr_reserved, f)[:snap.n_thr] = getattr(res, f)[:snap.n_thr]
            work._keep = None
        st_all.append(st), sm_all.append(sm), admitted.append(ok)
    return np.concatenate(st_all), np.concatenate(sm_all), np.array(admitted, np.uint8)


def _queue_pos(blockers, q):
    """The models name a blocker by its position inside the gang, the engine by its position in the queue."""
    out = np.array(blockers, np.int64)
    off = q.gang_off[:-1].reshape((-1,) + (1,) * (out.ndim - 1))
    return np.where(out >= 0, out + off, out)


def model_battery(mirror, q, oracle_mod, now=NOW):
    """``battery``'s dictionary from the host models and the oracle on the mirror (a paged mirror: the queries the models cover)."""
    snaps = mirror.snaps
    if len(snaps) > 1:
        return _paged_model_battery(mirror, q, oracle_mod, now)
    snap = snaps[0]
    page = [SimpleNamespace(snapshot=snap)]
    ng, m, T = len(q.gang_off) - 1, len(q.cands), snap.n_thr
    ctx = paging.preempt_context(snap, now)
    out = {}
    for eq in (False, True):
        out["check", eq] = _answer(lambda: oracle_mod.Oracle(snap).check(rows=q.pods, on_equal=eq, want_status=True))
        st, sm, _ = oracle_mod.Oracle(snap).admit(rows=q.gang_rows, on_equal=eq)
        out["admit", eq] = (np.array(st), np.array(sm))
        out["admit_gangs", eq] = _model_admit_gangs(snap, q, eq, oracle_mod)
        for cap in CAPS:
            h = [paging.headroom_of(page, p, cap, eq) for p in q.pods]
            out["headroom", cap, eq] = (np.array([x[0] for x in h], np.int64), np.array([x[1] for x in h], np.int32))
            h = [paging.headroom_gangs_of(snap, q.members(g), cap, eq) for g in range(ng)]
            out["headroom_gangs", cap, eq] = (np.array([x[0] for x in h], np.int64), np.array([x[1] for x in h], np.int32),
                                              _queue_pos([x[2] for x in h], q))
            a = [paging.headroom_forecast_of(snap, p, INSTANTS, cap, WANT, eq, ctx=ctx) for p in q.pods]
            out["headroom_forecast", cap, eq] = (np.array([x[0] for x in a], np.int64),
                                                 np.array([x[1] for x in a], np.int64).reshape(len(a), len(INSTANTS)),
                                                 np.array([x[2] for x in a], np.int32).reshape(len(a), len(INSTANTS)))
        for rep in (False, True):
            a = [paging.preempt_of(snap, p, q.cands, now, eq, ctx=ctx, reprieve=rep) for p in q.pods]
            out["preempt", rep, eq] = (np.array([x[0] for x in a], np.int64), np.array([x[1] for x in a], np.uint8).reshape(len(a), m))
            a = [paging.preempt_gangs_of(snap, q.members(g), q.cands, now, eq, ctx=ctx, reprieve=rep) for g in range(ng)]
            out["preempt_gangs", rep, eq] = (np.array([x[0] for x in a], np.int64), np.array([x[1] for x in a], np.uint8).reshape(ng, m),
                                             _queue_pos([x[2] for x in a], q))
        a = [paging.forecast_of(snap, p, INSTANTS, eq, ctx=ctx) for p in q.pods]
        out["forecast", eq] = (np.array([x[0] for x in a], np.int64), np.array([x[1] for x in a], np.uint8))
        a = [paging.forecast_gangs_of(snap, q.members(g), INSTANTS, eq, ctx=ctx) for g in range(ng)]
        out["forecast_gangs", eq] = (np.array([x[0] for x in a], np.int64), np.array([x[1] for x in a], np.uint8),
                                     _queue_pos([x[2] for x in a], q))
    inst = paging.override_instants_of(snap, NOW, FR.BEYOND)
    out["override_instants"] = ([(int(a), int(b)) for a, b in inst], len(inst))
    out["reserved"] = _amounts(snap.thr_reserved, T)
    return out


def _paged_model_battery(mirror, q, oracle_mod, now):
    snaps = mirror.snaps
    pages = [SimpleNamespace(snapshot=s) for s in snaps]
    ng, m = len(q.gang_off) - 1, len(q.cands)
    ctx = paging.paged_preempt_context(snaps, now)
    out = {}
    for eq in (False, True):
        out["check_status", eq] = (paging.combine_status([oracle_mod.Oracle(s).check(rows=q.pods, on_equal=eq)[0] for s in snaps]),)
        for cap in CAPS:
            h = [paging.headroom_of(pages, p, cap, eq) for p in q.pods]
            out["headroom", cap, eq] = (np.array([x[0] for x in h], np.int64), np.array([x[1] for x in h], np.int32))
            h = [paging.paged_headroom_gangs_of(snaps, q.members(g), cap, eq) for g in range(ng)]
            out["headroom_gangs", cap, eq] = (np.array([x[0] for x in h], np.int64), np.array([x[1] for x in h], np.int32),
                                              _queue_pos([x[2] for x in h], q))
            a = [paging.paged_headroom_forecast_of(snaps, p, INSTANTS, cap, WANT, eq, ctx=ctx) for p in q.pods]
            out["headroom_forecast", cap, eq] = (np.array([x[0] for x in a], np.int64),
                                                 np.array([x[1] for x in a], np.int64).reshape(len(a), len(INSTANTS)),
                                                 np.array([x[2] for x in a], np.int32).reshape(len(a), len(INSTANTS)))
        for rep in (False, True):
            a = [paging.paged_preempt_of(snaps, p, q.cands, now, eq, reprieve=rep, ctx=ctx) for p in q.pods]
            out["preempt", rep, eq] = (np.array([x[0] for x in a], np.int64), np.array([x[1] for x in a], np.uint8).reshape(len(a), m))
            a = [paging.paged_preempt_gangs_of(snaps, q.members(g), q.cands, now, eq, reprieve=rep, ctx=ctx) for g in range(ng)]
            out["preempt_gangs", rep, eq] = (np.array([x[0] for x in a], np.int64), np.array([x[1] for x in a], np.uint8).reshape(ng, m),
                                             _queue_pos([x[2] for x in a], q))
        a = [paging.paged_forecast_of(snaps, p, INSTANTS, eq, ctx=ctx) for p in q.pods]
        out["forecast", eq] = (np.array([x[0] for x in a], np.int64), np.array([x[1] for x in a], np.uint8))
        a = [paging.paged_forecast_gangs_of(snaps, q.members(g), INSTANTS, eq, ctx=ctx) for g in range(ng)]
        out["forecast_gangs", eq] = (np.array([x[0] for x in a], np.int64), np.array([x[1] for x in a], np.uint8),
                                     _queue_pos([x[2] for x in a], q))
    for k, s in enumerate(snaps):
        inst = paging.override_instants_of(s, NOW, FR.BEYOND)
        out["override_instants", k] = ([(int(a), int(b)) for a, b in inst], len(inst))
        out["reserved", k] = _amounts(s.thr_reserved, s.n_thr)
    return out


def stretched_model_battery(mirror, q, lay, oracle_mod):
    """``model_battery`` on the STRETCHED mirror — every page's snapshot in physical numbering, the questions' rows mapped in —
    with the answers mapped back by the Layout methods the Stretched engines use -> (battery in logical numbering, the stretched
    snapshots)."""
    snaps = [lay.stretch(m, base, mirror.pl) for m, base in zip(mirror.snaps, mirror.pl.snaps)]
    return lay.battery(model_battery(SimpleNamespace(snaps=snaps), lay.questions(q), oracle_mod), mirror.n_thr), snaps


def reconcile_answer(oracle_mod, snap, rows, now=NOW):
    """The oracle's dry reconcile of these throttle rows, as comparable arrays."""
    w = oracle_mod.Oracle(snap).reconcile(now, rows=np.asarray(rows, np.int32))
    n = len(rows)
    return tuple(np.array(getattr(w, f)[:n]) for f in ("calc_updated", "thrl_flag", "thrl_has", "thrl_pod", "error")) + \
        _amounts(w.used, n) + _amounts(w.calc, n)


def page_zero_alone(mirror, q, cap=CAP):
    """What page 0 alone would answer for the gangs' headroom (``headroom_gangs_of`` on its snapshot), shaped as the battery's
    ``("headroom_gangs", cap, eq)`` -> {eq: answer}.  Where the paged answer differs from it, a name of a later page decides."""
    out = {}
    for eq in (False, True):
        h = [paging.headroom_gangs_of(mirror.snaps[0], q.members(g), cap, eq) for g in range(len(q.gang_off) - 1)]
        out[eq] = (np.array([x[0] for x in h], np.int64), np.array([x[1] for x in h], np.int32), _queue_pos([x[2] for x in h], q))
    return out


def page_zero_alone_forecast(mirror, q, cap=CAP):
    """... and for the pods' headroom forecast (``headroom_forecast_of`` on page 0's snapshot), shaped as the battery's
    ``("headroom_forecast", cap, eq)`` -> {eq: answer}."""
    snap = mirror.snaps[0]
    ctx = paging.preempt_context(snap, NOW)
    out = {}
    for eq in (False, True):
        a = [paging.headroom_forecast_of(snap, p, INSTANTS, cap, WANT, eq, ctx=ctx) for p in q.pods]
        out[eq] = (np.array([x[0] for x in a], np.int64), np.array([x[1] for x in a], np.int64).reshape(len(a), len(INSTANTS)),
                   np.array([x[2] for x in a], np.int32).reshape(len(a), len(INSTANTS)))
    return out


def same(a, b):
    """Two answers, bit for bit."""
    err_a, err_b = isinstance(a[0], str), isinstance(b[0], str)
    if err_a or err_b:
        return err_a and err_b and tuple(a) == tuple(b)
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray) or isinstance(y, np.ndarray):
            x, y = np.asarray(x), np.asarray(y)
            if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
                return False
        elif x != y:
            return False
    return True


def differences(a, b, keys=None):
    """The keys (of ``keys``, default: those of b) at which two batteries differ."""
    return [k for k in (b if keys is None else keys) if k not in a or not same(a[k], b[k])]


def assert_same(a, b, what, keys=None):
    bad = differences(a, b, keys)
    assert not bad, f"{what}: differ at {bad[:6]}\n  {a.get(bad[0])}\n  {b.get(bad[0])}"


# ---- a life ----------------------------------------------------------------------------------------------------------------
class Life:
    """The mirror, and — with ``gpu=True`` — the live engine (one per page), fed by events from empty with spare capacity.  Every
    event is applied to both.  ``hold()`` records the models' battery (``self.held``: [(step name, battery)]); with engines it first
    compares live, twin and models."""

    def __init__(self, oracle_mod, gpu=False, wide=False, layout=None):
        """``layout``: a Layout — the live engine and every twin are Stretched ones (capacities T_PHYS x P_PHYS, on the variant
        "fillers" with the filler rows fed first); the mirror, the models and the lives stay in logical numbering."""
        self.o = oracle_mod
        self.layout = layout
        self.watch = None  # a function (life, step): called by every hold() (tests/test_lived_engine_cpu.py)
        self.pl = pool(wide)
        self.q = Questions(self.pl)
        self.mirror = Mirror(self.pl)
        self.engines = []
        self.held = []
        self.live_held = []
        self.alone = []  # a paged life: [(step name, page_zero_alone)]
        self.alone_forecast = []  # ... [(step name, page_zero_alone_forecast)]
        self.soft = None  # a list: hold() collects what differs there and goes on (a survey of a whole life)
        names = self.pl.placement
        self.mirror.put_throttles(range(len(self.pl.initial)), self.pl.initial)
        self.mirror.put_pods(range(len(names)), names)
        if gpu:
            for m, base in zip(self.mirror.snaps, self.pl.snaps):
                if layout is None:
                    e = E.Engine(base.D, max(base.L, 1), P_CAP, T_CAP, max(base.n_ns, 1) + 1)
                else:
                    e = Stretched(E.Engine(base.D, max(base.L, 1), P_PHYS, T_PHYS, max(base.n_ns, 1) + 1), layout)
                self.engines.append(e)
                e.upsert_namespaces(base)
                if layout is not None and len(layout.thr_fillers):
                    e.raw.upsert_throttles(_gather_throttles([(base, self.pl.thr["c-filler"])] * len(layout.thr_fillers), base.D, base.L),
                                           rows=layout.thr_fillers.astype(np.int32))
                    e.raw.upsert_pods(_permute_pods(base, [self.pl.pod["filler"]] * len(layout.pod_fillers)), rows=layout.pod_fillers)
                e.upsert_throttles(m.throttle_batch(np.arange(m.n_thr)), rows=np.arange(m.n_thr))
                e.upsert_pods(_permute_pods(base, self.mirror.state[:len(names)]), rows=np.arange(len(names)))

    @property
    def eng(self):
        return self.engines[0]

    def close(self):
        for e in self.engines:
            e.close()
        self.engines = []

    def row(self, name):
        return self.q.row[name]

    def compiles(self):
        return [e.compiles() for e in self.engines]

    # -- events
    def upsert_namespaces(self, rows, kinds):
        """kt_upsert_namespaces with ``rows=``: the batch holds the kinds in the order given (a row named twice included)."""
        for k, e in enumerate(self.engines):
            e.upsert_namespaces(self.mirror.namespace_batch(kinds, k), rows=np.asarray(rows, np.int32))
        self.mirror.put_namespaces(rows, kinds)

    def delete_namespaces(self, rows):
        for e in self.engines:
            e.delete_namespaces(np.asarray(rows, np.int32))
        self.mirror.drop_namespaces(rows)

    def upsert_namespace_flat(self, row, kind):
        """kt_upsert_namespace(row, exists, ...): the call the plugin mirror uses."""
        for k, e in enumerate(self.engines):
            valid, labels = self.pl.ns_kind(kind, k)
            e.upsert_namespace(row, valid, [key for key, _ in labels], [pair for _, pair in labels])
        self.mirror.put_namespaces([row], [kind])

    def upsert_pods(self, rows, kinds, ns=None):
        """``ns``: the namespace rows the pods are fed with (None: their kinds' own)."""
        rows = np.asarray(rows, np.int64)
        src = np.array([self.pl.pod[k] for k in kinds], np.int64)
        for e, base in zip(self.engines, self.pl.snaps):
            b = _permute_pods(base, src)
            for i, x in enumerate(ns or ()):
                if x is not None:
                    b.pod_ns[i] = x
            e.upsert_pods(b, rows=rows)
        self.mirror.put_pods(rows, kinds, ns)

    def delete_pods(self, rows):
        for e in self.engines:
            e.delete_pods(np.asarray(rows, np.int64))
        self.mirror.drop_pods(rows)

    def upsert_throttles(self, rows, kinds):
        self.mirror.put_throttles(rows, kinds)
        for e, m in zip(self.engines, self.mirror.snaps):
            e.upsert_throttles(m.throttle_batch(np.asarray(rows)), rows=np.asarray(rows, np.int32))

    def delete_throttles(self, rows):
        for e in self.engines:
            e.delete_throttles(np.asarray(rows, np.int32))
        self.mirror.drop_throttles(rows)

    def set_reserved(self, t, kinds, only_page=None):
        self.mirror.set_reserved(t, kinds, only_page)
        for e, m in zip(self.engines, self.mirror.snaps):
            a = S.Amounts(1, m.D)
            for f in ("v", "present", "count", "has_count"):
                getattr(a, f)[0] = getattr(m.thr_reserved, f)[t]
            e.set_reserved(np.array([t], np.int32), a)

    def set_used(self, t, name, value):
        """kt_set_status from the host: one throttle's `used` of one name is raised (the rest of its status as stored)."""
        k, d = self.pl.dim(name)
        m = self.mirror.snaps[k]
        m.thr_used.v[t, d] = value
        m.thr_used.present[t] |= np.uint32(1 << d)
        for e, m in zip(self.engines, self.mirror.snaps):
            used, calc = S.Amounts(1, m.D), S.Amounts(1, m.D)
            for f in ("v", "present", "count", "has_count"):
                getattr(used, f)[0] = getattr(m.thr_used, f)[t]
                getattr(calc, f)[0] = getattr(m.thr_calc, f)[t]
            fl = int(m.thr_flags[t])
            e.set_status(np.array([t], np.int32), used, calc, [1 if fl & S.THR_CALC_AT_NONZERO else 0], [m.thr_thrl_flag[t]],
                         [m.thr_thrl_has[t]], [1 if fl & S.THR_THROTTLED_POD else 0], msgs_fp=[m.thr_status_msgs_fp[t]])

    def reconcile(self, now=NOW):
        """reconcile(apply) on the live engine, the oracle's status into the mirror; the two are compared on the way."""
        want = self.mirror.reconcile(self.o, now)
        if len(self.engines) == 1:
            got = self.eng.reconcile(now, apply=True)
            rows, w = want[0]
            assert_reconcile_equal(_rows_of(got, rows, self.mirror.snap.D), w, len(rows))
        elif self.engines:
            paged_api(self.engines).paged_reconcile(self.engines, now, apply=True)

    def admit_commit(self, rows, on_equal=False):
        """admit(commit=True) of a short queue: the mirror takes the admission model's reservation."""
        rows = np.asarray(rows, np.int64)
        snap = self.mirror.snap
        st, sm, res = self.o.Oracle(snap).admit(rows=rows, on_equal=on_equal)
        if self.engines:
            got = _answer(lambda: self.eng.admit(rows=rows, on_equal=on_equal, commit=True))
            assert same(got, (np.array(st), np.array(sm))), f"admit(commit): {got} against the oracle's {(st, sm)}"
        self.mirror.take_reserved(res)
        return sm

    def admit_gangs_commit(self, q, on_equal=False):
        snap = self.mirror.snap
        want = _model_admit_gangs(snap, q, on_equal, self.o)
        work = copy.copy(snap)
        work.thr_reserved = snap.thr_reserved.copy()
        for g in range(len(q.gang_off) - 1):  # the admitted gangs' reservations, gang by gang
            if want[2][g]:
                work._keep = None
                _, _, res = self.o.Oracle(work).admit(rows=q.members(g), on_equal=on_equal)
                for f in ("v", "present", "count", "has_count"):
                    getattr(work.thr_reserved, f)[:snap.n_thr] = getattr(res, f)[:snap.n_thr]
        if self.engines:
            got = _answer(lambda: self.eng.admit_gangs(q.gang_rows, q.gang_off, on_equal=on_equal, commit=True))
            assert same(got, want), f"admit_gangs(commit): {got} against the model's {want}"
        self.mirror.take_reserved(work.thr_reserved)
        return want[2]

    # -- hold
    def twin(self):
        if self.layout is None:
            return [E.Engine.for_snapshot(m) for m in self.mirror.snaps]
        return [Stretched(E.Engine.for_snapshot(self.layout.stretch(m, base, self.pl)), self.layout)
                for m, base in zip(self.mirror.snaps, self.pl.snaps)]

    def hold(self, step, refused=(), live_refuses=()):
        """``refused``: query names the engine answers KT_ERR_UNSUPPORTED on live AND twin (the models are not asked);
        ``live_refuses``: ... on the live engine only — the twin serves them and is held to the models."""
        model = model_battery(self.mirror, self.q, self.o)
        self.held.append((step, model))
        if len(self.mirror.snaps) > 1:
            self.alone.append((step, page_zero_alone(self.mirror, self.q)))
            self.alone_forecast.append((step, page_zero_alone_forecast(self.mirror, self.q)))
        if self.watch is not None:
            self.watch(self, step)
        if not self.engines:
            return model
        target = self.engines if len(self.engines) > 1 else self.eng
        if self.layout is not None:
            self.engines[0].take_matrices()  # (what committed admissions since the last hold left there)
        live = battery(target, self.q)
        tw = self.twin()
        try:
            twin = battery(tw if len(tw) > 1 else tw[0], self.q)
        finally:
            for e in tw:
                e.close()
        problems = []
        if self.layout is not None:  # the physical status matrices, over all physical columns (the first page's engine keeps them)
            a, b = self.engines[0].take_matrices(), tw[0].take_matrices()
            assert len(a) == len(b) and len(a) >= 6, (len(a), len(b))
            for i, (x, y) in enumerate(zip(a, b)):
                if x.shape != y.shape or x.tobytes() != y.tobytes():
                    problems.append(f"{step}: physical status matrix number {i} of the battery: live {x.shape} and twin {y.shape} differ"
                                    + (f" at physical columns {np.nonzero((x != y).any(axis=0))[0]}" if x.shape == y.shape else ""))
        again = battery(target, self.q)
        if self.layout is not None:
            self.engines[0].take_matrices()

        def expect(x, y, what, keys=None):
            bad = differences(x, y, keys)
            if bad:
                problems.append(f"{step}: {what}: differ at {bad[:8]}\n  {x.get(bad[0])}\n  {y.get(bad[0])}")

        expect(live, again, "a second run of the battery on the live engine (queries are dry)")
        unsupported = ("error", -7)
        plain = [k for k in live if k[0] not in refused and k[0] not in live_refuses]
        for k in live:
            if k[0] in refused and not (live[k] == unsupported and twin[k] == unsupported):
                problems.append(f"{step}: {k}: live {live[k]}, twin {twin[k]}: both refuse it")
            elif k[0] in live_refuses and live[k] != unsupported:
                problems.append(f"{step}: {k}: live {live[k]}: the live engine refuses it")
        assert set(live) == set(twin)
        expect(live, twin, "live engine against a twin loaded fresh from the mirror", plain)
        expect(twin, model, "twin against the host models", [k for k in model if k[0] not in refused])
        expect(live, model, "live engine against the host models", [k for k in model if k in plain])
        if self.soft is None:
            assert not problems, "\n".join(problems)
        self.soft = None if self.soft is None else self.soft + problems
        self.live_held.append((step, live))
        return live


# ---- the lives: every step is named --------------------------------------------------------------------------------------------
def start(life):
    life.reconcile()
    life.hold("start")


def life_pod_events(life):
    r = life.row
    start(life)
    life.upsert_pods([r("0jy-r")], ["0jx-r"])               # other requests (and another team) in a candidate's row
    life.hold("an upsert changes the requests of a candidate's row")
    life.upsert_pods([r("1jy-p")], ["1jy-r"])               # a gang member (and single pod) becomes running ...
    life.hold("a pending gang member becomes running")
    life.upsert_pods([r("1jy-p")], ["1jy-p"])               # ... and pending again
    life.hold("... and pending again")
    n = life.mirror.n_pods
    life.upsert_pods([n + 2], ["1jy-r"])                    # beyond pod_rows_hi (row n and n + 1 stay empty)
    life.hold("a row is appended beyond pod_rows_hi")
    life.delete_pods([r("0dy-p"), r("0jx-r")])              # a member of gang 2 and a candidate
    life.hold("a delete hits a gang member and a candidate")
    life.upsert_pods([r("0dy-p")], ["1dx-r"])               # the freed row: a pod of another namespace
    life.hold("the freed row is reused by a pod of another namespace")
    life.upsert_pods([r("0wx-r"), r("none"), r("0wx-r")], ["0wy-p", "0wz-r", "small"])  # one batch names a row twice: the last wins
    life.hold("one batch names a row twice")


def life_threshold_and_override_events(life):
    t = {name: i for i, name in enumerate(life.pl.initial)}
    start(life)
    compiles = life.eng.compiles() if life.engines else None

    def step(name):
        life.hold(name)  # (no reconcile: the stored status is the old one, on the engine and in the mirror)
        if life.engines:
            assert life.eng.compiles() == compiles, f"{name}: {life.eng.compiles()} compiles, {compiles} before"

    life.upsert_throttles([t["ns1/t-job"]], ["ns1/t-job@tight"])
    step("a threshold edit moves the limiting throttle of a headroom answer")
    life.upsert_throttles([t["c-web"]], ["c-web@moved"])
    step("an override window is moved")
    life.upsert_throttles([t["ns0/t-job"]], ["ns0/t-job@ovr"])
    step("an override is added to a throttle that had none")
    life.upsert_throttles([t["c-x"]], ["c-x@plain"])
    step("an override is removed")
    life.reconcile()
    step("one reconcile(apply) behind the four events")


def life_selector_and_row_events(life):
    t = {name: i for i, name in enumerate(life.pl.initial)}
    start(life)
    compiles = [life.eng.compiles() if life.engines else 0]

    def step(name):
        life.hold(name)
        if life.engines:
            assert life.eng.compiles() == compiles[0] + 1, f"{name}: {life.eng.compiles()} compiles, {compiles[0]} before"
            compiles[0] += 1

    life.upsert_throttles([t["ns1/t-job"]], ["ns1/t-job@web"])      # right after reconcile(apply): the device's status is newer
    step("a throttle's selector changes right after reconcile(apply)")
    life.reconcile()
    life.upsert_throttles([t["ns1/t-team"]], ["ns1/t-team@ns2"])
    step("a throttle moves namespace")
    life.reconcile()
    new = life.mirror.n_thr + 1                                     # beyond thr_rows_hi (a row stays empty in between)
    life.upsert_throttles([new], ["c-none"])
    step("a new throttle appears in a row beyond thr_rows_hi")
    life.reconcile()
    life.delete_throttles([t["c-x"]])                               # the row that limited gang 1
    step("delete_throttles removes the row that limited a gang")
    life.reconcile()
    life.upsert_throttles([t["c-x"]], ["c-y"])
    step("the freed row is reused by a ClusterThrottle")
    life.reconcile()
    life.hold("... and has been reconciled too")


def life_reservations_survive(life):
    t = {name: i for i, name in enumerate(life.pl.initial)}
    r = life.row
    start(life)
    life.set_reserved(t["ns1/t-job"], ["1jx-p"])
    life.set_reserved(t["c-db"], ["0dx-p"])
    life.hold("set_reserved on two rows")
    life.admit_gangs_commit(life.q)
    life.hold("admit_gangs(commit=True)")
    life.admit_commit([r("0dx-p"), r("1wx-p"), r("none"), r("1jy-p"), r("two")])
    life.hold("admit(commit=True) on a short queue")
    life.upsert_throttles([t["ns2/t-web"]], ["ns2/t-web@db"])       # reserved amounts the device advanced go to the host and back
    life.hold("a selector-changing throttle event of an unrelated row")
    life.reconcile()
    used =int(life.mirror.snap.thr_used.v[t["ns1/t-web"], life.pl.dim("cpu")[1]])
    life.set_used(t["ns1/t-web"], "cpu", used + 150)
    life.hold("a set_status from the host raises one throttle's used")


def life_negative_came_and_went(life):
    start(life)
    n = life.mirror.n_pods
    life.upsert_pods([n], ["neg"])
    life.hold("a pod with a negative request is there", refused=("headroom_gangs",))
    life.reconcile()
    life.hold("... and has been reconciled", refused=("headroom_gangs",))
    life.delete_pods([n])
    life.hold("the pod with the negative request is gone", live_refuses=("headroom_gangs",))
    life.reconcile()
    life.hold("... and a reconcile behind it", live_refuses=("headroom_gangs",))


def life_two_pages(life):
    t = {name: i for i, name in enumerate(life.pl.initial)}
    r = life.row
    start(life)
    life.upsert_pods([r("1wy-p")], ["1wx-r"])
    life.hold("a pod upsert")
    life.delete_pods([r("0wx-r")])
    life.hold("a pod delete")
    life.upsert_pods([r("0wx-r")], ["1wy-r"])
    life.hold("the row is reused")
    life.set_reserved(t["ns1/t-web"], ["1wx-p"], only_page=1)
    life.hold("set_reserved on page 1")
    life.upsert_throttles([t["ns1/t-web"]], ["ns1/t-web@mem"])
    life.hold("a threshold edit on page 1")
    life.reconcile()
    life.hold("a reconcile behind them")


PAGE_ONE_STEPS = ("set_reserved on page 1 takes a copy of the web gang", "a threshold edit of a last-page name, reconciled",
                  "a pod event changes a member's request of a last-page name", "set_reserved on page 0: the decider moves to page 0",
                  "set_reserved on page 1: the decider moves back to page 1")


def life_page_one_decides(life):
    """The web gang (``Questions.WEB_GANG``) on web throttles that leave room: its headroom is decided by names of the last page,
    and every step named in PAGE_ONE_STEPS moves it (tests/test_lived_engine_cpu.py asserts that on the models)."""
    t = {name: i for i, name in enumerate(life.pl.initial)}
    r = life.row
    start(life)
    life.upsert_throttles([t["ns0/t-web"], t["c-web"], t["ns1/t-web"]], ["ns0/t-web@room", "c-web@room", "ns1/t-web@room"])
    life.reconcile()
    life.hold("the web throttles leave room, reconciled: page 1 decides the web gang")
    life.set_reserved(t["c-web"], ["1wx-p", "0wx-p"], only_page=1)      # two pods' worth of c-web's names of the last page
    life.hold(PAGE_ONE_STEPS[0])
    life.upsert_throttles([t["ns1/t-web"]], ["ns1/t-web@room-mem"])     # memory is a name of the last page: ns1/t-web limits now
    life.reconcile()
    life.hold(PAGE_ONE_STEPS[1])
    life.upsert_pods([r("1wy-p")], ["0wy-p"], ns=[1])                    # same namespace, labels and cpu; half the memory
    life.hold(PAGE_ONE_STEPS[2])
    life.set_reserved(t["ns0/t-web"], ["0wx-p"] * 14, only_page=0)      # the pod count is page 0's
    life.hold(PAGE_ONE_STEPS[3])
    life.set_reserved(t["c-web"], ["1wx-p", "0wx-p"] * 5, only_page=1)
    life.hold(PAGE_ONE_STEPS[4])


def life_negative_on_page_one(life):
    """life_negative_came_and_went on two pages: the negative request is of a name of the last page, so page 1's engine alone is
    fed one — the paged gang headroom is refused as a whole."""
    start(life)
    n = life.mirror.n_pods
    life.upsert_pods([n], ["neg1"])
    life.hold("a pod with a negative request of a last-page name is there", refused=("headroom_gangs",))
    life.reconcile()
    life.hold("... and has been reconciled", refused=("headroom_gangs",))
    life.delete_pods([n])
    life.hold("the pod with the negative request is gone", live_refuses=("headroom_gangs",))
    life.reconcile()
    life.hold("... and a reconcile behind it", live_refuses=("headroom_gangs",))


def life_rows_appended(life):
    """Throttle rows appended behind the twelve (on the layout `grow`: the first of them carries the row count across 1024), each a
    second copy of a throttle that limits an answer: same selector, same threshold, so the same number of copies from a row far
    above — a tie, and the lower row is the one to report.  Then the lower row goes (the far row limits alone) and returns."""
    t = {name: i for i, name in enumerate(life.pl.initial)}
    start(life)
    n = life.mirror.n_thr
    life.upsert_throttles([n], ["ns1/t-job2"])
    life.reconcile()
    life.hold("a second ns1/t-job is appended and reconciled")
    life.upsert_throttles([n + 1, n + 3], ["c-x2", "c-y"])   # one batch, two rows, one row stays empty in between
    life.reconcile()
    life.hold("one batch appends a second c-x and c-y")
    life.delete_throttles([t["ns1/t-job"], t["c-x"]])
    life.hold("the lower rows of both ties are deleted")
    life.upsert_throttles([t["ns1/t-job"], t["c-x"]], ["ns1/t-job", "c-x"])
    life.reconcile()
    life.hold("... and return")
    life.delete_throttles([n, n + 1])
    life.hold("the appended copies are deleted")


class _Gaps:
    """compiles() of every page's engine from one hold to the next: a gap that holds namespace events (or a pod of a namespace row
    the program was not compiled for) costs exactly ONE compile, however many events it holds; a gap without events costs none."""

    def __init__(self, life):
        self.life = life
        self.at = life.compiles()

    def hold(self, name, compiled, **kw):
        out = self.life.hold(name, **kw)
        now = self.life.compiles()
        want = [c + (1 if compiled else 0) for c in self.at]
        assert now == want, f"{name}: compiles() {now}, {self.at} at the step before"
        self.at = now
        return out


def _assert_battery_is(life, step, then):
    """The battery held last equals the one held at step number ``then``, byte for byte: models, and the live engine where there is one."""
    assert_same(life.held[-1][1], life.held[then][1], f"{step}: the models' battery against the one of '{life.held[then][0]}'")
    if life.engines:
        assert_same(life.live_held[-1][1], life.live_held[then][1], f"{step}: the live battery against the one of '{life.held[then][0]}'")


def life_namespace_labels(life):
    start(life)
    g = _Gaps(life)
    life.upsert_namespaces([2], ["ns2@prod"])               # the ClusterThrottles now reach the pods of ns2
    g.hold("ns2 becomes prod", True)
    life.reconcile()
    g.hold("... and has been reconciled", False)
    life.upsert_namespaces([0], ["ns0@dev"])
    g.hold("ns0 becomes dev", True)
    life.reconcile()
    g.hold("... and has been reconciled too", False)
    life.upsert_namespaces([2, 0], ["ns2", "ns0"])          # one batch, two rows
    life.reconcile()
    g.hold("both changes are undone in one batch, and a reconcile behind it", True)
    _assert_battery_is(life, "labels and status are those of the start", 0)
    life.upsert_namespaces([1, 2, 1], ["ns1@dev", "ns2@prod", "ns1"])  # one batch names a row twice: the last wins, ns1 stays prod
    g.hold("one batch names a row twice", True)
    _assert_battery_is(life, "ns1 named twice, as it was: what ns2 -> prod alone gave", 1)


def life_namespace_deleted_and_back(life):
    start(life)
    g = _Gaps(life)
    life.delete_namespaces([1])                             # its pods, gang members and candidates: Error among the answers
    g.hold("delete_namespaces takes the object of ns1", True)
    life.upsert_namespaces([1], ["ns1"])
    g.hold("the object returns with its old labels", True)
    _assert_battery_is(life, "ns1 is back", 0)
    life.upsert_namespaces([1], ["gone"])                   # the same state, reached by ns_valid = 0 ...
    g.hold("upsert_namespaces with ns_valid = 0", True)
    _assert_battery_is(life, "ns_valid = 0", 1)
    life.upsert_namespace_flat(1, "ns1")
    g.hold("the object returns through the flat form", True)
    _assert_battery_is(life, "ns1 is back again", 0)
    life.upsert_namespace_flat(1, "gone")                   # ... and by the flat form with exists = 0
    g.hold("the flat form with exists = 0", True)
    _assert_battery_is(life, "exists = 0", 1)
    life.reconcile()
    g.hold("a reconcile while the object is gone", False)
    life.upsert_namespaces([1], ["ns1@dev"])
    g.hold("the object returns with other labels", True)  # (a reconcile behind it moves nothing: no ClusterThrottle counts ns1 either way)


def life_namespace_arrives_after_its_pods(life):
    r = life.row
    start(life)
    g = _Gaps(life)
    life.upsert_namespaces([GHOST], ["ns0"])                # ghost-p and the gang that held an Error member are judged now
    g.hold("the namespace without an object gets one", True)
    life.upsert_pods([r("0jy-r")], ["0jy-r"], ns=[GHOST])   # (the only pod there was pending: a reconcile alone would move nothing)
    g.hold("a running candidate moves there", False)
    life.reconcile()
    g.hold("... and has been reconciled", False)
    life.upsert_pods([r("1jy-p")], ["1jy-p"], ns=[SPARE])   # beyond ns_rows_hi and beyond what the program was compiled for
    g.hold("a pod arrives in a namespace row nobody has named yet", True)
    life.upsert_namespaces([SPARE], ["ns1"])
    g.hold("... and its Namespace object afterwards", True)


def life_namespace_events_among_the_others(life):
    t = {name: i for i, name in enumerate(life.pl.initial)}
    r = life.row
    start(life)
    g = _Gaps(life)
    life.reconcile()
    life.upsert_namespaces([2], ["ns2@prod"])               # right after reconcile(apply): the device's status is newer
    g.hold("a namespace event right after reconcile(apply)", True)
    life.reconcile()
    life.admit_commit([r("0dx-p"), r("1wx-p"), r("none"), r("1jy-p"), r("two")])
    life.admit_gangs_commit(life.q)
    life.upsert_namespaces([2], ["ns2"])                    # the reserved rows the device advanced go to the host and back
    g.hold("a namespace event behind admit(commit=True) and admit_gangs(commit=True)", True)
    life.upsert_namespaces([1], ["ns1@dev"])
    life.upsert_pods([r("1jx-r")], ["1jy-r"])
    g.hold("a namespace event, then a pod event of that namespace", True)
    life.upsert_pods([r("1jx-r")], ["1jx-r"])
    life.upsert_namespaces([1], ["ns1"])
    g.hold("a pod event, then a namespace event of its namespace", True)
    life.upsert_namespaces([0], ["ns0@dev"])
    life.upsert_throttles([t["ns1/t-job"]], ["ns1/t-job@tight"])
    g.hold("a namespace event, then a threshold-only throttle event", True)
    life.reconcile()
    g.hold("... and a reconcile behind them", False)


LIVES = {"pod_events": life_pod_events, "threshold_and_override_events": life_threshold_and_override_events,
         "selector_and_row_events": life_selector_and_row_events, "reservations_survive": life_reservations_survive,
         "negative_came_and_went": life_negative_came_and_went, "rows_appended": life_rows_appended,
         "namespace_labels": life_namespace_labels,
         "namespace_deleted_and_back": life_namespace_deleted_and_back,
         "namespace_arrives_after_its_pods": life_namespace_arrives_after_its_pods,
         "namespace_events_among_the_others": life_namespace_events_among_the_others}
# the lives of a cluster with twenty resource names: two pages, every event reaches both
WIDE_LIVES = {"two_pages": life_two_pages, "page_one_decides": life_page_one_decides,
              "negative_on_page_one": life_negative_on_page_one, "namespace_labels_wide": life_namespace_labels,
              "namespace_deleted_and_back_wide": life_namespace_deleted_and_back}


# ---- refused batches -------------------------------------------------------------------------------------------------------
REFUSALS = ("row-outside-capacity", "namespace-id-outside-capacity", "more-labels-than-kept", "request-beyond-2^60")


def refused_pod_batch(pl, case, page=0):
    """(batch, rows, expected code): entry 0 a pod with a NEGATIVE request that is larger than any the engine holds and has new
    odd low bits, entry 1 the pod the engine refuses the batch for."""
    base = pl.snaps[page]
    b = _permute_pods(base, [pl.pod["neg"], pl.pod["0jx-p"]])
    b.ctr_req[0, pl.dim("cpu")[1]] = -((1 << 40) + 12345)
    rows = np.array([P_CAP - 2, P_CAP - 1], np.int64)
    code = -2
    if case == "row-outside-capacity":
        rows[1] = P_CAP
    elif case == "namespace-id-outside-capacity":
        b.pod_ns[1] = 1000
    elif case == "more-labels-than-kept":
        k = base.L + 1
        lo = int(b.pod_label_off[1])
        b.pod_label_key = np.concatenate([b.pod_label_key[:lo], np.arange(k, dtype=np.uint32)])
        b.pod_label_pair = np.concatenate([b.pod_label_pair[:lo], np.arange(k, dtype=np.uint32)])
        b.pod_label_off[2] = lo + k
    elif case == "request-beyond-2^60":
        b.ctr_req[1, pl.dim("cpu")[1]] = 1 << 61
        code = -4
    else:
        raise KeyError(case)
    return b, rows, code
