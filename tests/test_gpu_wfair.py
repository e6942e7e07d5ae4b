"""GPU: weighted fair shares between flows with turns carried across batches (SEMANTICS.md §3h; include/eppk.h eppk_wfair_resolve_device /
eppk_pick_wfair) against the numpy restatement (tests/wfair_ref.py), exactly: picks, ranks, loads, turns, scores as bit patterns, and the
sticky launch status.

The resolve alone on the generator's cases (tests/wfair_cases.py) under three geometries; device against device (NULL / NULL against the
fair resolve, ones and zeros against NULL / NULL, turns shifted by whole cycles against unshifted); the same inputs under the three
geometries; many chunks; the largest LDS request; one context through a carried session with the turns and the loads left on the device;
the worked examples read from the device's own answer; the picker end to end against the oracle's lists fed through the restatement; a
device group; argument checks; the scheduler driver.

The module sets the library switches itself (monkeypatch) before it creates a context."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# how the resolve is cut up: chunk size (EPPK_BOUND_CHUNK) and the width of the grid-stride loops (EPPK_MAX_CU); as tests/test_gpu_fair.py
GEOMETRIES = {"chunk64": {"EPPK_BOUND_CHUNK": "64"}, "default": {}, "chunk64-cu1": {"EPPK_BOUND_CHUNK": "64", "EPPK_MAX_CU": "1"}}
QUEUE = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("picks", "scores", "ranks", "loads")
TOP = 0xFFFFFFFF


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def wc():
    return _load("wfair_cases")


def _setenv(monkeypatch, env):
    for name in ("EPPK_BOUND_CHUNK", "EPPK_MAX_CU"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _bare_picker(pkg, geometry=None):
    """A context for the resolve alone: the lists come from the test, the snapshot only says how many pods there are."""
    pk = pkg.BatchedPicker([(QUEUE, 1)], max_pods=4096, max_blocks=0, max_batch=64)
    if geometry is not None:
        chunk, one_launch = pk.bounded_geometry()
        assert chunk == int(GEOMETRIES[geometry].get("EPPK_BOUND_CHUNK", chunk)) and chunk >= 64 and chunk & (chunk - 1) == 0
        assert one_launch == chunk
    return pk


def _dev(torch, a):
    """A numpy array on the device (unsigned words travel as the signed type of their width)."""
    a = np.ascontiguousarray(a)
    for u, s in ((np.uint16, np.int16), (np.uint32, np.int32), (np.uint64, np.int64)):
        if a.dtype == u:
            a = a.view(s)
    return torch.from_numpy(a.copy()).to(torch.device("cuda", 0))


def _resolve(pkg, pk, c, via="wfair", d_turns=None, d_load=None):
    """One case through eppk_wfair_resolve_device -- or, with via "fair" / "costed", its lists, flows, costs, bands, caps and loads
    through eppk_fair_resolve_device / eppk_costed_resolve_device: (pick, score | None, rank | None, load_out | None, launch-status
    flags, turns_out | None).  d_turns / d_load: tensors that stay on the device (a carried session) in place of the case's own."""
    import torch
    dev = torch.device("cuda", 0)
    R, k = c["lists"].shape
    if pk.n_pods != c["n_pods"]:
        torch.cuda.synchronize(dev)
        pk.publish(np.zeros(c["n_pods"], dtype=pkg.picker.POD_DTYPE))
    d_lists = _dev(torch, c["lists"])
    d_ls = None if c["scores"] is None else _dev(torch, c["scores"])
    d_band = None if c["band"] is None or R == 0 else _dev(torch, c["band"])
    d_flow = None if c["flow"] is None or R == 0 else _dev(torch, c["flow"])
    d_cost = None if c["cost"] is None else _dev(torch, c["cost"] if R else np.ones(1, dtype=np.uint32))
    d_cap = None if c["cap"] is None else _dev(torch, c["cap"])
    if d_load is None:
        d_load = None if c["load"] is None else _dev(torch, c["load"])
    d_weight = None if c.get("weight") is None else _dev(torch, c["weight"])
    if d_turns is None:
        d_turns = None if c.get("turns") is None else _dev(torch, c["turns"])
    d_pick = torch.full((max(R, 1),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_score = None if c["no_score"] else torch.full((max(R, 1),), 7.25, dtype=torch.float64, device=dev)
    d_rank = None if c["no_rank"] else torch.full((max(R, 1),), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None                  # noqa: E731
    lists = d_lists.data_ptr() if R else None
    if via == "costed":
        pk.bounded_resolve_costed_device(lists, ptr(d_ls), R, k, ptr(d_cost), 0, ptr(d_band), c["bands"], ptr(d_cap), c["cap_all"], ptr(d_load),
                                         d_pick.data_ptr(), ptr(d_score), ptr(d_rank))
    elif via == "fair":
        pk.bounded_resolve_fair_device(lists, ptr(d_ls), R, k, ptr(d_flow), c["n_flows"], ptr(d_cost), 0, ptr(d_band), c["bands"], ptr(d_cap),
                                       c["cap_all"], ptr(d_load), d_pick.data_ptr(), ptr(d_score), ptr(d_rank))
    else:
        pk.bounded_resolve_wfair_device(lists, ptr(d_ls), R, k, ptr(d_flow), c["n_flows"], ptr(d_weight), ptr(d_turns), ptr(d_cost), 0, ptr(d_band),
                                        c["bands"], ptr(d_cap), c["cap_all"], ptr(d_load), d_pick.data_ptr(), ptr(d_score), ptr(d_rank))
    flags = pk.launch_status()                                               # (synchronises)
    out = lambda t, dt: None if t is None else t.cpu().numpy()[:R].view(dt)  # noqa: E731
    turns_out = None
    if via == "wfair" and d_turns is not None:
        turns_out = d_turns.cpu().numpy().view(np.uint32).reshape(len(c["bands"]), c["n_flows"])
    return (out(d_pick, np.int32), out(d_score, np.float64), out(d_rank, np.uint8),
            None if d_load is None else d_load.cpu().numpy().view(np.uint32), flags, turns_out)


def _diff(wc, c, got, want):
    """What differs between the device's answer and the restatement's, as text ('' = nothing)."""
    pick, score, rank, load, flags, turns = got
    wp, ws, wr, wl, wflags, wt = want
    msgs = []
    if not np.array_equal(pick, wp):
        r = np.nonzero(pick != wp)[0]
        msgs.append(f"picks differ in {r.size} rows, first {r[:4]}: gpu {pick[r[:4]]} want {wp[r[:4]]}")
    if score is not None and not np.array_equal(score.view(np.uint64), ws.view(np.uint64)):
        msgs.append("scores differ (bitwise)")
    if rank is not None and not np.array_equal(rank, wr):
        r = np.nonzero(rank != wr)[0]
        msgs.append(f"ranks differ in {r.size} rows, first {r[:4]}: gpu {rank[r[:4]]} want {wr[r[:4]]}")
    if load is not None and not np.array_equal(load, wl):
        p = np.nonzero(load != wl)[0]
        msgs.append(f"loads differ on pods {p[:4]}: gpu {load[p[:4]]} want {wl[p[:4]]}")
    if (turns is None) != (wt is None) or (wt is not None and not np.array_equal(turns, wt)):
        g = None if turns is None or wt is None else np.argwhere(turns != wt)[:4].tolist()
        msgs.append(f"turns differ at (band, flow) {g}")
    if flags != wflags:
        msgs.append(f"launch status {flags}, want {wflags}")
    return f"{wc.info(c)}: " + "; ".join(msgs) if msgs else ""


def _same_bytes(a, b, what, turns=True):
    for x, y, name in zip(a[:4], b[:4], NAMES):
        assert (x is None and y is None) or np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: {name}"
    assert a[4] == b[4], f"{what}: launch status"
    if turns:
        assert (a[5] is None and b[5] is None) or np.array_equal(a[5], b[5]), f"{what}: turns"


@pytest.fixture(scope="module")
def wanted(wc):
    """The generator's cases and the restatement's answers per chunk size: computed once, shared, left unchanged."""
    memo = {}

    def get(chunk):
        if chunk not in memo:
            cases = sorted(wc.make_cases(chunk), key=lambda c: c["n_pods"])  # (one publish per pod count)
            memo[chunk] = (cases, [wc.want(c) for c in cases])
        return memo[chunk]

    return get


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_the_resolve_equals_the_restatement_on_the_generator_cases(pkg, wc, wanted, monkeypatch, geometry):
    _setenv(monkeypatch, GEOMETRIES[geometry])
    with _bare_picker(pkg, geometry) as pk:
        chunk = pk.bounded_geometry()[0]
        cases, wants = wanted(chunk)
        assert {0, 1, 63, 64, 65, chunk, chunk + 1} <= {c["lists"].shape[0] for c in cases}
        failed = [d for d in (_diff(wc, c, _resolve(pkg, pk, c), w) for c, w in zip(cases, wants)) if d]
        assert not failed, f"{len(failed)} of {len(cases)} cases: " + " | ".join(failed[:6])


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_the_equalities_device_against_device(pkg, wc, wanted, monkeypatch, geometry):
    """§3h's equalities, byte for byte: NULL / NULL against eppk_fair_resolve_device; ones and zeros against NULL / NULL; the turns of
    every band moved by m whole cycles against unmoved -- the same picks, scores, ranks and loads, the turns handed back moved alike."""
    _setenv(monkeypatch, GEOMETRIES[geometry])
    rng = np.random.default_rng(wc.SEED0 + 7)
    with _bare_picker(pkg, geometry) as pk:
        chunk = pk.bounded_geometry()[0]
        cases, wants = wanted(chunk)
        picked = cases[::3]
        assert any(c["lists"].shape[0] > chunk for c in picked) and any(0 < c["lists"].shape[0] <= chunk for c in picked)
        for c in picked:
            nb, nf = len(c["bands"]), c["n_flows"]
            plain = dict(c, weight=None, turns=None)
            null = _resolve(pkg, pk, plain)
            assert null[5] is None
            _same_bytes(null, _resolve(pkg, pk, plain, via="fair"), wc.info(c) + " (NULL / NULL against the fair resolve)")
            ones = _resolve(pkg, pk, dict(c, weight=np.ones(nf, dtype=np.uint16), turns=np.zeros((nb, nf), dtype=np.uint32)))
            _same_bytes(ones, null, wc.info(c) + " (ones and zeros against NULL / NULL)", turns=False)
        moved = 0
        for c, want in zip(cases, wants):
            if c["turns"] is None:
                continue
            nb, nf = len(c["bands"]), c["n_flows"]
            w, t = wc.ref.tables(nb, nf, c["weight"], c["turns"])
            m = np.minimum(rng.integers(1, 1000, size=nb), (TOP - want[5].astype(np.int64).max(axis=1)) // w.max())[:, None]
            if not m.any():
                continue
            base, shifted = _resolve(pkg, pk, c), _resolve(pkg, pk, dict(c, turns=(t + m * w).astype(np.uint32)))
            _same_bytes(shifted, base, wc.info(c) + " (turns moved by whole cycles)", turns=False)
            live = w >= 1
            assert np.array_equal(shifted[5].astype(np.int64)[:, live], (base[5].astype(np.int64) + m * w)[:, live]), wc.info(c)
            moved += 1
        assert moved >= 10


def _contended(wc, n, seed, n_flows, nb, cost=True, P=11, wtop=6, cycles=4):
    fc = wc.fc
    rng = np.random.default_rng(wc.SEED0 + seed)
    lists = rng.integers(0, P, size=(n, 4)).astype(np.int32)
    lists[rng.random((n, 4)) < 0.35] = 3 % P
    lists[rng.random((n, 4)) < 0.1] = wc.NO
    costs = fc._costs(rng, n, 512) if cost else None
    total = int(costs.sum()) if cost else n
    caps = rng.integers(2, max(6, total // 2 // P), size=P).astype(np.uint32)
    weight = rng.integers(1, wtop + 1, size=n_flows).astype(np.uint16)
    turns = (rng.random((nb, n_flows)) * cycles * weight).astype(np.uint32)
    return dict(name=f"contended-{n}", lists=lists, scores=rng.standard_normal((n, 4)), n_pods=P, flow=fc.heavy_flows(rng, n, n_flows), n_flows=n_flows,
                weight=weight, turns=turns, cost=costs, per_entry=False, bands=fc._table(rng, nb, 2), band=rng.integers(0, nb, size=n).astype(np.uint8),
                cap=caps, cap_all=0, load=rng.integers(0, 3, size=P).astype(np.uint32), no_score=False, no_rank=False)


def test_the_output_does_not_depend_on_chunk_size_or_grid(pkg, wc, monkeypatch):
    """The same inputs under EPPK_BOUND_CHUNK=64, the default chunk and EPPK_MAX_CU=1: identical bytes, and those of the restatement."""
    inputs = [_contended(wc, n, i, n_flows, nb, cost=bool(i % 2)) for i, (n, n_flows, nb) in
              enumerate(((63, 3, 1), (65, 64, 3), (511, 17, 8), (513, 1024, 3), (1543, 5, 3)))]
    results = {}
    for geometry, env in GEOMETRIES.items():
        _setenv(monkeypatch, env)
        with _bare_picker(pkg, geometry) as pk:
            results[geometry] = [_resolve(pkg, pk, c) for c in inputs]
    for geometry, res in results.items():
        for c, a, b in zip(inputs, results["chunk64"], res):
            _same_bytes(a, b, f"{geometry} against chunk64, {wc.info(c)}")
    for c, got in zip(inputs, results["chunk64"]):
        want = wc.want(c)
        assert (want[2] & wc.ref.RANK_OVERFLOW).any() and (want[2] < 4).any(), "the caps bind"
        assert not _diff(wc, c, got, want)


@pytest.mark.parametrize("n_chunks", [17, 33, 129])
def test_the_chunk_axis_past_the_scan_segments(pkg, wc, monkeypatch, n_chunks):
    """17, 33 and 129 chunks of 64 rows: past one chunk per segment of the offsets scan and past its eight-chunk trips.  Flow 5 of band 0
    has a row in every chunk, at a lane that moves, and weight 3: its cycles end inside chunks, between chunks and between trips."""
    _setenv(monkeypatch, GEOMETRIES["chunk64"])
    c = _contended(wc, 64 * n_chunks, n_chunks, 1024 if n_chunks != 33 else 40, 8 if n_chunks != 33 else 2, cost=bool(n_chunks % 2 == 1), P=7)
    at = np.arange(n_chunks) * 64 + (np.arange(n_chunks) * 5) % 64
    c["flow"][at], c["band"][at] = 5, 0
    c["weight"][5], c["turns"][0, 5] = 3, 2
    c["name"] = f"{n_chunks}-chunks"
    with _bare_picker(pkg, "chunk64") as pk:
        got = _resolve(pkg, pk, c)
    assert not _diff(wc, c, got, wc.want(c))


def test_the_largest_lds_request(pkg, wc, monkeypatch):
    """8 bands x 1 024 flows: 100 KiB of dynamic LDS, above the default limit; a few hundred rows, any weight, turns at the top of 32
    bits among them."""
    _setenv(monkeypatch, GEOMETRIES["default"])
    c = _contended(wc, 700, 99, 1024, 8, P=9, wtop=65535)
    c["bands"] = [(p, 0) for p, _ in c["bands"]]
    c["turns"][:, ::7] = TOP - 5
    with _bare_picker(pkg, "default") as pk:
        got = _resolve(pkg, pk, c)
        again = _resolve(pkg, pk, dict(c, n_flows=1000, weight=c["weight"][:1000], turns=c["turns"][:, :1000].copy(), flow=c["flow"] % 1000))
    assert not _diff(wc, c, got, wc.want(c))
    c2 = dict(c, n_flows=1000, weight=c["weight"][:1000], turns=c["turns"][:, :1000].copy(), flow=c["flow"] % 1000)
    assert not _diff(wc, c2, again, wc.want(c2))


def test_a_carried_session_on_one_context(pkg, wc, monkeypatch):
    """One context, d_turns and d_load left on the device from call to call: a dozen batches below and above one chunk (the larger
    ones grow the scratch), two flow counts (a turns table each), fair and costed resolves in between (they share the permutation, the
    keys and the histograms), a rebase between two batches.  Every step is held to the restatement fed with the step's own inputs: the
    turns and loads the step before left."""
    import torch
    _setenv(monkeypatch, GEOMETRIES["chunk64"])
    P, nb = 5, 2
    bands = [(wc.SHED, 0), (wc.SPILL, 1)]
    rng = np.random.default_rng(wc.SEED0 + 11)
    weight = {3: np.array([3, 1, 2], dtype=np.uint16), 40: rng.integers(1, 5, size=40).astype(np.uint16)}
    turns = {nf: np.zeros((nb, nf), dtype=np.uint32) for nf in weight}
    steps = [("wfair", 40, 3), ("wfair", 200, 3), ("fair", 90, 3), ("wfair", 63, 40), ("wfair", 700, 40), ("costed", 300, 1), ("wfair", 65, 3),
             ("rebase", 0, 3), ("wfair", 1500, 3), ("wfair", 30, 40), ("fair", 400, 40), ("wfair", 129, 3), ("rebase", 0, 40), ("wfair", 333, 40),
             ("wfair", 64, 3), ("wfair", 1, 40)]
    with _bare_picker(pkg, "chunk64") as pk:
        pk.publish(np.zeros(P, dtype=pkg.picker.POD_DTYPE))
        d_turns = {nf: _dev(torch, turns[nf]) for nf in weight}
        load = np.zeros(P, dtype=np.uint32)
        d_load = _dev(torch, load)
        moved, rebased, bound = 0, 0, 0
        for i, (via, n, nf) in enumerate(steps):
            if via == "rebase":
                now = d_turns[nf].cpu().numpy().view(np.uint32)
                assert np.array_equal(now, turns[nf])
                turns[nf] = pk.turns_rebase(now, weight[nf], 2)
                assert np.array_equal(turns[nf], wc.ref.rebase(now, weight[nf], 2))
                rebased += not np.array_equal(turns[nf], now)
                d_turns[nf].copy_(_dev(torch, turns[nf]))
                continue
            lists = rng.integers(0, P, size=(n, 2)).astype(np.int32)
            lists[rng.random((n, 2)) < 0.1] = wc.NO
            cost = wc.fc._costs(rng, n, 6) if i % 2 or via == "costed" else None
            total = int(cost.sum()) if cost is not None else n
            c = dict(name=f"step-{i}-{via}", lists=lists, scores=rng.standard_normal((n, 2)), n_pods=P, flow=wc.fc.heavy_flows(rng, n, nf), n_flows=nf,
                     weight=weight.get(nf), turns=turns.get(nf), cost=cost, per_entry=False, bands=bands, band=rng.integers(0, nb, size=n).astype(np.uint8),
                     cap=None, cap_all=int(load.max()) + max(2, total // (3 * P)), load=load, no_score=False, no_rank=False)
            if via == "wfair":
                want = wc.want(c)
                got = _resolve(pkg, pk, c, d_turns=d_turns[nf], d_load=d_load)
                assert not _diff(wc, c, got, want), f"step {i}"
                bound += bool((want[2] & wc.ref.RANK_OVERFLOW).any() and (want[2] < 2).any())
                moved += not np.array_equal(want[5], turns[nf])
                turns[nf] = want[5]
            elif via == "fair":
                want = wc.ref.fair.resolve(lists, c["scores"], P, c["flow"], nf, cost, bands, c["band"], None, c["cap_all"], c["load"])
                _same_bytes(_resolve(pkg, pk, c, via="fair", d_load=d_load), want + (None,), f"step {i}")
            else:
                want = wc.ref.costed.resolve(lists, c["scores"], P, cost, bands, c["band"], None, c["cap_all"], c["load"])
                _same_bytes(_resolve(pkg, pk, c, via="costed", d_load=d_load), want + (None,), f"step {i}")
            load = want[3]
        assert moved >= 9 and rebased >= 1 and bound >= 8, "the turns move, and the caps bind"
        for nf in weight:
            assert np.array_equal(d_turns[nf].cpu().numpy().view(np.uint32), turns[nf]), "a fair or costed call in between leaves the turns alone"


def test_the_worked_examples_from_the_device(pkg, wc, monkeypatch):
    """§3h: weights (3, 1, 1) over five slots place 3 / 1 / 1; one slot per batch with the turns carried goes to flow 0, 1, 2 in turn,
    and to flow 0 three times without them."""
    import torch
    _setenv(monkeypatch, GEOMETRIES["default"])
    lists, flow, weight, cap, rows = wc.shares_case()
    base = dict(name="example", scores=None, n_pods=1, cost=None, per_entry=False, bands=[(wc.SHED, 0)], band=None, cap=None, no_score=False, no_rank=False)
    with _bare_picker(pkg, "default") as pk:
        c = dict(base, lists=lists, flow=flow, n_flows=3, weight=weight, turns=None, cap_all=cap, load=np.zeros(1, dtype=np.uint32))
        pick = _resolve(pkg, pk, c)[0]
        assert list(np.nonzero(pick == 0)[0]) == rows
        assert [int(np.count_nonzero(pick[flow == f] == 0)) for f in range(3)] == [3, 1, 1]
        equal = _resolve(pkg, pk, dict(c, weight=None))[0]
        assert [int(np.count_nonzero(equal[flow == f] == 0)) for f in range(3)] == [2, 2, 1]
        one = dict(base, lists=np.zeros((3, 1), dtype=np.int32), flow=np.arange(3, dtype=np.uint16), n_flows=3, weight=None, cap_all=1,
                   load=np.zeros(1, dtype=np.uint32))
        d_turns = _dev(torch, np.zeros((1, 3), dtype=np.uint32))
        placed, stateless = [], []
        for _ in range(3):
            got = _resolve(pkg, pk, dict(one, turns=np.zeros((1, 3), dtype=np.uint32)), d_turns=d_turns)
            placed.append(int(np.nonzero(got[0] == 0)[0][0]))
            stateless.append(int(np.nonzero(_resolve(pkg, pk, dict(one, turns=None))[0] == 0)[0][0]))
        assert placed == [0, 1, 2] and stateless == [0, 0, 0] and got[5].tolist() == [[1, 1, 1]]


# ---- end to end ------------------------------------------------------------------------------------------------------------

R_E2E, P_E2E, NF_E2E = 256, 64, 9


@pytest.fixture(scope="module")
def e2e(pkg, orc):
    """256 requests x 64 pods under QUEUE + KV, band bytes, flows, weights, costs, and the oracle's lists."""
    wl = pkg.workload.make_workload(1, R=R_E2E, P=P_E2E)
    rng = np.random.default_rng(0x3FA1E)
    lists = {}

    def topk(k):
        if k not in lists:
            lists[k] = orc.pick_topk_batch(wl.chain, wl.pods, None, wl.reqs, wl.B, k, threads=8)
        return lists[k]

    return dict(wl=wl, band=rng.choice(3, size=R_E2E, p=[0.2, 0.5, 0.3]).astype(np.uint8), flow=np.sort(_load("fair_cases").heavy_flows(rng, R_E2E, NF_E2E)),
                cost=np.clip(np.floor((rng.pareto(1.1, size=R_E2E) + 1.0) * 2.0), 1, 64).astype(np.uint32),
                weight=rng.integers(1, 5, size=NF_E2E).astype(np.uint16), topk=topk)


def _picker(pkg, wl):
    pk = pkg.BatchedPicker(wl.chain, max_pods=P_E2E, max_blocks=wl.B, max_batch=R_E2E, index_slots=wl.index_slots)
    pk.publish(wl.pods)
    return pk


SETTINGS = ((1, 2, [(0, 0), (0, 0), (0, 0)], False, True), (4, 6, [(1, 0), (0, 1), (0, 2)], True, True), (4, 2, [(0, 0), (1, 1), (0, 1)], True, False))


@pytest.mark.parametrize("chunking", ["chunk64", "default"])
def test_pick_wfair_equals_the_oracle_lists_through_the_restatement(pkg, wc, e2e, monkeypatch, chunking):
    """eppk_pick_wfair and eppk_pick_wfair_device, two batches each with the turns of the first fed to the second."""
    import torch
    _setenv(monkeypatch, GEOMETRIES[chunking])
    wl, band, flow, weight = e2e["wl"], e2e["band"], e2e["flow"], e2e["weight"]
    dev = torch.device("cuda", 0)
    load0 = np.random.default_rng(7).integers(0, 2, size=P_E2E).astype(np.uint32)
    with _picker(pkg, wl) as pk:
        d_reqs, d_band, d_flow, d_costs, d_weight = _dev(torch, wl.reqs), _dev(torch, band), _dev(torch, flow), _dev(torch, e2e["cost"]), _dev(torch, weight)
        for k, cap_all, bands, with_load, with_cost in SETTINGS:
            cost, load = e2e["cost"] if with_cost else None, load0 if with_load else None
            cap = cap_all * (8 if with_cost else 1)
            lp, ls = e2e["topk"](k)
            turns = np.random.default_rng(k).integers(0, 6, size=(3, NF_E2E)).astype(np.uint32)
            d_turns = _dev(torch, turns)
            for batch in range(2):
                want = wc.ref.resolve(lp, ls, P_E2E, flow, NF_E2E, weight, turns, cost, bands, band, None, cap, load)
                equal = wc.ref.resolve(lp, ls, P_E2E, flow, NF_E2E, None, None, cost, bands, band, None, cap, load)
                assert want[4] == 0 and (want[2] > 7).any() and not np.array_equal(want[0], equal[0]), "the caps bind, and the weights decide"
                got = pk.pick_wfair(wl.reqs, k, flow, NF_E2E, weight, turns, cost, cap, bands, band, load)
                what = f"{chunking} k {k} bands {bands} cost {with_cost} batch {batch}"
                for g, w, name in zip(got[:3], want[:3], NAMES):
                    assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)), f"pick_wfair {what}: {name}"
                assert (got[3] is None) == (load is None) and (load is None or np.array_equal(got[3], want[3])), what
                assert np.array_equal(got[4], want[5]) and got[4] is not turns, what
                d_load = _dev(torch, load) if load is not None else None
                d_pick = torch.empty(R_E2E, dtype=torch.int32, device=dev)
                d_score = torch.empty(R_E2E, dtype=torch.float64, device=dev)
                d_rank = torch.empty(R_E2E, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize(dev)
                pk.pick_wfair_device(d_reqs.data_ptr(), R_E2E, None, k, d_flow.data_ptr(), NF_E2E, d_weight.data_ptr(), d_turns.data_ptr(),
                                     d_costs.data_ptr() if with_cost else None, d_band.data_ptr(), bands, None, cap,
                                     d_load.data_ptr() if load is not None else None, d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr())
                assert pk.launch_status() == 0
                for g, w, name in zip((d_pick, d_score, d_rank), want[:3], NAMES):
                    assert np.array_equal(g.cpu().numpy().view(np.uint8), np.asarray(w).view(np.uint8)), f"pick_wfair_device {what}: {name}"
                if load is not None:
                    assert np.array_equal(d_load.cpu().numpy().view(np.uint32), want[3]), what
                assert np.array_equal(d_turns.cpu().numpy().view(np.uint32), want[5]), what
                turns = want[5]
            no_turns = pk.pick_wfair(wl.reqs, k, flow, NF_E2E, weight, None, cost, cap, bands, band, load)
            assert no_turns[4] is None


def test_a_group_of_one_device_equals_the_single_context(pkg, wc, e2e, monkeypatch):
    _setenv(monkeypatch, GEOMETRIES["chunk64"])
    wl, band, flow, cost, weight = e2e["wl"], e2e["band"], e2e["flow"], e2e["cost"], e2e["weight"]
    load0 = np.random.default_rng(3).integers(0, 2, size=P_E2E).astype(np.uint32)
    t3 = np.random.default_rng(4).integers(0, 9, size=(3, NF_E2E)).astype(np.uint32)
    settings = ((4, NF_E2E, weight, t3, cost, 40, [(1, 0), (0, 8), (1, 16)], band, load0), (2, NF_E2E, weight, None, None, 3, [(0, 0), (1, 1)], band % 2, None),
                (1, 2, None, t3[:1, :2], cost, 30, [(0, 0)], None, load0))
    with _picker(pkg, wl) as pk:
        single = [pk.pick_wfair(wl.reqs, k, flow % nf, nf, w, t, c, cap, bands, b, load) for k, nf, w, t, c, cap, bands, b, load in settings]
    with pkg.DeviceGroup(wl.chain, [0], max_pods=P_E2E, max_blocks=wl.B, max_batch=R_E2E, index_slots=wl.index_slots, min_shard=1) as g:
        g.publish(wl.pods)
        for (k, nf, w, t, c, cap, bands, b, load), want in zip(settings, single):
            got = g.pick_wfair(wl.reqs, k, flow % nf, nf, w, t, c, cap, bands, b, load)
            for x, y, name in zip(got[:3], want[:3], NAMES):
                assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), f"group k {k} flows {nf}: {name}"
            assert (got[3] is None) == (load is None) and (load is None or np.array_equal(got[3], want[3]))
            assert (got[4] is None) == (t is None) and (t is None or (np.array_equal(got[4], want[4]) and not np.array_equal(got[4], t)))
            assert (want[2] > 7).any()
        zero = weight.copy()
        zero[4] = 0
        with pytest.raises(pkg.EppkError) as ei:
            g.pick_wfair(wl.reqs, 4, np.where(flow == 4, 3, flow), NF_E2E, zero, None, cost, 6, [(0, 0)] * 3, band)
        assert ei.value.code == -1 and "flow 4 has weight 0" in str(ei.value)
        assert g.pick_wfair(wl.reqs[:0], 4, flow[:0], NF_E2E, weight, t3, None, 6, [(0, 0)] * 3)[0].size == 0


def test_argument_validation(pkg, wc, e2e, monkeypatch):
    """Every refusal leaves the outputs and the turns as they were."""
    _setenv(monkeypatch, {})
    import torch
    wl, band, flow, cost = e2e["wl"], e2e["band"][:8], e2e["flow"][:8] % 3, e2e["cost"][:8]
    lib = pkg.load_library()
    ARG, LIMIT, NO_SNAPSHOT = -1, -2, -4
    dev = torch.device("cuda", 0)
    weight = np.array([2, 1, 3], dtype=np.uint16)
    turns0 = np.full((3, 3), 0x1234, dtype=np.uint32)
    d_lists = torch.zeros((8, 4), dtype=torch.int32, device=dev)
    d_pick = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_reqs, d_band, d_flow, d_cost = _dev(torch, wl.reqs[:8]), _dev(torch, band), _dev(torch, flow), _dev(torch, np.ones(8, dtype=np.uint32))
    d_weight, d_turns = _dev(torch, weight), _dev(torch, turns0)
    torch.cuda.synchronize(dev)
    ok = [(0, 0), (1, 1), (0, 1)]

    def untouched():
        torch.cuda.synchronize(dev)
        assert np.all(d_pick.cpu().numpy() == 0x5A5A5A5A) and np.array_equal(d_turns.cpu().numpy().view(np.uint32), turns0), "a refused call writes nothing"

    with _picker(pkg, wl) as pk:
        def calls(k, bands, n_flows=3, flags=0, d_c=d_cost.data_ptr(), c=cost):
            w = weight if n_flows == 3 else np.ones(max(n_flows, 1), dtype=np.uint16)[:n_flows]
            t = np.zeros((len(bands), n_flows), dtype=np.uint32)
            return (("pick_wfair", lambda: pk.pick_wfair(wl.reqs[:8], k, flow, n_flows, w, t, c, 6, bands, band)),
                    ("pick_wfair_device", lambda: pk.pick_wfair_device(d_reqs.data_ptr(), 8, None, k, d_flow.data_ptr(), n_flows, d_weight.data_ptr(),
                                                                       d_turns.data_ptr(), d_c, d_band.data_ptr(), bands, None, 6, None, d_pick.data_ptr(), None,
                                                                       None)),
                    ("wfair_resolve_device", lambda: pk.bounded_resolve_wfair_device(d_lists.data_ptr(), None, 8, k, d_flow.data_ptr(), n_flows,
                                                                                     d_weight.data_ptr(), d_turns.data_ptr(), d_c, flags, d_band.data_ptr(), bands,
                                                                                     None, 6, None, d_pick.data_ptr(), None, None)))

        for k, bands, n_flows, word in ((0, ok, 3, "k out of range"), (9, ok, 3, "k out of range"), (4, [], 3, "n_bands out of range"),
                                        (4, [(0, 0), (2, 0), (0, 0)], 3, "unknown policy 2 in band 1"), (4, [(0, 0), (0, 5), (1, 4)], 3, "reserve of band 2"),
                                        (4, ok, 0, "n_flows out of range"), (4, ok, 1025, "n_flows out of range")):
            for name, call in calls(k, bands, n_flows):
                with pytest.raises(pkg.EppkError) as ei:
                    call()
                assert ei.value.code == ARG and word in str(ei.value) and name in str(ei.value), (name, k, bands, n_flows, str(ei.value))
        untouched()
        # cost flags with a null cost; an unknown flag
        name, call = calls(4, ok, flags=1, d_c=None)[2]
        with pytest.raises(pkg.EppkError) as ei:
            call()
        assert ei.value.code == ARG and "null cost" in str(ei.value) and name in str(ei.value)
        with pytest.raises(pkg.EppkError) as ei:
            calls(4, ok, flags=2)[2][1]()
        assert ei.value.code == ARG and "cost flags 2" in str(ei.value)
        pk.set_assumed_load(2)
        for name, call in calls(4, ok):
            with pytest.raises(pkg.EppkError) as ei:
                call()
            assert ei.value.code == ARG and "assumed load" in str(ei.value), (name, str(ei.value))
        pk.set_assumed_load(0)
        untouched()
        tab = pkg._lib.BandTable()
        tab.n_bands = 1
        args = lambda lists, table, pick: (pk._ctx, lists, None, 8, 4, None, 1, None, d_turns.data_ptr(), None, 0, None, table, None, 6, None, pick, None,  # noqa: E731
                                           None, None)
        assert lib.eppk_wfair_resolve_device(*args(d_lists.data_ptr(), None, d_pick.data_ptr())) == ARG
        assert lib.eppk_wfair_resolve_device(*args(None, C.byref(tab), d_pick.data_ptr())) == ARG
        assert lib.eppk_wfair_resolve_device(*args(d_lists.data_ptr(), C.byref(tab), None)) == ARG
        assert lib.eppk_wfair_resolve_device(None, *args(d_lists.data_ptr(), C.byref(tab), d_pick.data_ptr())[1:]) == ARG
        untouched()
        with pytest.raises(pkg.EppkError) as ei:
            pk.pick_wfair(np.zeros((R_E2E + 1, pk.row_words), dtype=np.uint64), 4, None, 1, None, None, None, 6, ok)
        assert ei.value.code == LIMIT
        # a host form refuses the batch and names the lowest bad row -- a flow >= n_flows, a flow of weight 0 -- and any zero weight, by flow
        out, host_turns = np.full(8, 0x5A5A5A5A, dtype=np.int32), turns0.copy()
        tab.n_bands = 3
        for bad_w, bad_flow, words in (([2, 0, 3], np.array([0, 2, 1, 0, 1, 2, 0, 0]), ("row 2", "flow 1 of weight 0")),
                                       ([2, 0, 3], np.array([0, 2, 2, 0, 3, 2, 0, 0]), ("row 4", "flow 3 of 3")),
                                       ([2, 1, 0], np.array([0, 1, 1, 0, 1, 0, 0, 0]), ("flow 2 has weight 0",))):
            bw, bf = np.array(bad_w, dtype=np.uint16), bad_flow.astype(np.uint16)
            with pytest.raises(pkg.EppkError) as ei:
                pk.pick_wfair(wl.reqs[:8], 4, bf, 3, bw, host_turns, cost, 6, ok, band)
            assert ei.value.code == ARG and all(w in str(ei.value) for w in words), str(ei.value)
            assert lib.eppk_pick_wfair(pk._ctx, wl.reqs[:8].ctypes.data, 8, None, 4, bf.ctypes.data, 3, bw.ctypes.data, host_turns.ctypes.data, None, None,
                                       C.byref(tab), None, 6, None, out.ctypes.data, None, None) == ARG
        assert np.all(out == 0x5A5A5A5A) and np.array_equal(host_turns, turns0), "a refused call writes nothing"
        with pytest.raises(pkg.EppkError):
            pk.pick_wfair(wl.reqs[:8], 4, flow, 3, [1, 2, 70000], None, cost, 6, ok, band)
        untouched()
        # on the device forms a weight of 0 is no refusal: the flow's rows are answered as bad rows, the others as if they were not there
        d_zero = _dev(torch, np.array([2, 0, 3], dtype=np.uint16))
        mixed = np.array([0, 1, 2, 0, 1, 2, 0, 0], dtype=np.uint16)
        d_mixed = _dev(torch, mixed)
        d_t = _dev(torch, turns0)
        d_p, d_r = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=dev), torch.full((8,), 0x5A, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        pk.bounded_resolve_wfair_device(d_lists.data_ptr(), None, 8, 4, d_mixed.data_ptr(), 3, d_zero.data_ptr(), d_t.data_ptr(), None, 0, d_band.data_ptr(), ok,
                                        None, 60, None, d_p.data_ptr(), None, d_r.data_ptr())
        assert pk.launch_status() == 1
        p, r, t = d_p.cpu().numpy(), d_r.cpu().numpy(), d_t.cpu().numpy().view(np.uint32)
        assert np.all(p[mixed == 1] == -1) and np.all(r[mixed == 1] == 0x80) and np.all(p[mixed != 1] == 0) and np.array_equal(t[:, 1], turns0[:, 1])
        assert int(t.sum()) - int(turns0.sum()) == np.count_nonzero(mixed != 1)
        # n_reqs = 0: nothing to do, nothing touched
        pk.bounded_resolve_wfair_device(None, None, 0, 4, None, 3, d_weight.data_ptr(), d_turns.data_ptr(), None, 0, None, ok, None, 6, None, None, None, None)
        got = pk.pick_wfair(wl.reqs[:0], 4, flow[:0], 3, weight, turns0, None, 6, ok)
        assert got[0].size == 0 and np.array_equal(got[4], turns0)
        untouched()
    with pkg.BatchedPicker(wl.chain, max_pods=P_E2E, max_blocks=wl.B, max_batch=8) as pk:
        with pytest.raises(pkg.EppkError) as ei:
            pk.pick_wfair(wl.reqs[:8], 4, flow, 3, weight, turns0, cost, 6, ok, band)
        assert ei.value.code == NO_SNAPSHOT


def test_the_scheduler_driver_on_the_device(pkg):
    """tests/cpp/test_wfair_scheduler.cpp: a Bounded profile with flow_weights and a turn_window through eppk::Scheduler, against the
    real library."""
    exe = _load("test_wfair_scheduler_cpp").build_driver()
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120, env=dict(os.environ, EPPK_BOUND_CHUNK="64"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "wfair scheduler: ok" in out.stdout
