"""GPU: fair shares between flows for the banded and costed pickers (SEMANTICS.md §3g; include/eppk.h eppk_fair_resolve_device /
eppk_pick_fair) against the numpy restatement (tests/fair_ref.py), exactly: picks, ranks, loads, scores as bit patterns, and the sticky
launch status.

The resolve alone on the generator's cases (tests/fair_cases.py) under three geometries; device against device (one flow against the
costed resolve, no costs against the banded resolve and against costs of one); the same inputs under the three geometries; many chunks
(the offsets scan's segments and trips); a single chunk through the permutation route; fairness read from the device's own answer; the
picker end to end against the oracle's lists fed through the restatement; a device group; argument checks; one context through
interleaved resolves.

The module sets the library switches itself (monkeypatch) before it creates a context."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# how the resolve is cut up: chunk size (EPPK_BOUND_CHUNK) and the width of the grid-stride loops (EPPK_MAX_CU); as tests/test_gpu_costed.py
GEOMETRIES = {"chunk64": {"EPPK_BOUND_CHUNK": "64"}, "default": {}, "chunk64-cu1": {"EPPK_BOUND_CHUNK": "64", "EPPK_MAX_CU": "1"}}
QUEUE = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("picks", "scores", "ranks", "loads")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fc():
    return _load("fair_cases")


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


def _resolve(pkg, pk, c, via="fair"):
    """One case through eppk_fair_resolve_device -- or, with via "costed" / "banded", its lists, costs, bands, caps and loads through
    eppk_costed_resolve_device / eppk_banded_resolve_device: (pick, score | None, rank | None, load_out | None, launch-status flags)."""
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
    d_load = None if c["load"] is None else _dev(torch, c["load"])
    d_pick = torch.full((max(R, 1),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_score = None if c["no_score"] else torch.full((max(R, 1),), 7.25, dtype=torch.float64, device=dev)
    d_rank = None if c["no_rank"] else torch.full((max(R, 1),), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None                  # noqa: E731
    lists = d_lists.data_ptr() if R else None
    if via == "banded":
        pk.bounded_resolve_banded_device(lists, ptr(d_ls), R, k, ptr(d_band), c["bands"], ptr(d_cap), c["cap_all"], ptr(d_load), d_pick.data_ptr(),
                                         ptr(d_score), ptr(d_rank))
    elif via == "costed":
        pk.bounded_resolve_costed_device(lists, ptr(d_ls), R, k, ptr(d_cost), 0, ptr(d_band), c["bands"], ptr(d_cap), c["cap_all"], ptr(d_load),
                                         d_pick.data_ptr(), ptr(d_score), ptr(d_rank))
    else:
        pk.bounded_resolve_fair_device(lists, ptr(d_ls), R, k, ptr(d_flow), c["n_flows"], ptr(d_cost), 0, ptr(d_band), c["bands"], ptr(d_cap),
                                       c["cap_all"], ptr(d_load), d_pick.data_ptr(), ptr(d_score), ptr(d_rank))
    flags = pk.launch_status()                                               # (synchronises)
    out = lambda t, dt: None if t is None else t.cpu().numpy()[:R].view(dt)  # noqa: E731
    return (out(d_pick, np.int32), out(d_score, np.float64), out(d_rank, np.uint8),
            None if d_load is None else d_load.cpu().numpy().view(np.uint32), flags)


def _diff(fc, c, got, want):
    """What differs between the device's answer and the restatement's, as text ('' = nothing)."""
    pick, score, rank, load, flags = got
    wp, ws, wr, wl, wflags = want
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
    if flags != wflags:
        msgs.append(f"launch status {flags}, want {wflags}")
    return f"{fc.info(c)}: " + "; ".join(msgs) if msgs else ""


def _same_bytes(a, b, what):
    for x, y, name in zip(a[:4], b[:4], NAMES):
        assert (x is None and y is None) or np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: {name}"
    assert a[4] == b[4], f"{what}: launch status"


@pytest.fixture(scope="module")
def wanted(fc):
    """The generator's cases and the restatement's answers per chunk size: computed once, shared, left unchanged."""
    memo = {}

    def get(chunk):
        if chunk not in memo:
            cases = sorted(fc.make_cases(chunk), key=lambda c: c["n_pods"])  # (one publish per pod count)
            memo[chunk] = (cases, [fc.want(c) for c in cases])
        return memo[chunk]

    return get


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_the_resolve_equals_the_restatement_on_the_generator_cases(pkg, fc, wanted, monkeypatch, geometry):
    _setenv(monkeypatch, GEOMETRIES[geometry])
    with _bare_picker(pkg, geometry) as pk:
        chunk = pk.bounded_geometry()[0]
        cases, wants = wanted(chunk)
        assert {0, 1, 63, 64, 65, chunk, chunk + 1} <= {c["lists"].shape[0] for c in cases}
        failed = [d for d in (_diff(fc, c, _resolve(pkg, pk, c), w) for c, w in zip(cases, wants)) if d]
        assert not failed, f"{len(failed)} of {len(cases)} cases: " + " | ".join(failed[:6])


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_one_flow_is_the_costed_resolve_and_no_cost_is_the_banded_resolve(pkg, fc, wanted, monkeypatch, geometry):
    """Identities 1 and 2 of §3g, device against device, byte for byte: n_flows = 1 and a NULL d_flow against
    eppk_costed_resolve_device; a NULL d_cost against eppk_banded_resolve_device and against a cost array of ones."""
    _setenv(monkeypatch, GEOMETRIES[geometry])
    with _bare_picker(pkg, geometry) as pk:
        chunk = pk.bounded_geometry()[0]
        cases = wanted(chunk)[0]
        costed, counted = [c for c in cases if c["cost"] is not None][::2], [c for c in cases if c["cost"] is None]
        assert any(c["lists"].shape[0] > chunk for c in costed) and any(0 < c["lists"].shape[0] <= chunk for c in costed)
        assert any(c["lists"].shape[0] > chunk for c in counted) and any(0 < c["lists"].shape[0] <= chunk for c in counted)
        for c in costed:
            R = c["lists"].shape[0]
            want = _resolve(pkg, pk, c, via="costed")
            _same_bytes(_resolve(pkg, pk, dict(c, flow=None, n_flows=1)), want, fc.info(c) + " (no flow array, one flow)")
            _same_bytes(_resolve(pkg, pk, dict(c, flow=None, n_flows=9)), want, fc.info(c) + " (no flow array, nine flows)")
            _same_bytes(_resolve(pkg, pk, dict(c, flow=np.zeros(R, dtype=np.uint16), n_flows=1)), want, fc.info(c) + " (every row in flow 0 of one)")
        for c in counted:
            R = c["lists"].shape[0]
            got = _resolve(pkg, pk, c)
            _same_bytes(got, _resolve(pkg, pk, dict(c, cost=np.ones(R, dtype=np.uint32))), fc.info(c) + " (costs of one)")
            _same_bytes(_resolve(pkg, pk, dict(c, flow=None, n_flows=1)), _resolve(pkg, pk, c, via="banded"), fc.info(c) + " (banded)")


def _contended(fc, n, seed, n_flows, nb, cost=True, P=11):
    rng = np.random.default_rng(fc.SEED0 + seed)
    lists = rng.integers(0, P, size=(n, 4)).astype(np.int32)
    lists[rng.random((n, 4)) < 0.35] = 3 % P
    lists[rng.random((n, 4)) < 0.1] = fc.NO
    costs = fc._costs(rng, n, 512) if cost else None
    total = int(costs.sum()) if cost else n
    caps = rng.integers(2, max(6, total // 2 // P), size=P).astype(np.uint32)
    return dict(name=f"contended-{n}", lists=lists, scores=rng.standard_normal((n, 4)), n_pods=P, flow=fc.heavy_flows(rng, n, n_flows), n_flows=n_flows,
                cost=costs, per_entry=False, bands=fc._table(rng, nb, 2), band=rng.integers(0, nb, size=n).astype(np.uint8), cap=caps, cap_all=0,
                load=rng.integers(0, 3, size=P).astype(np.uint32), no_score=False, no_rank=False)


def test_the_output_does_not_depend_on_chunk_size_or_grid(pkg, fc, monkeypatch):
    """The same inputs under EPPK_BOUND_CHUNK=64, the default chunk and EPPK_MAX_CU=1: identical bytes, and those of the restatement."""
    inputs = [_contended(fc, n, i, n_flows, nb, cost=bool(i % 2)) for i, (n, n_flows, nb) in
              enumerate(((63, 3, 1), (65, 64, 3), (511, 17, 8), (513, 1024, 3), (1543, 5, 3), (1100, 1024, 8)))]
    results = {}
    for geometry, env in GEOMETRIES.items():
        _setenv(monkeypatch, env)
        with _bare_picker(pkg, geometry) as pk:
            results[geometry] = [_resolve(pkg, pk, c) for c in inputs]
    for geometry, res in results.items():
        for c, a, b in zip(inputs, results["chunk64"], res):
            _same_bytes(a, b, f"{geometry} against chunk64, {fc.info(c)}")
    for c, got in zip(inputs, results["chunk64"]):
        want = fc.want(c)
        assert (want[2] & fc.ref.RANK_OVERFLOW).any() and (want[2] < 4).any(), "the caps bind"
        assert not _diff(fc, c, got, want)


def _many_chunks(fc, n_chunks):
    """n_chunks chunks of 64 rows, 1 024 flows in 8 bands; flow 5 of band 0 has a row in every chunk, at a lane that moves."""
    c = _contended(fc, 64 * n_chunks, n_chunks, 1024, 8, cost=bool(n_chunks % 2 == 1 and n_chunks != 257), P=7)
    at = np.arange(n_chunks) * 64 + (np.arange(n_chunks) * 5) % 64
    c["flow"][at], c["band"][at] = 5, 0
    c["name"] = f"{n_chunks}-chunks"
    return c


@pytest.mark.parametrize("n_chunks", [17, 33, 129, 257])
def test_the_chunk_axis_past_the_scan_segments(pkg, fc, monkeypatch, n_chunks):
    """17, 33, 129 and 257 chunks: past one chunk per segment of the offsets scan, past its eight-chunk trips, and past 16 of them
    (a scan over chunks is tested where its segments and trips end)."""
    _setenv(monkeypatch, GEOMETRIES["chunk64"])
    c = _many_chunks(fc, n_chunks)
    with _bare_picker(pkg, "chunk64") as pk:
        got = _resolve(pkg, pk, c)
    assert not _diff(fc, c, got, fc.want(c))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_the_permutation_route_with_one_chunk(pkg, fc, monkeypatch, n):
    """A batch of at most one chunk of 512 rows: the round kernels over a permutation with a single chunk (the costed and banded resolves
    take their one-launch kernels there)."""
    _setenv(monkeypatch, GEOMETRIES["default"])
    with _bare_picker(pkg, "default") as pk:
        assert pk.bounded_geometry()[0] == 512
        for cost in (True, False):
            c = _contended(fc, n, n + cost, 6, 3, cost=cost, P=3 if n > 1 else 1)
            assert not _diff(fc, c, _resolve(pkg, pk, c), fc.want(c))


def test_fairness_read_from_the_answer(pkg, fc, monkeypatch):
    """One pod, k = 1, SHED, cost 1, one band.  From the device's picks alone: the pod is filled; the slots of any two flows that still
    had a request refused differ by at most 1; a flow with fewer requests than the water level gets all of them.  In batch order the
    first flow takes everything."""
    _setenv(monkeypatch, GEOMETRIES["default"])
    rng = np.random.default_rng(fc.SEED0)
    n, n_flows, cap = 3000, 40, 400
    flow = np.sort(fc.heavy_flows(rng, n, n_flows))                          # tenant by tenant: the worst batch order
    c = dict(name="fairness", lists=np.zeros((n, 1), dtype=np.int32), scores=None, n_pods=1, flow=flow, n_flows=n_flows, cost=None, per_entry=False,
             bands=[(fc.SHED, 0)], band=None, cap=None, cap_all=cap, load=np.zeros(1, dtype=np.uint32), no_score=False, no_rank=False)
    with _bare_picker(pkg, "default") as pk:
        pick, _, rank, load, flags = _resolve(pkg, pk, c)
        in_batch_order = _resolve(pkg, pk, c, via="banded")[0]
    assert flags == 0 and load[0] == cap and np.count_nonzero(pick == 0) == cap
    cnt = np.bincount(flow, minlength=n_flows)
    slots = np.bincount(flow[pick == 0], minlength=n_flows)
    refused = cnt > slots
    assert refused.sum() >= 2 and (~refused & (cnt > 0)).sum() >= 2, "flows on both sides of the water level"
    level = slots[refused].min()
    assert slots[refused].max() - level <= 1
    assert np.all(slots[cnt < level] == cnt[cnt < level]) and np.all(cnt[~refused] <= level + 1)
    assert np.array_equal(np.nonzero(in_batch_order == 0)[0], np.arange(cap)) and np.unique(flow[:cap]).size < n_flows // 4
    assert not _diff(fc, c, (pick, None, rank, load, flags), fc.want(c))


# ---- end to end ------------------------------------------------------------------------------------------------------------

R_E2E, P_E2E = 256, 64


@pytest.fixture(scope="module")
def e2e(pkg, orc):
    """256 requests x 64 pods under QUEUE + KV, band bytes, flows, costs, and the oracle's lists."""
    wl = pkg.workload.make_workload(1, R=R_E2E, P=P_E2E)
    rng = np.random.default_rng(0xFA1E)
    lists = {}

    def topk(k):
        if k not in lists:
            lists[k] = orc.pick_topk_batch(wl.chain, wl.pods, None, wl.reqs, wl.B, k, threads=8)
        return lists[k]

    return dict(wl=wl, band=rng.choice(3, size=R_E2E, p=[0.2, 0.5, 0.3]).astype(np.uint8), flow=np.sort(_load("fair_cases").heavy_flows(rng, R_E2E, 9)),
                cost=np.clip(np.floor((rng.pareto(1.1, size=R_E2E) + 1.0) * 2.0), 1, 64).astype(np.uint32), topk=topk)


def _picker(pkg, wl):
    pk = pkg.BatchedPicker(wl.chain, max_pods=P_E2E, max_blocks=wl.B, max_batch=R_E2E, index_slots=wl.index_slots)
    pk.publish(wl.pods)
    return pk


SETTINGS = ((1, 2, [(0, 0), (0, 0), (0, 0)], False, True), (4, 6, [(1, 0), (0, 1), (0, 2)], True, True), (4, 2, [(0, 0), (1, 1), (0, 1)], True, False))


@pytest.mark.parametrize("chunking", ["chunk64", "default"])
def test_pick_fair_equals_the_oracle_lists_through_the_restatement(pkg, fc, e2e, monkeypatch, chunking):
    import torch
    _setenv(monkeypatch, GEOMETRIES[chunking])
    wl, band, flow = e2e["wl"], e2e["band"], e2e["flow"]
    dev = torch.device("cuda", 0)
    load0 = np.random.default_rng(7).integers(0, 2, size=P_E2E).astype(np.uint32)
    with _picker(pkg, wl) as pk:
        d_reqs, d_band, d_flow, d_costs = _dev(torch, wl.reqs), _dev(torch, band), _dev(torch, flow), _dev(torch, e2e["cost"])
        for k, cap_all, bands, with_load, with_cost in SETTINGS:
            cost, load = e2e["cost"] if with_cost else None, load0 if with_load else None
            lp, ls = e2e["topk"](k)
            want = fc.ref.resolve(lp, ls, P_E2E, flow, 9, cost, bands, band, None, cap_all * (8 if with_cost else 1), load)
            unfair = fc.ref.resolve(lp, ls, P_E2E, None, 1, cost, bands, band, None, cap_all * (8 if with_cost else 1), load)
            assert want[4] == 0 and (want[2] > 7).any() and not np.array_equal(want[0], unfair[0]), "the caps bind, and the order decides"
            cap = cap_all * (8 if with_cost else 1)
            got = pk.pick_bounded_fair(wl.reqs, k, flow, 9, cost, cap, bands, band, load)
            what = f"{chunking} k {k} bands {bands} cost {with_cost}"
            for g, w, name in zip(got[:3], want[:3], NAMES):
                assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)), f"pick_bounded_fair {what}: {name}"
            assert (got[3] is None) == (load is None) and (load is None or np.array_equal(got[3], want[3])), what
            d_load = _dev(torch, load) if load is not None else None
            d_pick = torch.empty(R_E2E, dtype=torch.int32, device=dev)
            d_score = torch.empty(R_E2E, dtype=torch.float64, device=dev)
            d_rank = torch.empty(R_E2E, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            pk.pick_bounded_fair_device(d_reqs.data_ptr(), R_E2E, None, k, d_flow.data_ptr(), 9, d_costs.data_ptr() if with_cost else None, d_band.data_ptr(),
                                        bands, None, cap, d_load.data_ptr() if load is not None else None, d_pick.data_ptr(), d_score.data_ptr(),
                                        d_rank.data_ptr())
            assert pk.launch_status() == 0
            for g, w, name in zip((d_pick, d_score, d_rank), want[:3], NAMES):
                assert np.array_equal(g.cpu().numpy().view(np.uint8), np.asarray(w).view(np.uint8)), f"pick_bounded_fair_device {what}: {name}"
            if load is not None:
                assert np.array_equal(d_load.cpu().numpy().view(np.uint32), want[3]), what


def test_a_group_of_two_equals_the_single_context(pkg, fc, e2e, monkeypatch):
    _setenv(monkeypatch, GEOMETRIES["chunk64"])
    wl, band, flow, cost = e2e["wl"], e2e["band"], e2e["flow"], e2e["cost"]
    load0 = np.random.default_rng(3).integers(0, 2, size=P_E2E).astype(np.uint32)
    settings = ((4, 9, cost, 40, [(1, 0), (0, 8), (1, 16)], band, load0), (2, 9, None, 3, [(0, 0), (1, 1)], band % 2, None), (1, 1, cost, 30, [(0, 0)], None, load0))
    with _picker(pkg, wl) as pk:
        single = [pk.pick_bounded_fair(wl.reqs, k, flow % nf, nf, c, cap, bands, b, load) for k, nf, c, cap, bands, b, load in settings]
    with pkg.DeviceGroup(wl.chain, [0] * 2, max_pods=P_E2E, max_blocks=wl.B, max_batch=R_E2E, index_slots=wl.index_slots, min_shard=1) as g:
        g.publish(wl.pods)
        for (k, nf, c, cap, bands, b, load), want in zip(settings, single):
            got = g.pick_bounded_fair(wl.reqs, k, flow % nf, nf, c, cap, bands, b, load)
            for x, y, name in zip(got[:3], want[:3], NAMES):
                assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), f"2 members k {k} flows {nf}: {name}"
            assert (got[3] is None) == (load is None) and (load is None or np.array_equal(got[3], want[3]))
            assert (want[2] > 7).any()
        bad = flow.copy()
        bad[9], bad[3] = 9, 0xFFFF
        with pytest.raises(pkg.EppkError) as ei:
            g.pick_bounded_fair(wl.reqs, 4, bad, 9, cost, 6, [(0, 0)] * 3, band)
        assert ei.value.code == -1 and "row 3" in str(ei.value) and "flow 65535 of 9" in str(ei.value)
        assert g.pick_bounded_fair(wl.reqs[:0], 4, flow[:0], 9, None, 6)[0].size == 0


def test_argument_validation(pkg, fc, e2e, monkeypatch):
    _setenv(monkeypatch, {})
    import torch
    wl, band, flow, cost = e2e["wl"], e2e["band"][:8], e2e["flow"][:8] % 3, e2e["cost"][:8]
    lib = pkg.load_library()
    ARG, LIMIT, NO_SNAPSHOT = -1, -2, -4
    dev = torch.device("cuda", 0)
    d_lists = torch.zeros((8, 4), dtype=torch.int32, device=dev)
    d_pick = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_reqs, d_band, d_flow, d_cost = _dev(torch, wl.reqs[:8]), _dev(torch, band), _dev(torch, flow), _dev(torch, np.ones(8, dtype=np.uint32))
    torch.cuda.synchronize(dev)
    ok = [(0, 0), (1, 1), (0, 1)]
    with _picker(pkg, wl) as pk:
        def calls(k, bands, n_flows=3, flags=0, d_c=d_cost.data_ptr(), c=cost):
            return (("pick_fair", lambda: pk.pick_bounded_fair(wl.reqs[:8], k, flow, n_flows, c, 6, bands, band)),
                    ("pick_fair_device", lambda: pk.pick_bounded_fair_device(d_reqs.data_ptr(), 8, None, k, d_flow.data_ptr(), n_flows, d_c, d_band.data_ptr(),
                                                                             bands, None, 6, None, d_pick.data_ptr(), None, None)),
                    ("fair_resolve_device", lambda: pk.bounded_resolve_fair_device(d_lists.data_ptr(), None, 8, k, d_flow.data_ptr(), n_flows, d_c, flags,
                                                                                   d_band.data_ptr(), bands, None, 6, None, d_pick.data_ptr(), None, None)))

        for k, bands, n_flows, word in ((0, ok, 3, "k out of range"), (9, ok, 3, "k out of range"), (4, [], 3, "n_bands out of range"),
                                        (4, [(0, 0), (2, 0), (0, 0)], 3, "unknown policy 2 in band 1"), (4, [(0, 0), (0, 5), (1, 4)], 3, "reserve of band 2"),
                                        (4, ok, 0, "n_flows out of range"), (4, ok, 1025, "n_flows out of range")):
            for name, call in calls(k, bands, n_flows):
                with pytest.raises(pkg.EppkError) as ei:
                    call()
                assert ei.value.code == ARG and word in str(ei.value) and name in str(ei.value), (name, k, bands, n_flows, str(ei.value))
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
        # the largest n_flows, no cost, no flows: accepted
        for name, call in calls(4, ok, n_flows=1024, d_c=None, c=None):
            call()
        assert pk.launch_status() == 0
        d_pick.fill_(0x5A5A5A5A)
        torch.cuda.synchronize(dev)
        tab = pkg._lib.BandTable()
        tab.n_bands = 1
        args = lambda lists, table, pick: (pk._ctx, lists, None, 8, 4, None, 1, None, 0, None, table, None, 6, None, pick, None, None, None)  # noqa: E731
        assert lib.eppk_fair_resolve_device(*args(d_lists.data_ptr(), None, d_pick.data_ptr())) == ARG
        assert lib.eppk_fair_resolve_device(*args(None, C.byref(tab), d_pick.data_ptr())) == ARG
        assert lib.eppk_fair_resolve_device(*args(d_lists.data_ptr(), C.byref(tab), None)) == ARG
        assert lib.eppk_fair_resolve_device(None, *args(d_lists.data_ptr(), C.byref(tab), d_pick.data_ptr())[1:]) == ARG
        with pytest.raises(pkg.EppkError) as ei:
            pk.pick_bounded_fair(np.zeros((R_E2E + 1, pk.row_words), dtype=np.uint64), 4, None, 1, None, 6, ok)
        assert ei.value.code == LIMIT
        # a host form refuses the batch and names the lowest bad row: a flow >= n_flows, a band byte >= n_bands, a cost out of range
        out = np.full(8, 0x5A5A5A5A, dtype=np.int32)
        for at, value, words in ((6, 3, ("row 6", "flow 3 of 3")), (2, 0xFFFF, ("row 2", "flow 65535 of 3")), (0, 700, ("row 0", "flow 700 of 3"))):
            bad = flow.copy()
            bad[7], bad[at] = 3, value
            with pytest.raises(pkg.EppkError) as ei:
                pk.pick_bounded_fair(wl.reqs[:8], 4, bad, 3, cost, 6, ok, band)
            assert ei.value.code == ARG and all(w in str(ei.value) for w in words), str(ei.value)
            assert lib.eppk_pick_fair(pk._ctx, wl.reqs[:8].ctypes.data, 8, None, 4, bad.ctypes.data, 3, None, None, C.byref(tab), None, 6, None,
                                      out.ctypes.data, None, None) == ARG
        assert np.all(out == 0x5A5A5A5A), "a refused call writes nothing"
        bad_flow, bad_band, bad_cost = flow.copy(), band.copy(), cost.copy()
        bad_flow[5], bad_band[4], bad_cost[3] = 3, 3, 0
        with pytest.raises(pkg.EppkError) as ei:
            pk.pick_bounded_fair(wl.reqs[:8], 4, bad_flow, 3, bad_cost, 6, ok, bad_band)
        assert ei.value.code == ARG and "row 3" in str(ei.value) and "cost 0" in str(ei.value)
        torch.cuda.synchronize(dev)
        assert np.all(d_pick.cpu().numpy() == 0x5A5A5A5A), "a refused call writes nothing"
        # n_reqs = 0: nothing to do, nothing touched
        pk.bounded_resolve_fair_device(None, None, 0, 4, None, 3, None, 0, None, ok, None, 6, None, None, None, None)
        assert pk.pick_bounded_fair(wl.reqs[:0], 4, flow[:0], 3, None, 6, ok)[0].size == 0
    with pkg.BatchedPicker(wl.chain, max_pods=P_E2E, max_blocks=wl.B, max_batch=8) as pk:
        with pytest.raises(pkg.EppkError) as ei:
            pk.pick_bounded_fair(wl.reqs[:8], 4, flow, 3, cost, 6, ok, band)
        assert ei.value.code == NO_SNAPSHOT


def test_one_context_through_interleaved_resolves(pkg, fc, monkeypatch):
    """One context: fair (4 flows, 100 rows), costed (5 000 rows), fair (1 024 flows, 5 000 rows), banded (70 rows), fair (2 flows, 9 000
    rows), each held to its restatement.  The resolves share the permutation, the segment bounds and the histograms; the flow histogram
    is needed small, large, and small per chunk over many chunks."""
    _setenv(monkeypatch, GEOMETRIES["chunk64"])
    steps = (("fair", _contended(fc, 100, 1, 4, 3)), ("costed", _contended(fc, 5000, 2, 1, 8)), ("fair", _contended(fc, 5000, 3, 1024, 8)),
             ("banded", _contended(fc, 70, 4, 1, 3, cost=False)), ("fair", _contended(fc, 9000, 5, 2, 3)))
    cr = fc.ref.costed
    with _bare_picker(pkg, "chunk64") as pk:
        for via, c in steps:
            got = _resolve(pkg, pk, c, via=via)
            if via == "fair":
                want = fc.want(c)
            elif via == "costed":
                want = cr.resolve(c["lists"], c["scores"], c["n_pods"], c["cost"], c["bands"], c["band"], c["cap"], c["cap_all"], c["load"])
            else:
                want = cr.banded.resolve(c["lists"], c["scores"], c["n_pods"], c["bands"], c["band"], c["cap"], c["cap_all"], c["load"])
            assert (want[2] > 7).any() and (want[2] < 4).any(), "the caps bind"
            assert not _diff(fc, c, got, want), via


def test_the_scheduler_driver_on_the_device(pkg):
    """tests/cpp/test_fair_scheduler.cpp: a Bounded profile with n_flows through eppk::Scheduler, against the real library."""
    exe = _load("test_fair_scheduler_cpp").build_driver()
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120, env=dict(os.environ, EPPK_BOUND_CHUNK="64"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fair scheduler: ok" in out.stdout
