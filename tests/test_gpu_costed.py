"""GPU: cost-weighted caps for the bounded and banded pickers (SEMANTICS.md §3f; include/eppk.h eppk_costed_resolve_device /
eppk_pick_costed) against the numpy restatement (tests/costed_ref.py), exactly: picks, ranks, loads, scores as bit patterns, and the
sticky launch status.

The resolve alone on the generator's cases (tests/costed_cases.py), placed by the chunk size the context reports; every cost 1 against
eppk_banded_resolve_device; the same inputs under different chunk sizes and grid widths; per-entry costs; the picker end to end against
the oracle's lists fed through the restatement; argument checks; a device group; the C++ scheduler driver.

The module sets the library switches itself (monkeypatch) before it creates a context."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# how the resolve is cut up: chunk size (EPPK_BOUND_CHUNK) and the width of the grid-stride loops (EPPK_MAX_CU)
GEOMETRIES = {"chunk64": {"EPPK_BOUND_CHUNK": "64"}, "default": {}, "chunk64-cu1": {"EPPK_BOUND_CHUNK": "64", "EPPK_MAX_CU": "1"}}
MODES = {"default": {}, "quadmin4": {"EPPK_QUAD_MIN": "4"}}
QUEUE = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PER_ENTRY = 1


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def cs():
    return _load("costed_cases")


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
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).to(torch.device("cuda", 0))


def _resolve(pkg, pk, c, banded=False):
    """One case through eppk_costed_resolve_device -- or, with banded, its lists, bands, caps and loads through
    eppk_banded_resolve_device: (pick, score | None, rank | None, load_out | None, launch-status flags)."""
    import torch
    dev = torch.device("cuda", 0)
    R, k = c["lists"].shape
    if pk.n_pods != c["n_pods"]:
        torch.cuda.synchronize(dev)
        pk.publish(np.zeros(c["n_pods"], dtype=pkg.picker.POD_DTYPE))
    d_lists = _dev(torch, c["lists"])
    d_ls = None if c["scores"] is None else _dev(torch, c["scores"])
    d_band = None if c["band"] is None or R == 0 else _dev(torch, c["band"])
    d_cost = _dev(torch, c["cost"] if R else np.ones(1, dtype=np.uint32))
    d_cap = None if c["cap"] is None else _dev(torch, c["cap"])
    d_load = None if c["load"] is None else _dev(torch, c["load"])
    d_pick = torch.full((max(R, 1),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_score = None if c["no_score"] else torch.full((max(R, 1),), 7.25, dtype=torch.float64, device=dev)
    d_rank = None if c["no_rank"] else torch.full((max(R, 1),), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None                  # noqa: E731
    if banded:
        pk.bounded_resolve_banded_device(d_lists.data_ptr() if R else None, ptr(d_ls), R, k, ptr(d_band), c["bands"], ptr(d_cap), c["cap_all"], ptr(d_load),
                                         d_pick.data_ptr(), ptr(d_score), ptr(d_rank))
    else:
        pk.bounded_resolve_costed_device(d_lists.data_ptr() if R else None, ptr(d_ls), R, k, d_cost.data_ptr(), PER_ENTRY if c["per_entry"] else 0,
                                         ptr(d_band), c["bands"], ptr(d_cap), c["cap_all"], ptr(d_load), d_pick.data_ptr(), ptr(d_score), ptr(d_rank))
    flags = pk.launch_status()                                               # (synchronises)
    out = lambda t, dt: None if t is None else t.cpu().numpy()[:R].view(dt)  # noqa: E731
    return (out(d_pick, np.int32), out(d_score, np.float64), out(d_rank, np.uint8),
            None if d_load is None else d_load.cpu().numpy().view(np.uint32), flags)


def _diff(cs, c, got, want):
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
    return f"{cs.info(c)}: " + "; ".join(msgs) if msgs else ""


@pytest.fixture(scope="module")
def wanted(cs):
    """The generator's cases and the restatement's answers per chunk size: computed once, shared, left unchanged."""
    memo = {}

    def get(chunk):
        if chunk not in memo:
            cases = sorted(cs.make_cases(chunk), key=lambda c: c["n_pods"])  # (one publish per pod count)
            memo[chunk] = (cases, [cs.want(c) for c in cases])
        return memo[chunk]

    return get


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_the_resolve_equals_the_restatement_on_the_smallest_shapes_that_can_break_it(pkg, cs, wanted, monkeypatch, geometry):
    _setenv(monkeypatch, GEOMETRIES[geometry])
    with _bare_picker(pkg, geometry) as pk:
        chunk = pk.bounded_geometry()[0]
        cases, wants = wanted(chunk)
        assert not set(cs.REQUIRED) - set().union(*(c["tags"] for c in cases))
        sizes = {c["lists"].shape[0] for c in cases}
        assert {0, 1, 63, 64, 65, 127, 129, chunk - 1, chunk, chunk + 1, 2 * chunk + 3, 9 * chunk + 5} <= sizes and max(sizes) == 9 * chunk + 5
        assert {c["n_pods"] for c in cases} >= {1, 2, 64, 65, 4096} and {c["lists"].shape[1] for c in cases} >= {1, 2, 4, 8}
        failed = [d for d in (_diff(cs, c, _resolve(pkg, pk, c), w) for c, w in zip(cases, wants)) if d]
        assert not failed, f"{len(failed)} of {len(cases)} cases: " + " | ".join(failed[:6])


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_every_cost_one_equals_the_banded_resolve(pkg, cs, wanted, monkeypatch, geometry):
    """Every cost 1: the outputs of eppk_banded_resolve_device on the same inputs, byte for byte."""
    _setenv(monkeypatch, GEOMETRIES[geometry])
    with _bare_picker(pkg, geometry) as pk:
        chunk = pk.bounded_geometry()[0]
        cases = wanted(chunk)[0][::2]
        assert any(c["lists"].shape[0] > chunk for c in cases) and any(0 < c["lists"].shape[0] <= chunk for c in cases)
        for c in cases:
            u = cs.unit_cost(c)
            got, want = _resolve(pkg, pk, u), _resolve(pkg, pk, u, banded=True)
            for x, y, what in zip(got[:4], want[:4], ("picks", "scores", "ranks", "loads")):
                assert (x is None and y is None) or np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{cs.info(c)}: {what}"
            assert got[4] == want[4], f"{cs.info(c)}: launch status"


def _contended(cs, n, seed, per_entry=False):
    rng = np.random.default_rng(cs.SEED0 + seed)
    P, nb = 11, (1, 3, 8)[seed % 3]
    lists = rng.integers(0, P, size=(n, 4)).astype(np.int32)
    lists[rng.random((n, 4)) < 0.35] = 3
    lists[rng.random((n, 4)) < 0.1] = cs.NO
    cost = cs._costs(rng, (n, 4) if per_entry else n, 512)
    caps = rng.integers(8, max(40, int(cost.sum()) // (8 if per_entry else 2) // P), size=P).astype(np.uint32)
    return dict(name=f"contended-{n}", tags=set(), lists=lists, scores=rng.standard_normal((n, 4)), n_pods=P, cost=cost, per_entry=per_entry,
                bands=cs._table(rng, nb, 6), band=rng.integers(0, nb, size=n).astype(np.uint8), cap=caps, cap_all=0,
                load=rng.integers(0, 30, size=P).astype(np.uint32), no_score=False, no_rank=False)


def _across_geometries(pkg, cs, monkeypatch, per_entry):
    sizes = set()
    for env in GEOMETRIES.values():
        _setenv(monkeypatch, env)
        with _bare_picker(pkg) as pk:
            one = pk.bounded_geometry()[1]
        sizes |= {one - 1, one, one + 1, 3 * one + 7}
    inputs = [_contended(cs, n, i, per_entry) for i, n in enumerate(sorted(sizes))]
    results = {}
    for geometry, env in GEOMETRIES.items():
        _setenv(monkeypatch, env)
        with _bare_picker(pkg, geometry) as pk:
            results[geometry] = [_resolve(pkg, pk, c) for c in inputs]
    first = results["chunk64"]
    for geometry, res in results.items():
        for c, a, b in zip(inputs, first, res):
            for x, y, what in zip(a[:4], b[:4], ("picks", "scores", "ranks", "loads")):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{geometry} against chunk64, {cs.info(c)}: {what}"
    for c, got in zip(inputs, first):
        want = cs.want(c)
        assert (want[2] & cs.ref.RANK_OVERFLOW).any() and (want[2] < 4).any(), "the caps bind"
        assert not _diff(cs, c, got, want)


def test_the_output_does_not_depend_on_chunk_size_or_grid(pkg, cs, monkeypatch):
    """The same inputs under EPPK_BOUND_CHUNK=64, the default chunk and EPPK_MAX_CU=1: identical outputs -- on either side of each
    geometry's one-launch threshold, and over several chunks with a ragged end."""
    _across_geometries(pkg, cs, monkeypatch, per_entry=False)


def test_per_entry_costs(pkg, cs, wanted, monkeypatch):
    """EPPK_COST_PER_ENTRY: the generator's per-entry cases are part of the first test; here contended batches under every geometry, and
    a per-entry matrix with equal columns against the per-request form."""
    _across_geometries(pkg, cs, monkeypatch, per_entry=True)
    _setenv(monkeypatch, {})
    with _bare_picker(pkg, "default") as pk:
        chunk = pk.bounded_geometry()[0]
        for n in (100, 2 * chunk + 3):
            c = _contended(cs, n, n)
            wide = dict(c, cost=np.repeat(c["cost"][:, None], 4, axis=1), per_entry=True)
            a, b = _resolve(pkg, pk, c), _resolve(pkg, pk, wide)
            for x, y in zip(a[:4], b[:4]):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), cs.info(c)


# ---- end to end ------------------------------------------------------------------------------------------------------------

R_E2E, P_E2E = 256, 1000                                                     # (the batch tests/test_gpu_bounded.py takes end to end)
CHUNKINGS = {"chunk64": {"EPPK_BOUND_CHUNK": "64"}, "default": {}}


@pytest.fixture(scope="module")
def e2e(pkg, orc):
    """make_workload(3)-sized batch, its oracle index, a mask (one request without candidates), band bytes, costs, and the oracle's lists."""
    wl = pkg.workload.make_workload(3, R=R_E2E, P=P_E2E)
    oix = orc.OracleIndex()
    oix.insert(wl.index_hashes, wl.index_pods)
    rng = np.random.default_rng(0xE2E)
    J = (P_E2E + 63) // 64
    mask = rng.integers(0, 1 << 63, size=(R_E2E, J), dtype=np.uint64) | (rng.integers(0, 2, size=(R_E2E, J), dtype=np.uint64) << np.uint64(63))
    mask[:, J - 1] &= np.uint64((1 << (P_E2E % 64)) - 1)
    mask[5, :] = 0
    band = rng.choice(3, size=R_E2E, p=[0.1, 0.6, 0.3]).astype(np.uint8)
    cost = np.clip(np.floor((rng.pareto(1.1, size=R_E2E) + 1.0) * 2.0), 1, 64).astype(np.uint32)
    lists = {}

    def topk(k, masked):
        if (k, masked) not in lists:
            lists[(k, masked)] = orc.pick_topk_batch(wl.chain, wl.pods, oix, wl.reqs, wl.B, k, mask=mask if masked else None, threads=8)
        return lists[(k, masked)]

    return dict(wl=wl, mask=mask, band=band, cost=cost, topk=topk)


@pytest.fixture(params=list(CHUNKINGS))
def chunking(request, monkeypatch):
    _setenv(monkeypatch, CHUNKINGS[request.param])
    return request.param


def _picker(pkg, wl, chunking, max_batch=R_E2E):
    pk = pkg.BatchedPicker(wl.chain, max_pods=1024, max_blocks=wl.B, max_batch=max_batch, index_slots=wl.index_slots)
    chunk, one_launch = pk.bounded_geometry()
    if chunking == "chunk64":
        assert chunk == 64 and R_E2E > one_launch, "the batch spans several chunks"
    else:
        assert R_E2E <= one_launch, "the batch fits the one-launch kernel"
    pk.publish(wl.pods)
    pk.index_insert(wl.index_hashes, wl.index_pods)
    return pk


def _same(got, want, what):
    for g, w, name in zip(got, want, ("picks", "scores", "ranks", "loads")):
        assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)), f"{what}: {name}"


# (k, caps or one cap for all, cap_all, bands, with loads)
SETTINGS = ((1, None, 6, [(0, 0), (0, 0), (0, 0)], False), (4, None, 12, [(1, 0), (0, 4), (0, 8)], True),
            (4, "caps", 0, [(0, 0), (1, 3), (0, 3)], True), (8, None, 10, [(0, 0), (0, 0), (1, 6)], False))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_pick_bounded_costed_equals_the_oracle_lists_through_the_restatement(pkg, cs, e2e, monkeypatch, chunking, mode, masked):
    import torch
    for name, value in MODES[mode].items():
        monkeypatch.setenv(name, value)
    wl, mask, band, cost = e2e["wl"], e2e["mask"] if masked else None, e2e["band"], e2e["cost"]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    caps = rng.integers(0, 20, size=P_E2E).astype(np.uint32)
    load0 = rng.integers(0, 4, size=P_E2E).astype(np.uint32)
    with _picker(pkg, wl, chunking) as pk:
        d_reqs = _dev(torch, wl.reqs)
        d_mask = _dev(torch, mask) if masked else None
        d_band = _dev(torch, band)
        d_cost = _dev(torch, cost)
        for k, cap, cap_all, bands, with_load in SETTINGS:
            cap = caps if cap is not None else None
            load = load0 if with_load else None
            lp, ls = e2e["topk"](k, masked)
            want = cs.ref.resolve(lp, ls, P_E2E, cost, bands, band, cap, cap_all, load)
            counts = cs.ref.resolve(lp, ls, P_E2E, np.ones(R_E2E, dtype=np.uint32), bands, band, cap, cap_all, load)
            assert want[4] == 0 and (want[2] != 0).any() and not np.array_equal(want[0], counts[0]), "the caps bind, and the costs decide"
            got = pk.pick_bounded_costed(wl.reqs, k, cost, cap if cap is not None else cap_all, bands, band, load, mask)
            what = f"{mode} masked {masked} k {k} bands {bands}"
            _same(got[:3], want[:3], "pick_bounded_costed " + what)
            assert (got[3] is None) == (load is None) and (load is None or np.array_equal(got[3], want[3])), what
            if masked:
                assert got[0][5] == -1 and got[2][5] == cs.ref.RANK_NONE
            # the device form: nothing leaves the device
            d_cap = _dev(torch, cap) if cap is not None else None
            d_load = _dev(torch, load) if load is not None else None
            d_pick = torch.empty(R_E2E, dtype=torch.int32, device=dev)
            d_score = torch.empty(R_E2E, dtype=torch.float64, device=dev)
            d_rank = torch.empty(R_E2E, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            pk.pick_bounded_costed_device(d_reqs.data_ptr(), R_E2E, d_mask.data_ptr() if masked else None, k, d_cost.data_ptr(), d_band.data_ptr(), bands,
                                          d_cap.data_ptr() if cap is not None else None, cap_all, d_load.data_ptr() if load is not None else None,
                                          d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr())
            assert pk.launch_status() == 0
            _same((d_pick.cpu().numpy(), d_score.cpu().numpy(), d_rank.cpu().numpy()), want[:3], "pick_bounded_costed_device " + what)
            if load is not None:
                assert np.array_equal(d_load.cpu().numpy().view(np.uint32), want[3]), what


def test_a_group_of_three_equals_the_single_context(pkg, cs, e2e, chunking):
    wl, mask, band, cost = e2e["wl"], e2e["mask"], e2e["band"], e2e["cost"]
    rng = np.random.default_rng(3)
    caps = rng.integers(0, 16, size=P_E2E).astype(np.uint32)
    load0 = rng.integers(0, 4, size=P_E2E).astype(np.uint32)
    settings = ((4, 6, [(0, 0), (0, 0), (0, 0)], band, None, None), (4, caps, [(1, 0), (0, 2), (1, 5)], band, load0, mask),
                (8, 10, [(0, 0), (1, 4)], band % 2, load0, None), (1, caps, [(1, 0)], None, None, mask))
    with _picker(pkg, wl, chunking) as pk:
        single = [pk.pick_bounded_costed(wl.reqs, k, cost, cap, bands, b, load, m) for k, cap, bands, b, load, m in settings]
    with pkg.DeviceGroup(wl.chain, [0] * 3, max_pods=1024, max_blocks=wl.B, max_batch=R_E2E, index_slots=wl.index_slots, min_shard=1) as g:
        g.publish(wl.pods)
        g.index_insert(wl.index_hashes, wl.index_pods)
        for (k, cap, bands, b, load, m), want in zip(settings, single):
            got = g.pick_bounded_costed(wl.reqs, k, cost, cap, bands, b, load, m)
            _same(got[:3], want[:3], f"3 members k {k} bands {bands}")
            assert (got[3] is None) == (load is None) and (load is None or np.array_equal(got[3], want[3]))
            assert (want[2] != 0).any()
        bad = cost.copy()
        bad[9], bad[3] = 0, cs.MAX_COST + 1
        with pytest.raises(pkg.EppkError) as ei:
            g.pick_bounded_costed(wl.reqs, 4, bad, 6, [(0, 0)] * 3, band)
        assert ei.value.code == -1 and "row 3" in str(ei.value) and "cost" in str(ei.value)
        assert g.pick_bounded_costed(wl.reqs[:0], 4, cost[:0], 6)[0].size == 0


def test_argument_validation(pkg, cs, e2e, monkeypatch):
    _setenv(monkeypatch, {})
    import torch
    wl, band, cost = e2e["wl"], e2e["band"][:8], e2e["cost"][:8]
    lib = pkg.load_library()
    ARG, LIMIT, NO_SNAPSHOT = -1, -2, -4
    dev = torch.device("cuda", 0)
    d_lists = torch.zeros((8, 8), dtype=torch.int32, device=dev)
    d_pick = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_reqs = _dev(torch, wl.reqs[:8])
    d_band = _dev(torch, band)
    d_cost = _dev(torch, np.ones((8, 8), dtype=np.uint32))
    torch.cuda.synchronize(dev)
    ok = [(0, 0), (1, 1), (0, 1)]
    with _picker(pkg, wl, "default") as pk:
        def calls(k, bands):
            return (("pick_costed", lambda: pk.pick_bounded_costed(wl.reqs[:8], k, cost, 6, bands, band)),
                    ("pick_costed_device", lambda: pk.pick_bounded_costed_device(d_reqs.data_ptr(), 8, None, k, d_cost.data_ptr(), d_band.data_ptr(), bands, None,
                                                                                 6, None, d_pick.data_ptr(), None, None)),
                    ("costed_resolve_device", lambda: pk.bounded_resolve_costed_device(d_lists.data_ptr(), None, 8, k, d_cost.data_ptr(), 0, d_band.data_ptr(),
                                                                                       bands, None, 6, None, d_pick.data_ptr(), None, None)))

        for k, bands, word in ((0, ok, "k out of range"), (9, ok, "k out of range"), (4, [], "n_bands out of range"), (4, [(0, 0)] * 9, "n_bands out of range"),
                               (4, [(0, 0), (2, 0), (0, 0)], "unknown policy 2 in band 1"), (4, [(0, 0), (0, 5), (1, 4)], "reserve of band 2")):
            for name, call in calls(k, bands):
                with pytest.raises(pkg.EppkError) as ei:
                    call()
                assert ei.value.code == ARG and word in str(ei.value) and name in str(ei.value), (name, k, bands, str(ei.value))
        pk.set_assumed_load(2)
        for name, call in calls(4, ok):
            with pytest.raises(pkg.EppkError) as ei:
                call()
            assert ei.value.code == ARG and "assumed load" in str(ei.value), (name, str(ei.value))
        pk.set_assumed_load(0)
        tab = pkg._lib.BandTable()
        tab.n_bands = 1
        err = lambda: (lib.eppk_last_error(pk._ctx) or b"").decode()                                                             # noqa: E731
        args = lambda lists, cost_ptr, flags, table, pick: (pk._ctx, lists, None, 8, 4, cost_ptr, flags, None, table, None, 6, None, pick, None, None, None)  # noqa: E731
        assert lib.eppk_costed_resolve_device(*args(d_lists.data_ptr(), d_cost.data_ptr(), PER_ENTRY, C.byref(tab), d_pick.data_ptr())) == 0
        assert pk.launch_status() == 0
        d_pick.fill_(0x5A5A5A5A)
        torch.cuda.synchronize(dev)
        # a null cost array, an unknown cost flag, and the nulls of §3e
        assert lib.eppk_costed_resolve_device(*args(d_lists.data_ptr(), None, 0, C.byref(tab), d_pick.data_ptr())) == ARG
        assert "null cost" in err() and "eppk_costed_resolve_device" in err()
        assert lib.eppk_costed_resolve_device(*args(d_lists.data_ptr(), d_cost.data_ptr(), 2, C.byref(tab), d_pick.data_ptr())) == ARG
        assert "cost flags 2" in err()
        assert lib.eppk_costed_resolve_device(*args(d_lists.data_ptr(), d_cost.data_ptr(), 0, None, d_pick.data_ptr())) == ARG
        assert lib.eppk_costed_resolve_device(*args(None, d_cost.data_ptr(), 0, C.byref(tab), d_pick.data_ptr())) == ARG
        assert lib.eppk_costed_resolve_device(*args(d_lists.data_ptr(), d_cost.data_ptr(), 0, C.byref(tab), None)) == ARG
        assert lib.eppk_pick_costed(pk._ctx, wl.reqs[:8].ctypes.data, 8, None, 4, None, None, C.byref(tab), None, 6, None, d_pick.data_ptr(), None, None) == ARG
        assert "null cost" in err()
        assert lib.eppk_pick_costed_device(pk._ctx, d_reqs.data_ptr(), 8, None, 4, None, None, C.byref(tab), None, 6, None, d_pick.data_ptr(), None, None, None) == ARG
        assert lib.eppk_costed_resolve_device(None, d_lists.data_ptr(), None, 8, 4, d_cost.data_ptr(), 0, None, C.byref(tab), None, 6, None, d_pick.data_ptr(),
                                              None, None, None) == ARG
        with pytest.raises(pkg.EppkError) as ei:
            pk.pick_bounded_costed(np.zeros((R_E2E + 1, pk.row_words), dtype=np.uint64), 4, np.ones(R_E2E + 1, dtype=np.uint32), 6, ok)
        assert ei.value.code == LIMIT
        # a host form refuses the batch and names the lowest bad row: a cost of 0, a cost above EPPK_MAX_COST, a band byte >= n_bands
        for at, value, words in ((6, 0, ("row 6", "cost 0")), (2, cs.MAX_COST + 1, ("row 2", f"cost {cs.MAX_COST + 1}")), (0, 0xFFFFFFFF, ("row 0", "cost 4294967295"))):
            bad = cost.copy()
            bad[7], bad[at] = 0, value
            with pytest.raises(pkg.EppkError) as ei:
                pk.pick_bounded_costed(wl.reqs[:8], 4, bad, 6, ok, band)
            assert ei.value.code == ARG and all(w in str(ei.value) for w in words), str(ei.value)
        bad_band, bad = band.copy(), cost.copy()
        bad_band[3], bad[5] = 3, 0
        with pytest.raises(pkg.EppkError) as ei:
            pk.pick_bounded_costed(wl.reqs[:8], 4, bad, 6, ok, bad_band)
        assert ei.value.code == ARG and "row 3" in str(ei.value) and "band 3 of 3" in str(ei.value)
        torch.cuda.synchronize(dev)
        assert np.all(d_pick.cpu().numpy() == 0x5A5A5A5A), "a refused call writes nothing"
        # n_reqs = 0: nothing to do, nothing touched
        pk.bounded_resolve_costed_device(None, None, 0, 4, None, 0, None, ok, None, 6, None, None, None, None)
        assert pk.pick_bounded_costed(wl.reqs[:0], 4, cost[:0], 6, ok)[0].size == 0
    with pkg.BatchedPicker(wl.chain, max_pods=1024, max_blocks=wl.B, max_batch=8) as pk:
        with pytest.raises(pkg.EppkError) as ei:
            pk.pick_bounded_costed(wl.reqs[:8], 4, cost, 6, ok, band)
        assert ei.value.code == NO_SNAPSHOT


def test_the_scheduler_driver_on_the_device(pkg):
    """tests/cpp/test_costed_scheduler.cpp: a costed Bounded profile through eppk::Scheduler, against the real library."""
    exe = _load("test_costed_scheduler_cpp").build_driver()
    # a chunk of 64 rows: the scheduler's groups of 128 requests take the band order and the launches per band, the last group one launch
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120, env=dict(os.environ, EPPK_BOUND_CHUNK="64"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "costed scheduler: ok" in out.stdout
