"""GPU: priority bands over the bounded picker (SEMANTICS.md §3e; include/eppk.h eppk_banded_resolve_device / eppk_pick_banded) against
the numpy restatement (tests/banded_ref.py), exactly: picks, ranks, loads, scores as bit patterns, and the sticky launch status.

The resolve alone on the generator's cases (tests/banded_cases.py), placed by the chunk size the context reports; one band without a
reserve against the plain bounded resolve; the same inputs under different chunk sizes and grid widths; the picker end to end against
the oracle's lists fed through the restatement; argument checks; device groups; the C++ scheduler driver.

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


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def bn():
    return _load("banded_cases")


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


def _resolve(pkg, pk, c, plain_policy=None):
    """One case through eppk_banded_resolve_device -- or, with plain_policy, its lists, caps and loads through the plain
    eppk_bounded_resolve_device: (pick, score | None, rank | None, load_out | None, launch-status flags)."""
    import torch
    dev = torch.device("cuda", 0)
    R, k = c["lists"].shape
    if pk.n_pods != c["n_pods"]:
        torch.cuda.synchronize(dev)
        pk.publish(np.zeros(c["n_pods"], dtype=pkg.picker.POD_DTYPE))
    d_lists = _dev(torch, c["lists"])
    d_ls = None if c["scores"] is None else _dev(torch, c["scores"])
    d_band = None if c["band"] is None or R == 0 else _dev(torch, c["band"])
    d_cap = None if c["cap"] is None else _dev(torch, c["cap"])
    d_load = None if c["load"] is None else _dev(torch, c["load"])
    d_pick = torch.full((max(R, 1),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_score = None if c["no_score"] else torch.full((max(R, 1),), 7.25, dtype=torch.float64, device=dev)
    d_rank = None if c["no_rank"] else torch.full((max(R, 1),), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None                  # noqa: E731
    if plain_policy is None:
        pk.bounded_resolve_banded_device(d_lists.data_ptr() if R else None, ptr(d_ls), R, k, ptr(d_band), c["bands"], ptr(d_cap), c["cap_all"], ptr(d_load),
                                         d_pick.data_ptr(), ptr(d_score), ptr(d_rank))
    else:
        pk.bounded_resolve_device(d_lists.data_ptr() if R else None, ptr(d_ls), R, k, ptr(d_cap), c["cap_all"], plain_policy, ptr(d_load),
                                  d_pick.data_ptr(), ptr(d_score), ptr(d_rank))
    flags = pk.launch_status()                                               # (synchronises)
    out = lambda t, dt: None if t is None else t.cpu().numpy()[:R].view(dt)  # noqa: E731
    return (out(d_pick, np.int32), out(d_score, np.float64), out(d_rank, np.uint8),
            None if d_load is None else d_load.cpu().numpy().view(np.uint32), flags)


def _diff(bn, c, got, want):
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
        msgs.append(f"loads differ: gpu {load[:8]} want {wl[:8]}")
    if flags != wflags:
        msgs.append(f"launch status {flags}, want {wflags}")
    return f"{bn.info(c)}: " + "; ".join(msgs) if msgs else ""


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_the_resolve_equals_the_restatement_on_the_smallest_shapes_that_can_break_it(pkg, bn, monkeypatch, geometry):
    _setenv(monkeypatch, GEOMETRIES[geometry])
    with _bare_picker(pkg, geometry) as pk:
        chunk = pk.bounded_geometry()[0]
        cases = sorted(bn.make_cases(chunk), key=lambda c: c["n_pods"])       # (one publish per pod count)
        assert not set(bn.REQUIRED) - set().union(*(c["tags"] for c in cases))
        sizes = {c["lists"].shape[0] for c in cases}
        assert {0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 7} <= sizes and max(sizes) <= 4 * chunk + 100
        failed = [d for d in (_diff(bn, c, _resolve(pkg, pk, c), bn.want(c)) for c in cases) if d]
        assert not failed, f"{len(failed)} of {len(cases)} cases: " + " | ".join(failed[:6])


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_one_band_without_reserve_equals_the_plain_resolve(pkg, bn, monkeypatch, geometry):
    """n_bands = 1, reserve 0: the outputs of eppk_bounded_resolve_device on the same inputs, bit for bit."""
    _setenv(monkeypatch, GEOMETRIES[geometry])
    with _bare_picker(pkg, geometry) as pk:
        chunk = pk.bounded_geometry()[0]
        cases = sorted((c for c in bn.make_cases(chunk) if bn.host_ok(c)), key=lambda c: c["n_pods"])[::3]
        assert any(c["lists"].shape[0] > chunk for c in cases) and any(0 < c["lists"].shape[0] <= chunk for c in cases)
        for i, c in enumerate(cases):
            policy = i & 1
            one = dict(c, bands=[(policy, 0)], band=None if i % 3 else np.zeros(c["lists"].shape[0], dtype=np.uint8))
            got, want = _resolve(pkg, pk, one), _resolve(pkg, pk, c, plain_policy=policy)
            for x, y, what in zip(got[:4], want[:4], ("picks", "scores", "ranks", "loads")):
                assert (x is None and y is None) or np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{bn.info(c)}: {what}"
            assert got[4] == want[4], f"{bn.info(c)}: launch status"


def _contended(bn, n, seed):
    rng = np.random.default_rng(bn.SEED0 + seed)
    P, nb = 11, (2, 3, 8)[seed % 3]
    lists = rng.integers(0, P, size=(n, 4)).astype(np.int32)
    lists[rng.random((n, 4)) < 0.35] = 3
    lists[rng.random((n, 4)) < 0.1] = bn.NO
    caps = rng.integers(0, max(2, n // 8), size=P).astype(np.uint32)
    return dict(name=f"contended-{n}", tags=set(), lists=lists, scores=rng.standard_normal((n, 4)), n_pods=P, bands=bn._table(rng, nb, 3),
                band=rng.integers(0, nb, size=n).astype(np.uint8), cap=caps, cap_all=0, load=rng.integers(0, 3, size=P).astype(np.uint32),
                no_score=False, no_rank=False)


def test_the_output_does_not_depend_on_chunk_size_or_grid(pkg, bn, monkeypatch):
    """The same inputs under EPPK_BOUND_CHUNK=64, the default chunk and EPPK_MAX_CU=1: identical outputs -- on either side of each
    geometry's one-launch threshold, and over several chunks with a ragged end."""
    sizes = set()
    for env in GEOMETRIES.values():
        _setenv(monkeypatch, env)
        with _bare_picker(pkg) as pk:
            one = pk.bounded_geometry()[1]
        sizes |= {one - 1, one, one + 1, 3 * one + 7}
    inputs = [_contended(bn, n, i) for i, n in enumerate(sorted(sizes))]
    results = {}
    for geometry, env in GEOMETRIES.items():
        _setenv(monkeypatch, env)
        with _bare_picker(pkg, geometry) as pk:
            results[geometry] = [_resolve(pkg, pk, c) for c in inputs]
    first = results["chunk64"]
    for geometry, res in results.items():
        for c, a, b in zip(inputs, first, res):
            for x, y, what in zip(a[:4], b[:4], ("picks", "scores", "ranks", "loads")):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{geometry} against chunk64, {bn.info(c)}: {what}"
    for c, got in zip(inputs, first):
        assert not _diff(bn, c, got, bn.want(c))


# ---- end to end ------------------------------------------------------------------------------------------------------------

R_E2E, P_E2E = 256, 1000                                                     # (the batch tests/test_gpu_bounded.py takes end to end)
CHUNKINGS = {"chunk64": {"EPPK_BOUND_CHUNK": "64"}, "default": {}}


@pytest.fixture(scope="module")
def e2e(pkg, orc):
    """make_workload(3)-sized batch, its oracle index, a mask (one request without candidates), band bytes, and the oracle's lists."""
    wl = pkg.workload.make_workload(3, R=R_E2E, P=P_E2E)
    oix = orc.OracleIndex()
    oix.insert(wl.index_hashes, wl.index_pods)
    rng = np.random.default_rng(0xE2E)
    J = (P_E2E + 63) // 64
    mask = rng.integers(0, 1 << 63, size=(R_E2E, J), dtype=np.uint64) | (rng.integers(0, 2, size=(R_E2E, J), dtype=np.uint64) << np.uint64(63))
    mask[:, J - 1] &= np.uint64((1 << (P_E2E % 64)) - 1)
    mask[5, :] = 0
    band = rng.choice(3, size=R_E2E, p=[0.1, 0.6, 0.3]).astype(np.uint8)
    lists = {}

    def topk(k, masked):
        if (k, masked) not in lists:
            lists[(k, masked)] = orc.pick_topk_batch(wl.chain, wl.pods, oix, wl.reqs, wl.B, k, mask=mask if masked else None, threads=8)
        return lists[(k, masked)]

    return dict(wl=wl, mask=mask, band=band, topk=topk)


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
SETTINGS = ((1, None, 1, [(0, 0), (0, 0), (0, 0)], False), (4, None, 2, [(1, 0), (0, 1), (0, 2)], True),
            (4, "caps", 0, [(0, 0), (1, 1), (0, 1)], True), (8, None, 2, [(0, 0), (0, 0), (1, 2)], False))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_pick_bounded_banded_equals_the_oracle_lists_through_the_restatement(pkg, bn, e2e, monkeypatch, chunking, mode, masked):
    import torch
    for name, value in MODES[mode].items():
        monkeypatch.setenv(name, value)
    wl, mask, band = e2e["wl"], e2e["mask"] if masked else None, e2e["band"]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    caps = rng.integers(0, 5, size=P_E2E).astype(np.uint32)
    load0 = rng.integers(0, 2, size=P_E2E).astype(np.uint32)
    with _picker(pkg, wl, chunking) as pk:
        d_reqs = _dev(torch, wl.reqs)
        d_mask = _dev(torch, mask) if masked else None
        d_band = _dev(torch, band)
        for k, cap, cap_all, bands, with_load in SETTINGS:
            cap = caps if cap is not None else None
            load = load0 if with_load else None
            lp, ls = e2e["topk"](k, masked)
            want = bn.ref.resolve(lp, ls, P_E2E, bands, band, cap, cap_all, load)
            plain = bn.ref.ref.resolve(lp, ls, P_E2E, cap, cap_all, bands[0][0], load)
            assert want[4] == 0 and (want[2] != 0).any() and not np.array_equal(want[0], plain[0]), "the caps bind, and the bands decide"
            got = pk.pick_bounded_banded(wl.reqs, k, cap if cap is not None else cap_all, bands, band, load, mask)
            what = f"{mode} masked {masked} k {k} bands {bands}"
            _same(got[:3], want[:3], "pick_bounded_banded " + what)
            assert (got[3] is None) == (load is None) and (load is None or np.array_equal(got[3], want[3])), what
            if masked:
                assert got[0][5] == -1 and got[2][5] == bn.ref.RANK_NONE
            # the device form: nothing leaves the device
            d_cap = _dev(torch, cap) if cap is not None else None
            d_load = _dev(torch, load) if load is not None else None
            d_pick = torch.empty(R_E2E, dtype=torch.int32, device=dev)
            d_score = torch.empty(R_E2E, dtype=torch.float64, device=dev)
            d_rank = torch.empty(R_E2E, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            pk.pick_bounded_banded_device(d_reqs.data_ptr(), R_E2E, d_mask.data_ptr() if masked else None, k, d_band.data_ptr(), bands,
                                          d_cap.data_ptr() if cap is not None else None, cap_all, d_load.data_ptr() if load is not None else None,
                                          d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr())
            assert pk.launch_status() == 0
            _same((d_pick.cpu().numpy(), d_score.cpu().numpy(), d_rank.cpu().numpy()), want[:3], "pick_bounded_banded_device " + what)
            if load is not None:
                assert np.array_equal(d_load.cpu().numpy().view(np.uint32), want[3]), what


@pytest.mark.parametrize("members", [2, 3])
def test_a_group_equals_the_single_context(pkg, bn, e2e, chunking, members):
    wl, mask, band = e2e["wl"], e2e["mask"], e2e["band"]
    rng = np.random.default_rng(members)
    caps = rng.integers(0, 3, size=P_E2E).astype(np.uint32)
    load0 = rng.integers(0, 2, size=P_E2E).astype(np.uint32)
    settings = ((4, 1, [(0, 0), (0, 0), (0, 0)], band, None, None), (4, caps, [(1, 0), (0, 1), (1, 1)], band, load0, mask),
                (8, 2, [(0, 0), (1, 1)], band % 2, load0, None), (1, caps, [(0, 0), (0, 2), (0, 2)], None, None, mask))
    with _picker(pkg, wl, chunking) as pk:
        single = [pk.pick_bounded_banded(wl.reqs, k, cap, bands, b, load, m) for k, cap, bands, b, load, m in settings]
    with pkg.DeviceGroup(wl.chain, [0] * members, max_pods=1024, max_blocks=wl.B, max_batch=R_E2E, index_slots=wl.index_slots, min_shard=1) as g:
        g.publish(wl.pods)
        g.index_insert(wl.index_hashes, wl.index_pods)
        for (k, cap, bands, b, load, m), want in zip(settings, single):
            got = g.pick_bounded_banded(wl.reqs, k, cap, bands, b, load, m)
            _same(got[:3], want[:3], f"{members} members k {k} bands {bands}")
            assert (got[3] is None) == (load is None) and (load is None or np.array_equal(got[3], want[3]))
            assert (want[2] != 0).any()
        with pytest.raises(pkg.EppkError) as ei:
            g.pick_bounded_banded(wl.reqs, 4, 1, [(0, 2), (0, 1)], band)
        assert ei.value.code == -1 and "reserve" in str(ei.value)
        bad = band.copy()
        bad[7] = 3
        with pytest.raises(pkg.EppkError) as ei:
            g.pick_bounded_banded(wl.reqs, 4, 1, [(0, 0)] * 3, bad)
        assert ei.value.code == -1 and "row 7" in str(ei.value)
        assert g.pick_bounded_banded(wl.reqs[:0], 4, 1, [(0, 0)])[0].size == 0


def test_argument_validation(pkg, bn, e2e, monkeypatch):
    _setenv(monkeypatch, {})
    import torch
    wl, band = e2e["wl"], e2e["band"][:8]
    lib = pkg.load_library()
    ARG, LIMIT, NO_SNAPSHOT = -1, -2, -4
    dev = torch.device("cuda", 0)
    d_lists = torch.zeros((8, 8), dtype=torch.int32, device=dev)
    d_pick = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_reqs = _dev(torch, wl.reqs[:8])
    d_band = _dev(torch, band)
    torch.cuda.synchronize(dev)
    ok = [(0, 0), (1, 1), (0, 1)]
    with _picker(pkg, wl, "default") as pk:
        def calls(k, bands):
            return (("pick_banded", lambda: pk.pick_bounded_banded(wl.reqs[:8], k, 1, bands, band)),
                    ("pick_banded_device", lambda: pk.pick_bounded_banded_device(d_reqs.data_ptr(), 8, None, k, d_band.data_ptr(), bands, None, 1, None,
                                                                                 d_pick.data_ptr(), None, None)),
                    ("banded_resolve_device", lambda: pk.bounded_resolve_banded_device(d_lists.data_ptr(), None, 8, k, d_band.data_ptr(), bands, None, 1,
                                                                                       None, d_pick.data_ptr(), None, None)))

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
        # an entry behind n_bands is not read: garbage there is no error
        tab.policy[1], tab.reserve[1] = 77, 0
        assert lib.eppk_banded_resolve_device(pk._ctx, d_lists.data_ptr(), None, 8, 4, None, C.byref(tab), None, 1, None, d_pick.data_ptr(), None, None, None) == 0
        assert pk.launch_status() == 0
        d_pick.fill_(0x5A5A5A5A)
        torch.cuda.synchronize(dev)
        assert lib.eppk_banded_resolve_device(pk._ctx, d_lists.data_ptr(), None, 8, 4, None, None, None, 1, None, d_pick.data_ptr(), None, None, None) == ARG
        assert lib.eppk_banded_resolve_device(pk._ctx, None, None, 8, 4, None, C.byref(tab), None, 1, None, d_pick.data_ptr(), None, None, None) == ARG
        assert lib.eppk_banded_resolve_device(pk._ctx, d_lists.data_ptr(), None, 8, 4, None, C.byref(tab), None, 1, None, None, None, None, None) == ARG
        assert lib.eppk_pick_banded(pk._ctx, None, 8, None, 4, None, C.byref(tab), None, 1, None, d_pick.data_ptr(), None, None) == ARG
        assert lib.eppk_banded_resolve_device(None, d_lists.data_ptr(), None, 8, 4, None, C.byref(tab), None, 1, None, d_pick.data_ptr(), None, None, None) == ARG
        with pytest.raises(pkg.EppkError) as ei:
            pk.pick_bounded_banded(np.zeros((R_E2E + 1, pk.row_words), dtype=np.uint64), 4, 1, ok)
        assert ei.value.code == LIMIT
        # a band byte >= n_bands on a host form: the batch is refused, the lowest such row is named
        bad = band.copy()
        bad[6], bad[2] = 200, 3
        with pytest.raises(pkg.EppkError) as ei:
            pk.pick_bounded_banded(wl.reqs[:8], 4, 1, ok, bad)
        assert ei.value.code == ARG and "row 2" in str(ei.value) and "band 3 of 3" in str(ei.value)
        torch.cuda.synchronize(dev)
        assert np.all(d_pick.cpu().numpy() == 0x5A5A5A5A), "a refused call writes nothing"
        # n_reqs = 0: nothing to do, nothing touched
        pk.bounded_resolve_banded_device(None, None, 0, 4, None, ok, None, 1, None, None, None, None)
        assert pk.pick_bounded_banded(wl.reqs[:0], 4, 1, ok)[0].size == 0
    with pkg.BatchedPicker(wl.chain, max_pods=1024, max_blocks=wl.B, max_batch=8) as pk:
        with pytest.raises(pkg.EppkError) as ei:
            pk.pick_bounded_banded(wl.reqs[:8], 4, 1, ok, band)
        assert ei.value.code == NO_SNAPSHOT


def test_the_scheduler_driver_on_the_device(pkg):
    """tests/cpp/test_banded_scheduler.cpp: a Bounded profile with bands through eppk::Scheduler, against the real library."""
    exe = _load("test_banded_scheduler_cpp").build_driver()
    # a chunk of 64 rows: the scheduler's groups of 128 requests take the band order and the launches per band, the last group one launch
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120, env=dict(os.environ, EPPK_BOUND_CHUNK="64"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "banded scheduler: ok" in out.stdout
