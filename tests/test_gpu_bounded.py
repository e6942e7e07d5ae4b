"""GPU: the picker "best-score under per-pod caps" (SEMANTICS.md §3d; include/eppk.h eppk_bounded_resolve_device / eppk_pick_bounded)
against its numpy restatement (tests/bounded_ref.py), exactly: picks, ranks, loads, and scores as bit patterns.

The resolve alone on the generator's lists (tests/bounded_cases.py), placed by the chunk size the context reports; the same inputs under
different chunk sizes and grid widths; the pickers end to end against the oracle's lists fed through the restatement; composition with the
other list producers and with the post-route index update; argument checks; device groups.

The module sets the library switches itself (monkeypatch) before it creates a context."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# how the resolve is cut up: chunk size (EPPK_BOUND_CHUNK) and the width of the grid-stride loops (EPPK_MAX_CU)
GEOMETRIES = {"chunk64": {"EPPK_BOUND_CHUNK": "64"}, "default": {}, "chunk64-cu1": {"EPPK_BOUND_CHUNK": "64", "EPPK_MAX_CU": "1"},
              "default-cu1": {"EPPK_MAX_CU": "1"}}
MODES = {"default": {}, "quadmin4": {"EPPK_QUAD_MIN": "4"}, "quad0": {"EPPK_QUAD": "0"}}
QUEUE = 1


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def bc():
    return _load("bounded_cases")


def _setenv(monkeypatch, env):
    for name in ("EPPK_BOUND_CHUNK", "EPPK_MAX_CU"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _bare_picker(pkg):
    """A context for the resolve alone: the lists come from the test, the snapshot only says how many pods there are."""
    return pkg.BatchedPicker([(QUEUE, 1)], max_pods=4096, max_blocks=0, max_batch=64)


def _dev(torch, a, dtype=None):
    """A numpy array on the device (unsigned words travel as the signed type of their width)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).to(torch.device("cuda", 0))


def _resolve(pkg, pk, c):
    """One case through eppk_bounded_resolve_device: (pick, score | None, rank | None, load_out | None, launch-status flags)."""
    import torch
    dev = torch.device("cuda", 0)
    R, k = c["lists"].shape
    if pk.n_pods != c["n_pods"]:
        torch.cuda.synchronize(dev)
        pk.publish(np.zeros(c["n_pods"], dtype=pkg.picker.POD_DTYPE))
    d_lists = _dev(torch, c["lists"])
    d_ls = None if c["scores"] is None else _dev(torch, c["scores"])
    d_cap = None if c["cap"] is None else _dev(torch, c["cap"])
    d_load = None if c["load"] is None else _dev(torch, c["load"])
    d_pick = torch.full((max(R, 1),), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_score = None if c["no_score"] else torch.full((max(R, 1),), 7.25, dtype=torch.float64, device=dev)
    d_rank = None if c["no_rank"] else torch.full((max(R, 1),), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None                  # noqa: E731
    pk.bounded_resolve_device(d_lists.data_ptr() if R else None, ptr(d_ls), R, k, ptr(d_cap), c["cap_all"], c["policy"], ptr(d_load), d_pick.data_ptr(),
                              ptr(d_score), ptr(d_rank))
    flags = pk.launch_status()                                               # (synchronises)
    out = lambda t, dt: None if t is None else t.cpu().numpy()[:R].view(dt)  # noqa: E731
    return (out(d_pick, np.int32), out(d_score, np.float64), out(d_rank, np.uint8),
            None if d_load is None else d_load.cpu().numpy().view(np.uint32), flags)


def _diff(bc, c, got, want):
    """What differs between the device's answer and the restatement's, as text ('' = nothing)."""
    pick, score, rank, load, flags = got
    wp, ws, wr, wl, bad = want
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
    if bool(flags & bc.ref.LAUNCH_BAD_PICK) != bad or flags & ~bc.ref.LAUNCH_BAD_PICK:
        msgs.append(f"launch status {flags}, out-of-range entries: {bad}")
    return f"{bc.info(c)}: " + "; ".join(msgs) if msgs else ""


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_the_resolve_equals_the_restatement_on_the_smallest_shapes_that_can_break_it(pkg, bc, monkeypatch, geometry):
    _setenv(monkeypatch, GEOMETRIES[geometry])
    with _bare_picker(pkg) as pk:
        chunk, one_launch = pk.bounded_geometry()
        assert chunk == int(GEOMETRIES[geometry].get("EPPK_BOUND_CHUNK", chunk)) and chunk >= 64 and chunk & (chunk - 1) == 0
        assert one_launch == chunk
        cases = sorted(bc.make_cases(chunk), key=lambda c: c["n_pods"])       # (one publish per pod count)
        assert not set(bc.REQUIRED) - set().union(*(c["tags"] for c in cases))
        sizes = {c["lists"].shape[0] for c in cases}
        assert {one_launch - 1, one_launch, one_launch + 1, 3 * chunk + 7} <= sizes
        failed = [d for d in (_diff(bc, c, _resolve(pkg, pk, c), bc.want(c)) for c in cases) if d]
        assert not failed, f"{len(failed)} of {len(cases)} cases: " + " | ".join(failed[:6])


def _contended(bc, n, seed):
    rng = np.random.default_rng(bc.SEED0 + seed)
    P = 11
    lists = rng.integers(0, P, size=(n, 4)).astype(np.int32)
    lists[rng.random((n, 4)) < 0.35] = 3
    lists[rng.random((n, 4)) < 0.1] = bc.NO
    caps = rng.integers(0, max(2, n // 8), size=P).astype(np.uint32)
    return dict(name=f"contended-{n}", tags=set(), lists=lists, scores=rng.standard_normal((n, 4)), n_pods=P, cap=caps, cap_all=0, policy=seed & 1,
                load=rng.integers(0, 3, size=P).astype(np.uint32), no_score=False, no_rank=False)


def test_the_output_does_not_depend_on_chunk_size_or_grid(pkg, bc, monkeypatch):
    """The same inputs under EPPK_BOUND_CHUNK=64, the default chunk and EPPK_MAX_CU=1: identical outputs -- on either side of each
    geometry's one-launch threshold, and over several chunks with a ragged end."""
    sizes = set()
    for env in GEOMETRIES.values():
        _setenv(monkeypatch, env)
        with _bare_picker(pkg) as pk:
            one = pk.bounded_geometry()[1]
        sizes |= {one - 1, one, one + 1, 3 * one + 7}
    inputs = [_contended(bc, n, i) for i, n in enumerate(sorted(sizes))]
    results = {}
    for geometry, env in GEOMETRIES.items():
        _setenv(monkeypatch, env)
        with _bare_picker(pkg) as pk:
            results[geometry] = [_resolve(pkg, pk, c) for c in inputs]
    first = results["chunk64"]
    for geometry, res in results.items():
        for c, a, b in zip(inputs, first, res):
            for x, y, what in zip(a[:4], b[:4], ("picks", "scores", "ranks", "loads")):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{geometry} against chunk64, {bc.info(c)}: {what}"
    for c, got in zip(inputs, first):
        assert not _diff(bc, c, got, bc.want(c))


# ---- end to end ------------------------------------------------------------------------------------------------------------

R_E2E, P_E2E = 256, 1000


@pytest.fixture(scope="module")
def e2e(pkg, orc):
    """make_workload(3)-sized batch, its oracle index, a mask (one request without candidates), and the oracle's lists per (k, masked)."""
    wl = pkg.workload.make_workload(3, R=R_E2E, P=P_E2E)
    oix = orc.OracleIndex()
    oix.insert(wl.index_hashes, wl.index_pods)
    rng = np.random.default_rng(0xE2E)
    J = (P_E2E + 63) // 64
    mask = rng.integers(0, 1 << 63, size=(R_E2E, J), dtype=np.uint64) | (rng.integers(0, 2, size=(R_E2E, J), dtype=np.uint64) << np.uint64(63))
    mask[:, J - 1] &= np.uint64((1 << (P_E2E % 64)) - 1)
    mask[5, :] = 0
    lists = {}

    def topk(k, masked):
        if (k, masked) not in lists:
            lists[(k, masked)] = orc.pick_topk_batch(wl.chain, wl.pods, oix, wl.reqs, wl.B, k, mask=mask if masked else None, threads=8)
        return lists[(k, masked)]

    return dict(wl=wl, oix=oix, mask=mask, topk=topk)


# The batches of R_E2E = 256 requests under a chunk of 64 rows span four chunks and take the count / scan / assign launches per round, as the
# 64k x 4096 batches do; under the default chunk they take the one-launch kernel.
CHUNKINGS = {"chunk64": {"EPPK_BOUND_CHUNK": "64"}, "default": {}}


@pytest.fixture(params=list(CHUNKINGS))
def chunking(request, monkeypatch):
    _setenv(monkeypatch, CHUNKINGS[request.param])
    return request.param


def _check_chunking(chunking, geometry, n_reqs=R_E2E):
    chunk, one_launch = geometry
    if chunking == "chunk64":
        assert chunk == 64 and n_reqs > one_launch, "the batch spans several chunks"
    else:
        assert n_reqs <= one_launch, "the batch fits the one-launch kernel"


def _picker(pkg, wl, chunking, max_batch=R_E2E):
    pk = pkg.BatchedPicker(wl.chain, max_pods=1024, max_blocks=wl.B, max_batch=max_batch, index_slots=wl.index_slots)
    _check_chunking(chunking, pk.bounded_geometry())
    pk.publish(wl.pods)
    pk.index_insert(wl.index_hashes, wl.index_pods)
    return pk


def _same(got, want, what):
    for g, w, name in zip(got, want, ("picks", "scores", "ranks", "loads")):
        assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)), f"{what}: {name}"


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_pick_bounded_equals_the_oracle_lists_through_the_restatement(pkg, bc, e2e, monkeypatch, chunking, mode, masked):
    import torch
    for name, value in MODES[mode].items():
        monkeypatch.setenv(name, value)
    wl, mask = e2e["wl"], e2e["mask"] if masked else None
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(77)
    caps = rng.integers(0, 4, size=P_E2E).astype(np.uint32)
    load0 = rng.integers(0, 2, size=P_E2E).astype(np.uint32)
    with _picker(pkg, wl, chunking) as pk:
        d_reqs = _dev(torch, wl.reqs)
        d_mask = _dev(torch, mask) if masked else None
        for k, cap, cap_all, policy, load in ((1, None, 1, bc.ref.SHED, None), (4, None, 1, bc.ref.SPILL, load0), (4, caps, 0, bc.ref.SHED, load0),
                                              (8, None, 2, bc.ref.SHED, None), (8, caps, 0, bc.ref.SPILL, None)):
            lp, ls = e2e["topk"](k, masked)
            want = bc.ref.resolve(lp, ls, P_E2E, cap, cap_all, policy, load)
            assert not want[4] and (want[2] != 0).any(), "the caps bind"
            got = pk.pick_bounded(wl.reqs, k, cap if cap is not None else cap_all, policy, load, mask)
            what = f"{mode} masked {masked} k {k} policy {policy}"
            _same(got[:3], want[:3], "pick_bounded " + what)
            assert (got[3] is None) == (load is None) and (load is None or np.array_equal(got[3], want[3])), what
            if masked:
                assert got[0][5] == -1 and got[2][5] == bc.ref.RANK_NONE
            # the device form: nothing leaves the device
            d_cap = _dev(torch, cap) if cap is not None else None
            d_load = _dev(torch, load) if load is not None else None
            d_pick = torch.empty(R_E2E, dtype=torch.int32, device=dev)
            d_score = torch.empty(R_E2E, dtype=torch.float64, device=dev)
            d_rank = torch.empty(R_E2E, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            pk.pick_bounded_device(d_reqs.data_ptr(), R_E2E, d_mask.data_ptr() if masked else None, k, d_cap.data_ptr() if cap is not None else None,
                                   cap_all, policy, d_load.data_ptr() if load is not None else None, d_pick.data_ptr(), d_score.data_ptr(),
                                   d_rank.data_ptr())
            assert pk.launch_status() == 0
            _same((d_pick.cpu().numpy(), d_score.cpu().numpy(), d_rank.cpu().numpy()), want[:3], "pick_bounded_device " + what)
            if load is not None:
                assert np.array_equal(d_load.cpu().numpy().view(np.uint32), want[3]), what


@pytest.mark.parametrize("masked", [False, True])
def test_caps_that_bind_nothing_equal_pick(pkg, bc, e2e, chunking, masked):
    wl, mask = e2e["wl"], e2e["mask"] if masked else None
    with _picker(pkg, wl, chunking) as pk:
        wp, ws = pk.pick(wl.reqs, mask)
        for k, policy in ((1, bc.ref.SHED), (4, bc.ref.SPILL)):
            picks, scores, ranks, _ = pk.pick_bounded(wl.reqs, k, R_E2E, policy, mask=mask)
            assert np.array_equal(picks, wp) and np.array_equal(scores.view(np.uint64), ws.view(np.uint64))
            assert np.array_equal(ranks, np.where(wp >= 0, 0, bc.ref.RANK_NONE).astype(np.uint8))


def test_the_resolve_composes_with_the_other_list_producers(pkg, bc, e2e, chunking):
    """Weighted-random rounds and filtered fallbacks are [n_reqs][k] lists like any other."""
    import torch
    wl = e2e["wl"]
    dev = torch.device("cuda", 0)
    k = 4
    with _picker(pkg, wl, chunking) as pk:
        d_reqs = _dev(torch, wl.reqs)
        d_lists = torch.empty((R_E2E, k), dtype=torch.int32, device=dev)
        d_ls = torch.empty((R_E2E, k), dtype=torch.float64, device=dev)
        d_pick = torch.empty(R_E2E, dtype=torch.int32, device=dev)
        d_score = torch.empty(R_E2E, dtype=torch.float64, device=dev)
        d_rank = torch.empty(R_E2E, dtype=torch.uint8, device=dev)
        d_load = torch.zeros(P_E2E, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)

        def resolve_and_compare(what, policy):
            d_load.zero_()
            torch.cuda.synchronize(dev)
            pk.bounded_resolve_device(d_lists.data_ptr(), d_ls.data_ptr(), R_E2E, k, None, 1, policy, d_load.data_ptr(), d_pick.data_ptr(),
                                      d_score.data_ptr(), d_rank.data_ptr())
            assert pk.launch_status() == 0
            want = bc.ref.resolve(d_lists.cpu().numpy(), d_ls.cpu().numpy(), P_E2E, None, 1, policy, np.zeros(P_E2E, dtype=np.uint32))
            assert (want[2] != 0).any(), what
            _same((d_pick.cpu().numpy(), d_score.cpu().numpy(), d_rank.cpu().numpy(), d_load.cpu().numpy()), want[:4], what)

        pk.pick_weighted_random_device(d_reqs.data_ptr(), R_E2E, None, k, 0xC0FFEE, d_lists.data_ptr(), d_ls.data_ptr())
        resolve_and_compare("weighted-random rounds", bc.ref.SPILL)
        pk.set_filters([[(pkg.picker.PredicateKind.QUEUE_LE, pkg.picker.OnEmpty.REQUIRE, int(np.median(wl.pods["queue"])))]])
        pk.pick_filtered_device(d_reqs.data_ptr(), R_E2E, None, None, k, d_lists.data_ptr(), d_ls.data_ptr(), None)
        resolve_and_compare("filtered fallbacks", bc.ref.SHED)


def test_the_index_learns_bounded_picks(pkg, orc, bc, e2e, chunking):
    """eppk_index_insert_picks_device takes the bounded picks as they are; the next batch is scored against the index they leave."""
    import torch
    wl = e2e["wl"]
    dev = torch.device("cuda", 0)
    k = 4
    lp, ls = e2e["topk"](k, False)
    want = bc.ref.resolve(lp, ls, P_E2E, None, 1, bc.ref.SHED, None)
    assert (want[0] == -1).any() and (want[0] >= 0).any()
    oix = orc.OracleIndex()
    oix.insert(wl.index_hashes, wl.index_pods)
    oix.insert_picks(wl.reqs, wl.B, want[0])
    second = pkg.workload.make_requests(wl, 4242, revisit_of=wl.reqs, revisit_frac=0.5)
    op, osc, _ = orc.pick_batch(wl.chain, wl.pods, oix, second, wl.B)
    with _picker(pkg, wl, chunking) as pk:
        d_reqs = _dev(torch, wl.reqs)
        d_pick = torch.empty(R_E2E, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        pk.pick_bounded_device(d_reqs.data_ptr(), R_E2E, None, k, None, 1, bc.ref.SHED, None, d_pick.data_ptr(), None, None)
        pk.index_insert_picks_device(d_reqs.data_ptr(), d_pick.data_ptr(), R_E2E)
        assert pk.launch_status() == 0
        assert np.array_equal(d_pick.cpu().numpy(), want[0])
        assert pk.index_size() == oix.size() and pk.index_selfcheck() == 0
        picks, scores = pk.pick(second)
        assert np.array_equal(picks, op) and np.array_equal(scores.view(np.uint64), osc.view(np.uint64))


def test_argument_validation(pkg, bc, e2e, monkeypatch):
    _setenv(monkeypatch, {})
    import torch
    wl = e2e["wl"]
    lib = pkg.load_library()
    ARG, LIMIT, NO_SNAPSHOT = -1, -2, -4
    dev = torch.device("cuda", 0)
    d_lists = torch.zeros((8, 8), dtype=torch.int32, device=dev)
    d_pick = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_reqs = _dev(torch, wl.reqs[:8])
    torch.cuda.synchronize(dev)
    with _picker(pkg, wl, "default") as pk:
        def calls(k, policy):
            return (("pick_bounded", lambda: pk.pick_bounded(wl.reqs[:8], k, 1, policy)),
                    ("pick_bounded_device", lambda: pk.pick_bounded_device(d_reqs.data_ptr(), 8, None, k, None, 1, policy, None, d_pick.data_ptr(), None, None)),
                    ("bounded_resolve_device", lambda: pk.bounded_resolve_device(d_lists.data_ptr(), None, 8, k, None, 1, policy, None, d_pick.data_ptr(), None, None)))

        for k, policy, word in ((0, 0, "k out of range"), (9, 0, "k out of range"), (4, 2, "unknown policy"), (4, 0xFFFFFFFF, "unknown policy")):
            for name, call in calls(k, policy):
                with pytest.raises(pkg.EppkError) as ei:
                    call()
                assert ei.value.code == ARG and word in str(ei.value) and name in str(ei.value), (name, k, policy, str(ei.value))
        pk.set_assumed_load(2)
        for name, call in calls(4, 0):
            with pytest.raises(pkg.EppkError) as ei:
                call()
            assert ei.value.code == ARG and "assumed load" in str(ei.value), (name, str(ei.value))
        pk.set_assumed_load(0)
        assert lib.eppk_bounded_resolve_device(pk._ctx, None, None, 8, 4, None, 1, 0, None, d_pick.data_ptr(), None, None, None) == ARG
        assert lib.eppk_bounded_resolve_device(pk._ctx, d_lists.data_ptr(), None, 8, 4, None, 1, 0, None, None, None, None, None) == ARG
        assert lib.eppk_pick_bounded(pk._ctx, None, 8, None, 4, None, 1, 0, None, d_pick.data_ptr(), None, None) == ARG
        assert lib.eppk_bounded_resolve_device(None, d_lists.data_ptr(), None, 8, 4, None, 1, 0, None, d_pick.data_ptr(), None, None, None) == ARG
        assert lib.eppk_bounded_geometry(None, None) == ARG
        with pytest.raises(pkg.EppkError) as ei:
            pk.pick_bounded(np.zeros((R_E2E + 1, pk.row_words), dtype=np.uint64), 4, 1)
        assert ei.value.code == LIMIT
        bad = wl.reqs[:8].copy()
        bad[3, 0] = np.uint64(128)                                            # adapter 128
        with pytest.raises(pkg.EppkError) as ei:
            pk.pick_bounded(bad, 4, 1)
        assert ei.value.code == ARG and "row 3" in str(ei.value)
        torch.cuda.synchronize(dev)
        assert np.all(d_pick.cpu().numpy() == 0x5A5A5A5A), "a refused call writes nothing"
        # n_reqs = 0: nothing to do, nothing touched
        pk.bounded_resolve_device(None, None, 0, 4, None, 1, 0, None, None, None, None)
        assert pk.pick_bounded(wl.reqs[:0], 4, 1)[0].size == 0
    with pkg.BatchedPicker(wl.chain, max_pods=1024, max_blocks=wl.B, max_batch=8) as pk:
        for name, call in (("pick_bounded", lambda: pk.pick_bounded(wl.reqs[:8], 4, 1)),
                           ("bounded_resolve_device", lambda: pk.bounded_resolve_device(d_lists.data_ptr(), None, 8, 4, None, 1, 0, None, d_pick.data_ptr(),
                                                                                         None, None))):
            with pytest.raises(pkg.EppkError) as ei:
                call()
            assert ei.value.code == NO_SNAPSHOT, name


@pytest.mark.parametrize("members", [2, 3])
def test_a_group_equals_the_single_context(pkg, bc, e2e, chunking, members):
    wl, mask = e2e["wl"], e2e["mask"]
    rng = np.random.default_rng(members)
    caps = rng.integers(0, 3, size=P_E2E).astype(np.uint32)
    load0 = rng.integers(0, 2, size=P_E2E).astype(np.uint32)
    settings = ((4, 1, bc.ref.SHED, None, None), (4, caps, bc.ref.SPILL, load0, mask), (8, 2, bc.ref.SPILL, load0, None), (1, caps, bc.ref.SHED, None, mask))
    with _picker(pkg, wl, chunking) as pk:
        single = [pk.pick_bounded(wl.reqs, k, cap, policy, load, m) for k, cap, policy, load, m in settings]
    with pkg.DeviceGroup(wl.chain, [0] * members, max_pods=1024, max_blocks=wl.B, max_batch=R_E2E, index_slots=wl.index_slots, min_shard=1) as g:
        geo = (C.c_uint32 * 2)()
        lib = pkg.load_library()
        assert lib.eppk_bounded_geometry(lib.eppk_group_ctx(g._g, 0), geo) == 0      # member 0 resolves
        _check_chunking(chunking, (int(geo[0]), int(geo[1])))
        g.publish(wl.pods)
        g.index_insert(wl.index_hashes, wl.index_pods)
        for (k, cap, policy, load, m), want in zip(settings, single):
            got = g.pick_bounded(wl.reqs, k, cap, policy, load, m)
            _same(got[:3], want[:3], f"{members} members k {k} policy {policy}")
            assert (got[3] is None) == (load is None) and (load is None or np.array_equal(got[3], want[3]))
            assert (want[2] != 0).any()
        for k in (0, 9):
            with pytest.raises(pkg.EppkError) as ei:
                g.pick_bounded(wl.reqs, k, 1)
            assert ei.value.code == -1 and "k out of range" in str(ei.value)
        assert g.pick_bounded(wl.reqs[:0], 4, 1)[0].size == 0
