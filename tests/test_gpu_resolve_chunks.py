"""GPU: the bounded, banded and cost-weighted resolves (SEMANTICS.md §3d-§3f; eppk_bounded.hip.h, eppk_banded.hip.h, eppk_costed.hip.h)
over MANY chunks, against their numpy restatements, exactly: picks, ranks, loads, scores as bit patterns, and the launch status.

The scan kernels cut the chunks of a batch (of a band) into 16 segments and walk a segment in trips of eight chunks; banded_offsets_kernel
cuts the chunks of the batch into 32.  tests/test_gpu_bounded.py, test_gpu_banded.py and test_gpu_costed.py stop at ten chunks -- one
chunk per segment -- and the 64k comparisons of scripts/gpu_bounded_time.py, gpu_banded_time.py and gpu_costed_time.py at 128 chunks:
seg_len == 8, one full trip and no more.  Here: 16, 17, 31, 32, 33, 128, 129 and 257 chunks of 64 and of 128 rows (EPPK_BOUND_CHUNK;
128 is new to the suite), each with the grid-stride loops at full width and under EPPK_MAX_CU=1; 17 and 33 chunks of the default 512
rows; once 1025 chunks of 64 rows.  The cases come from tests/resolve_chunk_cases.py, whose CPU twin is
tests/test_resolve_chunks_cpu.py; no case is skipped and every comparison is exact.

The module sets the library switches itself (monkeypatch) before it creates a context."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GEOMETRIES = {"chunk64": {"EPPK_BOUND_CHUNK": "64"}, "chunk128": {"EPPK_BOUND_CHUNK": "128"},
              "chunk64-cu1": {"EPPK_BOUND_CHUNK": "64", "EPPK_MAX_CU": "1"}, "chunk128-cu1": {"EPPK_BOUND_CHUNK": "128", "EPPK_MAX_CU": "1"},
              "default": {}}
QUEUE = 1
PER_ENTRY = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rc = _load("resolve_chunk_cases")
COUNTS = {g: ((17, 33) if g == "default" else rc.COUNTS) for g in GEOMETRIES}
RUNS = [(g, n) for g in GEOMETRIES for n in COUNTS[g]]


def _setenv(monkeypatch, env):
    for name in ("EPPK_BOUND_CHUNK", "EPPK_MAX_CU"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _bare_picker(pkg, geometry):
    """A context for the resolve alone: the lists come from the test, the snapshot only says how many pods there are.  max_batch = 64:
    every per-request buffer of the context has to grow to the batch."""
    pk = pkg.BatchedPicker([(QUEUE, 1)], max_pods=4096, max_blocks=0, max_batch=64)
    chunk, one_launch = pk.bounded_geometry()
    assert chunk == int(GEOMETRIES[geometry].get("EPPK_BOUND_CHUNK", 512)) and one_launch == chunk
    return pk


def _dev(torch, a):
    """A numpy array on the device (unsigned words travel as the signed type of their width)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).to(torch.device("cuda", 0))


def _resolve(pkg, pk, family, c):
    """One case through eppk_bounded_resolve_device / eppk_banded_resolve_device / eppk_costed_resolve_device:
    (pick, score | None, rank | None, load_out | None, launch-status flags)."""
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
    d_band = None if c.get("band") is None else _dev(torch, c["band"])
    d_cost = None if family != "costed" else _dev(torch, c["cost"])
    d_pick = torch.full((R,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_score = None if c["no_score"] else torch.full((R,), 7.25, dtype=torch.float64, device=dev)
    d_rank = None if c["no_rank"] else torch.full((R,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None                  # noqa: E731
    if family == "bounded":
        pk.bounded_resolve_device(d_lists.data_ptr(), ptr(d_ls), R, k, ptr(d_cap), c["cap_all"], c["policy"], ptr(d_load), d_pick.data_ptr(), ptr(d_score),
                                  ptr(d_rank))
    elif family == "banded":
        pk.bounded_resolve_banded_device(d_lists.data_ptr(), ptr(d_ls), R, k, ptr(d_band), c["bands"], ptr(d_cap), c["cap_all"], ptr(d_load),
                                         d_pick.data_ptr(), ptr(d_score), ptr(d_rank))
    else:
        pk.bounded_resolve_costed_device(d_lists.data_ptr(), ptr(d_ls), R, k, d_cost.data_ptr(), PER_ENTRY if c["per_entry"] else 0, ptr(d_band), c["bands"],
                                         ptr(d_cap), c["cap_all"], ptr(d_load), d_pick.data_ptr(), ptr(d_score), ptr(d_rank))
    flags = pk.launch_status()                                               # (synchronises)
    out = lambda t, dt: None if t is None else t.cpu().numpy().view(dt)      # noqa: E731
    return (out(d_pick, np.int32), out(d_score, np.float64), out(d_rank, np.uint8),
            None if d_load is None else d_load.cpu().numpy().view(np.uint32), flags)


def _flags(want):
    """The launch status a restatement's fifth value stands for (bounded_ref: a bool, the others: the flags)."""
    return rc.bc.ref.LAUNCH_BAD_PICK if want[4] is True else int(want[4])


def _diff(family, c, chunk, got, want):
    """What differs between the device's answer and the restatement's, as text ('' = nothing): the case, the first differing rows, and
    the chunk and scan segment they lie in."""
    pick, score, rank, load, flags = got
    wp, ws, wr, wl = want[:4]
    msgs = []
    if not np.array_equal(pick, wp):
        r = np.nonzero(pick != wp)[0]
        msgs.append(f"picks differ in {r.size} rows, first {r[:4]}: gpu {pick[r[:4]]} want {wp[r[:4]]} ({rc.locate(c, chunk, r[:2])})")
    if score is not None and not np.array_equal(score.view(np.uint64), ws.view(np.uint64)):
        r = np.nonzero(score.view(np.uint64) != ws.view(np.uint64))[0]
        msgs.append(f"scores differ (bitwise) in {r.size} rows, first {r[:4]} ({rc.locate(c, chunk, r[:2])})")
    if rank is not None and not np.array_equal(rank, wr):
        r = np.nonzero(rank != wr)[0]
        msgs.append(f"ranks differ in {r.size} rows, first {r[:4]}: gpu {rank[r[:4]]} want {wr[r[:4]]} ({rc.locate(c, chunk, r[:2])})")
    if load is not None and not np.array_equal(load, wl):
        p = np.nonzero(load != wl)[0]
        msgs.append(f"loads differ on pods {p[:4]}: gpu {load[p[:4]]} want {wl[p[:4]]}")
    if flags != _flags(want):
        msgs.append(f"launch status {flags}, want {_flags(want)}")
    return f"{family} {rc.INFO[family](c)}: " + "; ".join(msgs) if msgs else ""


def _forms(family, c, i):
    """The entry points a case goes through: its own, and the ones that have to give the same answer -- a bounded case as one band
    with reserve 0, a banded case at cost 1 (per request and, every other case, per entry)."""
    out = [(family, c)]
    if family == "bounded":
        out.append(("banded", rc.as_banded(c)))
    if family != "costed":
        out.append(("costed", rc.as_costed(out[-1][1], per_entry=bool(i & 1))))
    return out


@pytest.fixture(scope="module")
def wanted():
    """The generator's cases and the restatement's answers per (chunk, chunk count): computed once, shared, left unchanged."""
    memo = {}

    def get(chunk, n_chunks):
        if (chunk, n_chunks) not in memo:
            cases = rc.make_cases(chunk, n_chunks)
            flat = sorted(((f, c) for f, cs in cases.items() for c in cs), key=lambda fc: fc[1]["n_pods"])      # (one publish per pod count)
            memo[(chunk, n_chunks)] = [(f, c, rc.WANT[f](c)) for f, c in flat]
        return memo[(chunk, n_chunks)]

    return get


def _run_all(pkg, pk, chunk, todo):
    failed, ran = [], 0
    for i, (family, c, want) in enumerate(todo):
        failed += rc.violations(family, c, chunk, want)
        for form, case in _forms(family, c, i):
            d = _diff(form, case, chunk, _resolve(pkg, pk, form, case), want)
            ran += 1
            if d:
                failed.append(d)
    return failed, ran


@pytest.mark.parametrize("geometry,n_chunks", RUNS)
def test_the_resolves_equal_the_restatements_over_many_chunks(pkg, wanted, monkeypatch, geometry, n_chunks):
    _setenv(monkeypatch, GEOMETRIES[geometry])
    with _bare_picker(pkg, geometry) as pk:
        chunk = pk.bounded_geometry()[0]
        todo = wanted(chunk, n_chunks)
        assert {f for f, _, _ in todo} == {"bounded", "banded", "costed"}
        assert any(-(-c["lists"].shape[0] // chunk) == n_chunks for _, c, _ in todo)
        failed, ran = _run_all(pkg, pk, chunk, todo)
        assert not failed, f"{len(failed)} of {ran} resolves: " + " | ".join(failed[:6])


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_the_cases_that_ran_cover_every_required_branch(wanted, geometry):
    chunk = int(GEOMETRIES[geometry].get("EPPK_BOUND_CHUNK", 512))
    tags = {f: set() for f in ("bounded", "banded", "costed")}
    for n_chunks in COUNTS[geometry]:
        for f, c, _ in wanted(chunk, n_chunks):
            tags[f] |= c["tags"]
    if geometry == "default":
        assert not set(rc.REQUIRED_17_33) - set().union(*tags.values())
    else:
        assert not set(rc.REQUIRED) - set().union(*tags.values())
        for f in tags:
            assert not set(rc.SCAN_TAGS) - tags[f], (f, sorted(set(rc.SCAN_TAGS) - tags[f]))


def test_1025_chunks_of_64_rows_at_full_width(pkg, wanted, monkeypatch):
    """The production batch under the small chunk: 65,545 rows, seg_len 65 and 33, and more chunks than the chunk grid has workgroups."""
    import torch
    _setenv(monkeypatch, GEOMETRIES["chunk64"])
    assert torch.cuda.get_device_properties(0).multi_processor_count * 4 < rc.BIG, "the grid of the per-chunk kernels is capped"
    with _bare_picker(pkg, "chunk64") as pk:
        todo = wanted(64, rc.BIG)
        assert all(c["lists"].shape[0] == 65545 for _, c, _ in todo) and {f for f, _, _ in todo} == {"bounded", "banded", "costed"}
        sizes = [-(-r.size // 64) for r in rc.band_places(next(c for f, c, _ in todo if f == "banded"))]
        # (7 band-chunks: three standard deviations of the draw and one chunk for the rounding up, as tests/test_resolve_chunks_cpu.py works out)
        assert all(abs(s - w) <= 7 for s, w in zip(sizes, rc.BAND_CHUNKS[rc.BIG])), sizes
        failed, ran = _run_all(pkg, pk, 64, todo)
        assert not failed, f"{len(failed)} of {ran} resolves: " + " | ".join(failed[:6])


@pytest.mark.parametrize("family", ["bounded", "banded", "costed"])
def test_the_answer_does_not_depend_on_chunk_size_or_grid(pkg, wanted, monkeypatch, family):
    """One random input per chunk count (that many chunks of 64 rows) under chunks of 64, 128 and 512 rows and under EPPK_MAX_CU=1:
    outputs byte-identical to each other and to the restatement."""
    inputs = []
    for n_chunks in rc.COUNTS:
        f, c, want = next(x for x in wanted(64, n_chunks) if x[0] == family and "random" in x[1]["tags"])
        inputs.append((c, want))
    results = {}
    for geometry, env in GEOMETRIES.items():
        _setenv(monkeypatch, env)
        with _bare_picker(pkg, geometry) as pk:
            results[geometry] = [_resolve(pkg, pk, family, c) for c, _ in inputs]
    first = results["chunk64"]
    for geometry, res in results.items():
        for (c, _), a, b in zip(inputs, first, res):
            for x, y, what in zip(a[:4], b[:4], ("picks", "scores", "ranks", "loads")):
                assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{geometry} against chunk64, {rc.INFO[family](c)}: {what}"
            assert a[4] == b[4]
    for (c, want), got in zip(inputs, first):
        assert not _diff(family, c, 64, got, want)


def test_grown_scratch_is_reused_by_smaller_and_larger_batches(pkg, wanted, monkeypatch):
    """In ONE context: 257 chunks, then 17, then 257 again, the three resolves interleaved -- hist, bh and perm hold rows of the larger
    batch when the smaller one runs, and the other resolves' words when a resolve comes back."""
    _setenv(monkeypatch, GEOMETRIES["chunk64"])
    pick = lambda n, f: next(x for x in wanted(64, n) if x[0] == f and "random" in x[1]["tags"])          # noqa: E731
    order = [(257, "bounded"), (257, "banded"), (257, "costed"), (17, "bounded"), (17, "costed"), (17, "banded"), (257, "bounded"), (257, "costed"),
             (257, "banded"), (17, "banded"), (257, "costed")]
    with _bare_picker(pkg, "chunk64") as pk:
        for step, (n, f) in enumerate(order):
            _, c, want = pick(n, f)
            d = _diff(f, c, 64, _resolve(pkg, pk, f, c), want)
            assert not d, f"step {step} ({n} chunks, {f}): {d}"


# ---- the host-buffer forms: grids sized from the host's counts per band, empty bands skipped ------------------------------------

R_HOST, P_HOST, K_HOST = 35 * 64 - 21, 1000, 4
HOST_TABLE = [(0, 0), (1, 1), (0, 1), (1, 2), (0, 3)]                         # band 2 stays empty


def test_the_host_forms_over_35_chunks(pkg, monkeypatch):
    """pick_bounded, pick_bounded_banded and pick_bounded_costed on one batch of 35 chunks of 64 rows.  The lists are the library's own
    top-k answer for the batch (held to the oracle by tests/test_gpu_pickers.py and the three resolve modules): the resolve is what is
    under test, against the restatement fed those lists."""
    _setenv(monkeypatch, GEOMETRIES["chunk64"])
    wl = pkg.workload.make_workload(3, R=R_HOST, P=P_HOST)
    rng = np.random.default_rng(rc.SEED0)
    band = rng.choice([0, 1, 3, 4], size=R_HOST, p=[0.2, 0.4, 0.25, 0.15]).astype(np.uint8)
    cost = rng.integers(1, 9, size=R_HOST).astype(np.uint32)
    load0 = rng.integers(0, 2, size=P_HOST).astype(np.uint32)
    with pkg.BatchedPicker(wl.chain, max_pods=1024, max_blocks=wl.B, max_batch=R_HOST, index_slots=wl.index_slots) as pk:
        assert pk.bounded_geometry()[0] == 64
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        lp, ls = pk.pick_topk(wl.reqs, K_HOST)
        lp, ls = np.ascontiguousarray(lp, dtype=np.int32), np.ascontiguousarray(ls, dtype=np.float64)

        def same(got, want, what):
            for g, w, name in zip(got, want, ("picks", "scores", "ranks", "loads")):
                assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)), f"{what}: {name}"

        for policy in (rc.SHED, rc.SPILL):
            want = rc.bc.ref.resolve(lp, ls, P_HOST, None, 3, policy, load0)
            assert not want[4] and len(set(want[2][want[2] < K_HOST].tolist())) >= 2 and (want[2] & rc.OVERFLOW).any(), "the cap binds"
            same(pk.pick_bounded(wl.reqs, K_HOST, 3, policy, load0), want[:4], f"pick_bounded policy {policy}")
        banded = dict(lists=lp, bands=HOST_TABLE, band=band)
        want = rc.nc.ref.resolve(lp, ls, P_HOST, HOST_TABLE, band, None, 4, load0)
        trace = rc.band_trace(banded, want)
        assert sorted(trace) == [0, 1, 3, 4] and all(rounds >= 2 and left for rounds, left, _ in trace.values()), f"the caps bind in every band: {trace}"
        same(pk.pick_bounded_banded(wl.reqs, K_HOST, 4, HOST_TABLE, band, load0), want[:4], "pick_bounded_banded")
        table = [(p, 4 * r) for p, r in HOST_TABLE]
        want = rc.cc.ref.resolve(lp, ls, P_HOST, cost, table, band, None, 16, load0 * 4)
        trace = rc.band_trace(banded, want)
        assert want[4] == 0 and all(rounds >= 2 and left for rounds, left, _ in trace.values()), f"the caps bind in every band: {trace}"
        same(pk.pick_bounded_costed(wl.reqs, K_HOST, cost, 16, table, band, load0 * 4), want[:4], "pick_bounded_costed")
