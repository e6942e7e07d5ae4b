"""GPU: fair shares between flows in cost units, the rows sorted by carried service (SEMANTICS.md §3i; include/eppk.h
eppk_sfair_resolve_device / eppk_pick_sfair) against the numpy restatement (tests/sfair_ref.py), exactly: picks, ranks, loads, service,
scores as bit patterns, and the sticky launch status.  The module sets the library switches itself (monkeypatch) before it creates a
context."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GEOMETRIES = {"chunk64": {"EPPK_BOUND_CHUNK": "64"}, "default": {}, "chunk64-cu1": {"EPPK_BOUND_CHUNK": "64", "EPPK_MAX_CU": "1"}}
NAMES = ("picks", "scores", "ranks", "loads", "launch status", "service")
_spec = importlib.util.spec_from_file_location("sfair_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "sfair_ref.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)
TOP, SHED, SPILL = ref.TOP, ref.SHED, ref.SPILL

# (name, rows, flows, bands, k, pods, top weight, service below, top cost): what each is the smallest shape to reach is in its test
SHAPES = {"two-trips": (65, 3, 1, 2, 8, 3, 40, 64), "contended": (300, 16, 2, 3, 16, 16, 1 << 20, 8192), "129-chunks": (129 * 64, 1024, 8, 2, 64, 4, 64, 512),
          "five-digits": (200, 2, 1, 2, 8, 65535, TOP, (1 << 24) - 1), "bad-rows": (150, 5, 2, 2, 8, 3, 40, 64)}


def _case(name, seed=0, **over):
    """The inputs of one resolve, built from the shape's tuple and a seed; `over` replaces fields (None: the NULL form)."""
    R, nf, nb, k, P, wtop, stop, ctop = SHAPES[name]
    rng = np.random.default_rng(0x5FA1 + seed)
    lists = rng.integers(0, P, size=(R, k)).astype(np.int32)
    lists[rng.random((R, k)) < 0.1] = ref.NO_PICK
    cost = np.clip(np.floor((rng.pareto(1.1, size=R) + 1.0) * 2.0), 1, ctop).astype(np.uint32)
    c = dict(name=name, lists=lists, scores=rng.standard_normal((R, k)), n_pods=P, flow=rng.integers(0, nf, size=R).astype(np.uint16), n_flows=nf,
             weight=rng.integers(1, wtop + 1, size=nf).astype(np.uint16), service=rng.integers(0, stop, size=(nb, nf)).astype(np.uint32), cost=cost,
             bands=[(SHED if b % 2 == 0 else SPILL, 4 * b) for b in range(nb)], band=rng.integers(0, nb, size=R).astype(np.uint8), cap=None,
             cap_all=int(cost.sum()) // (2 * P), load=rng.integers(0, 3, size=P).astype(np.uint32), no_score=False, no_rank=False)
    if name == "contended":
        c["cap_all"] = 12 * int(np.median(cost))
    if name == "129-chunks":                                                  # flow 5 of band 0 has a row in every chunk, at a lane that moves
        at = np.arange(129) * 64 + (np.arange(129) * 5) % 64
        c["flow"][at], c["band"][at] = 5, 0
    if name == "five-digits":
        c["service"], c["weight"] = np.array([[TOP, 0]], dtype=np.uint32), np.array([1, 65535], dtype=np.uint16)
        c["cost"] = rng.choice(np.array([1, (1 << 24) - 1], dtype=np.uint32), size=R)
        c["cap_all"] = 6 << 24
    if name == "bad-rows":                                                    # every kind of row that is out of the order or charges nothing
        c["weight"][2] = 0
        c["band"][::11], c["flow"][3::13], c["cost"][5::7], c["cost"][6::17] = nb, nf, 0, ref.MAX_COST + 1
    return dict(c, **over)


def want(c):
    return ref.resolve(c["lists"], c["scores"], c["n_pods"], c["flow"], c["n_flows"], c["weight"], c["service"], c["cost"], c["bands"], c["band"], c["cap"],
                       c["cap_all"], c["load"])


def _setenv(monkeypatch, geometry):
    for name in ("EPPK_BOUND_CHUNK", "EPPK_MAX_CU"):
        monkeypatch.delenv(name, raising=False)
    for name, value in GEOMETRIES[geometry].items():
        monkeypatch.setenv(name, value)


def _bare_picker(pkg):
    """A context for the resolve alone: the lists come from the test, the snapshot only says how many pods there are."""
    return pkg.BatchedPicker([(1, 1)], max_pods=4096, max_blocks=0, max_batch=64)


def _dev(torch, a):
    a = np.ascontiguousarray(a)
    for u, s in ((np.uint16, np.int16), (np.uint32, np.int32), (np.uint64, np.int64)):
        if a.dtype == u:
            a = a.view(s)
    return torch.from_numpy(a.copy()).to(torch.device("cuda", 0))


def _resolve(pkg, pk, c, via="sfair", d_table=None, d_load=None):
    """One case through eppk_sfair_resolve_device ("wfair" / "costed": the same inputs through those): (pick, score | None, rank | None,
    load_out | None, launch-status flags, table_out | None).  d_table / d_load: tensors that stay on the device, in place of the case's own."""
    import torch
    dev = torch.device("cuda", 0)
    R, k = c["lists"].shape
    if pk.n_pods != c["n_pods"]:
        torch.cuda.synchronize(dev)
        pk.publish(np.zeros(c["n_pods"], dtype=pkg.picker.POD_DTYPE))
    d = {n: None if c[n] is None else _dev(torch, c[n]) for n in ("lists", "scores", "band", "flow", "cost", "cap", "load", "weight", "service")}
    d_load = d["load"] if d_load is None else d_load
    d_table = d["service"] if d_table is None else d_table
    d_pick = torch.full((R,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_score = None if c["no_score"] else torch.full((R,), 7.25, dtype=torch.float64, device=dev)
    d_rank = None if c["no_rank"] else torch.full((R,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    ptr = lambda t: t.data_ptr() if t is not None else None                  # noqa: E731
    tail = (ptr(d["band"]), c["bands"], ptr(d["cap"]), c["cap_all"], ptr(d_load), d_pick.data_ptr(), ptr(d_score), ptr(d_rank))
    if via == "costed":
        pk.bounded_resolve_costed_device(ptr(d["lists"]), ptr(d["scores"]), R, k, ptr(d["cost"]), 0, *tail)
    else:
        call = pk.bounded_resolve_sfair_device if via == "sfair" else pk.bounded_resolve_wfair_device
        call(ptr(d["lists"]), ptr(d["scores"]), R, k, ptr(d["flow"]), c["n_flows"], ptr(d["weight"]), ptr(d_table), ptr(d["cost"]), 0, *tail)
    flags = pk.launch_status()                                               # (synchronises)
    out = lambda t, dt: None if t is None else t.cpu().numpy().view(dt)      # noqa: E731
    table = None if via == "costed" or d_table is None else out(d_table, np.uint32).reshape(len(c["bands"]), c["n_flows"])
    return out(d_pick, np.int32), out(d_score, np.float64), out(d_rank, np.uint8), out(d_load, np.uint32), flags, table


def _same(got, wanted, what, upto=6):
    for x, y, name in list(zip(got, wanted, NAMES))[:upto]:
        if name == "launch status":
            assert x == y, f"{what}: launch status {x}, want {y}"
        else:
            assert name != "service" or (x is None) == (y is None), f"{what}: service"
            if x is not None and y is not None:                               # (a NULL out_score / out_rank / load has nothing to compare)
                diff = np.nonzero(np.asarray(x).ravel().view(np.uint8) != np.asarray(y).ravel().view(np.uint8))[0]
                assert diff.size == 0, f"{what}: {name} differ, first at byte {diff[:1]}"


NULLS = [dict(weight=None), dict(service=None), dict(cost=None), dict(band=None, bands=[(SHED, 0)], service=np.zeros((1, 16), dtype=np.uint32)), dict(scores=None),
         dict(no_score=True), dict(no_rank=True), dict(load=None)]
# (129 chunks of 64 rows exist under EPPK_BOUND_CHUNK=64 alone)
RESOLVES = [(g, n, o) for g in GEOMETRIES for n, o in [(n, {}) for n in SHAPES] + [("contended", o) for o in NULLS] if (g, n) != ("default", "129-chunks")]


@pytest.mark.parametrize("geometry,name,over", RESOLVES, ids=[f"{g}-{n}" + "".join("-" + x for x in o) for g, n, o in RESOLVES])
def test_the_resolve_equals_the_restatement(pkg, monkeypatch, geometry, name, over):
    """two-trips: the second trip of a chunk and under chunk64 the second chunk, the carried charge sum across both.  contended: caps that
    bind in two bands.  129-chunks: past one chunk per segment of both offsets scans and past their trips of eight.  five-digits: tags
    2^32 apart and costs of 1 and 2^24 - 1 mixed, so the four digits below the band's each decide (the fifth is the band's at this size:
    contended and 129-chunks decide it).  bad-rows: rows out of the order and rows that charge nothing."""
    c = _case(name, **over)
    w = want(c)
    if name in ("contended", "five-digits") and not over:
        placed = np.count_nonzero(w[2] < c["lists"].shape[1]) / w[2].size
        assert 0.25 <= placed <= 0.75, f"the caps bind: {placed:.2f} of the rows are placed"
    if name == "bad-rows":
        assert w[4] == ref.LAUNCH_BAD_REQUEST_ROW
    _setenv(monkeypatch, geometry)
    with _bare_picker(pkg) as pk:
        assert "EPPK_BOUND_CHUNK" not in GEOMETRIES[geometry] or pk.bounded_geometry()[0] == 64
        _same(_resolve(pkg, pk, c), w, f"{geometry} {name} {sorted(over)}")


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_the_identities_device_against_device(pkg, monkeypatch, geometry):
    """§3i: every cost 1 and no costs are eppk_wfair_resolve_device, the table included; one flow without weights and service is
    eppk_costed_resolve_device; service moved by m * weight per band changes no answer and nothing of what is taken."""
    _setenv(monkeypatch, geometry)
    c = _case("contended")
    with _bare_picker(pkg) as pk:
        for cost in (np.ones(300, dtype=np.uint32), None):
            unit = dict(c, cost=cost, cap_all=5)
            _same(_resolve(pkg, pk, unit), _resolve(pkg, pk, unit, via="wfair"), f"cost {cost is not None} against the wfair resolve")
        one = dict(c, n_flows=1, flow=None, weight=None, service=None)
        _same(_resolve(pkg, pk, one), _resolve(pkg, pk, one, via="costed"), "one flow against the costed resolve")
        m = np.array([[7], [1000]], dtype=np.int64)
        base, moved = _resolve(pkg, pk, c), _resolve(pkg, pk, dict(c, service=(c["service"] + m * c["weight"].astype(np.int64)).astype(np.uint32)))
        _same(moved, base, "service moved by whole tags", upto=5)
        assert np.array_equal(moved[5].astype(np.int64) - m * c["weight"], base[5].astype(np.int64)) and not np.array_equal(base[5], c["service"])


def test_four_carried_batches_on_one_context(pkg, monkeypatch):
    """d_service and d_load stay on the device between the calls; a wfair and a costed resolve in between share the scratch."""
    import torch
    _setenv(monkeypatch, "chunk64")
    service, load = np.zeros((2, 16), dtype=np.uint32), np.zeros(16, dtype=np.uint32)
    with _bare_picker(pkg) as pk:
        d_service, d_load = _dev(torch, service), _dev(torch, load)
        for step, via in enumerate(("sfair", "sfair", "wfair", "sfair", "costed", "sfair")):
            c = _case("contended" if step % 2 else "two-trips", seed=step, n_pods=16, n_flows=16, bands=[(SHED, 0), (SPILL, 4)], service=service, load=load)
            c["weight"], c["cap_all"] = _case("contended")["weight"], int(load.max()) + 6 * int(np.median(c["cost"]))
            if via == "sfair":
                w = want(c)
                _same(_resolve(pkg, pk, c, d_table=d_service, d_load=d_load), w, f"step {step}")
                assert not np.array_equal(w[5], service), "the service moves"
                service, load = w[5], w[3]
            else:
                load = _resolve(pkg, pk, dict(c, service=None), via=via, d_load=d_load)[3]
        assert np.array_equal(d_service.cpu().numpy().view(np.uint32).reshape(2, 16), service), "a wfair or costed call leaves the service alone"


def test_the_pickers_end_to_end(pkg, orc, monkeypatch):
    """eppk_pick_sfair, eppk_pick_sfair_device and the group form on a small snapshot against the oracle's lists through the restatement."""
    import torch
    _setenv(monkeypatch, "chunk64")
    R, P, nf, k = 256, 64, 9, 4
    wl = pkg.workload.make_workload(1, R=R, P=P)
    lp, ls = orc.pick_topk_batch(wl.chain, wl.pods, None, wl.reqs, wl.B, k, threads=8)
    c = _case("contended", n_flows=nf)
    rng = np.random.default_rng(3)
    flow, band, cost, weight = rng.integers(0, nf, size=R).astype(np.uint16), rng.integers(0, 2, size=R).astype(np.uint8), c["cost"][:R], c["weight"][:nf]
    service, load, bands, cap = rng.integers(0, 99, size=(2, nf)).astype(np.uint32), np.zeros(P, dtype=np.uint32), [(SHED, 0), (SPILL, 2)], 24
    w = ref.resolve(lp, ls, P, flow, nf, weight, service, cost, bands, band, None, cap, load)
    assert w[4] == 0 and (w[2] > 7).any() and (w[2] < k).any(), "the caps bind"
    dev = torch.device("cuda", 0)
    with pkg.BatchedPicker(wl.chain, max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots) as pk:
        pk.publish(wl.pods)
        got = pk.pick_sfair(wl.reqs, k, flow, nf, weight, service, cost, cap, bands, band, load)
        _same((got[0], got[1], got[2], got[3], 0, got[4]), w, "pick_sfair")
        d = [_dev(torch, a) for a in (wl.reqs, flow, weight, service, cost, band, load)]
        d_pick, d_score = torch.empty(R, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.float64, device=dev)
        d_rank = torch.empty(R, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        pk.pick_sfair_device(d[0].data_ptr(), R, None, k, d[1].data_ptr(), nf, d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), d[5].data_ptr(), bands, None, cap,
                             d[6].data_ptr(), d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr())
        flags = pk.launch_status()
        _same([t.cpu().numpy() for t in (d_pick, d_score, d_rank, d[6])] + [flags, d[3].cpu().numpy()], w, "pick_sfair_device")
    with pkg.DeviceGroup(wl.chain, [0], max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots, min_shard=1) as g:
        g.publish(wl.pods)
        grp = g.pick_sfair(wl.reqs, k, flow, nf, weight, service, cost, cap, bands, band, load)
        _same((grp[0], grp[1], grp[2], grp[3], 0, grp[4]), w, "group pick_sfair")


def test_argument_errors_launch_and_change_nothing(pkg, monkeypatch):
    _setenv(monkeypatch, "default")
    import torch
    ARG, LIMIT = -1, -2
    dev = torch.device("cuda", 0)
    d_lists, d_cost = torch.zeros((8, 2), dtype=torch.int32, device=dev), _dev(torch, np.ones(8, dtype=np.uint32))
    d_pick, d_service = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device=dev), _dev(torch, np.full((1, 3), 0x1234, dtype=np.uint32))
    ok = [(SHED, 0)]
    with _bare_picker(pkg) as pk:
        pk.publish(np.zeros(4, dtype=pkg.picker.POD_DTYPE))

        def call(n=8, flags=0, n_flows=3, bands=ok):
            pk.bounded_resolve_sfair_device(d_lists.data_ptr(), None, n, 2, None, n_flows, None, d_service.data_ptr(), d_cost.data_ptr(), flags, None, bands, None, 60,
                                            None, d_pick.data_ptr(), None, None)

        for kw, code, word in ((dict(n=pkg._lib.EPPK_SFAIR_MAX_REQS + 1), LIMIT, "n_reqs > 131072"), (dict(flags=1), ARG, "cost flags 1"),
                               (dict(n_flows=0), ARG, "n_flows out of range"), (dict(n_flows=1025), ARG, "n_flows out of range"),
                               (dict(bands=ok * 9), ARG, "n_bands out of range")):
            with pytest.raises(pkg.EppkError) as ei:
                call(**kw)
            assert ei.value.code == code and word in str(ei.value) and "eppk_sfair_resolve_device" in str(ei.value), (kw, str(ei.value))
        pk.set_assumed_load(2)
        with pytest.raises(pkg.EppkError) as ei:
            call()
        assert ei.value.code == ARG and "assumed load" in str(ei.value)
        pk.set_assumed_load(0)
        with pytest.raises(pkg.EppkError) as ei:
            pk.pick_sfair(np.zeros((8, pk.row_words), dtype=np.uint64), 2, np.array([0, 1, 2, 0, 1, 2, 0, 0]), 3, [1, 0, 1], None, None, 6, ok)
        assert ei.value.code == ARG and "row 1" in str(ei.value) and "weight 0" in str(ei.value)
        assert pk.launch_status() == 0
        assert np.all(d_pick.cpu().numpy() == 0x5A5A5A5A) and np.all(d_service.cpu().numpy() == 0x1234), "a refused call writes nothing"
        call()
        assert pk.launch_status() == 0 and np.all(d_pick.cpu().numpy() == 0) and d_service.cpu().numpy().tolist() == [[0x1234 + 8, 0x1234, 0x1234]]
