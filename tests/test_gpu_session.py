"""GPU: ONE long-lived context held to the oracle across interleaved calls.

Every other GPU module creates a context, drives one feature through it and throws it away; a scheduler keeps one eppk_ctx alive and
calls everything on it in any order, and the context carries state from call to call: the quad route's back-off and report ring, a
work-list buffer per stream, the set table's rebuild counter, the filter planes and the stream they were built on, the occupancy cache
and the process-wide dynamic-LDS limit, scratch that grows on demand and is shared by the bounded, banded and costed resolves, the
double-buffered snapshot and everything sized by J = ceil(n_pods / 64), the assumed-load switch and the rows it bumps.  Here a seeded
session (tests/session_cases.py: publishes that change J, index updates, every picker, the filter, the three load resolves in their
nine forms, refusals) runs on one context; after EVERY step the outputs equal the reference model's byte for byte and the launch status
is 0.  No step is skipped or filtered here.  The CPU twin (tests/test_session_cpu.py) holds the generator to its coverage.

The module sets the library switches it needs itself (monkeypatch) before it creates a context."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = {"default": {}, "quadmin4": {"EPPK_QUAD_MIN": "4"},
            "quadmin4-chunk64-cu1": {"EPPK_QUAD_MIN": "4", "EPPK_BOUND_CHUNK": "64", "EPPK_MAX_CU": "1"},
            "lists0-chunk64": {"EPPK_LISTS": "0", "EPPK_BOUND_CHUNK": "64"}}
KNOBS = ("EPPK_QUAD_MIN", "EPPK_QUAD", "EPPK_BOUND_CHUNK", "EPPK_MAX_CU", "EPPK_LISTS", "EPPK_RESIDENT", "EPPK_MAX_WG_PER_CU")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


sc = _load("session_cases")


def _setenv(monkeypatch, env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _dev(torch, a):
    """A numpy array on the device (unsigned words travel as the signed type of their width); None stays None."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    a = a.view({np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype, a.dtype))
    return torch.from_numpy(a.copy()).to(torch.device("cuda", 0))


def _ptr(t):
    return None if t is None else t.data_ptr()


def _same(got, want, what):
    """'' when got equals want byte for byte, else what differs."""
    if want is None:
        return "" if got is None else f"{what}: something where nothing is due"
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if np.ndim(want) == 0 or np.ndim(got) == 0:
        return "" if int(got) == int(want) else f"{what}: gpu {int(got)} want {int(want)}"
    if got.shape != want.shape or got.dtype.itemsize != want.dtype.itemsize:
        return f"{what}: shape {got.shape} / {got.dtype}, want {want.shape} / {want.dtype}"
    if got.tobytes() == want.tobytes():
        return ""
    rows = np.nonzero(np.any((got.view(np.uint8) != want.view(np.uint8)).reshape(got.shape[0], -1), axis=1))[0]
    return f"{what}: {rows.size} rows differ, first {rows[:4]}: gpu {got[rows[:2]]!r} want {want[rows[:2]]!r}"


class Session:
    """One context and the streams, driven step by step."""

    def __init__(self, pkg, cfg):
        import torch
        self.torch, self.pkg = torch, pkg
        self.dev = torch.device("cuda", 0)
        self.pk = pkg.BatchedPicker(cfg["chain"], max_pods=cfg["max_pods"], max_blocks=cfg["max_blocks"], max_batch=cfg["max_batch"],
                                    index_slots=cfg["index_slots"])
        self.streams = [torch.cuda.Stream(device=self.dev) for _ in range(3)]
        self.cfg = cfg

    def close(self):
        self.torch.cuda.synchronize(self.dev)
        self.pk.close()

    def stream(self, s):
        return self.streams[s.get("stream", 0)].cuda_stream

    def sync(self):
        self.torch.cuda.synchronize(self.dev)

    def outs(self, R, k=None):
        t = self.torch
        shape = (R,) if k is None else (R, k)
        return (t.full(shape, 0x5A5A5A5A, dtype=t.int32, device=self.dev), t.full(shape, 7.25, dtype=t.float64, device=self.dev),
                t.full((R,), 0x5A, dtype=t.uint8, device=self.dev))

    # -- a step: what the library answers, under the keys of the model's answer -------------------------------------------------------
    def run(self, s, inp):
        pk, op, t = self.pk, s["op"], self.torch
        J = (pk.n_pods + 63) // 64
        if op == "publish":
            self.sync()
            pk.publish(inp["pods"])
            return dict(size=pk.index_size())
        if op in ("seed_index", "insert", "clear"):
            if op == "clear":
                pk.index_clear()
            pk.index_insert(inp["hashes"], inp["pods"])
            return dict(size=pk.index_size())
        if op == "insert_picks_device":
            d_reqs, d_picks = _dev(t, inp["reqs"]), _dev(t, inp["picks"])
            self.sync()
            pk.index_insert_picks_device(d_reqs.data_ptr(), d_picks.data_ptr(), inp["reqs"].shape[0], self.stream(s))
            self.sync()
            return dict(size=pk.index_size())
        if op == "remove_pod":
            pk.index_remove_pod(s["pod"])
            return dict(size=pk.index_size())
        if op == "tick_evict":
            e = pk.index_advance_epoch()
            pk.index_insert(inp["hashes"], inp["pods"])
            n = pk.index_evict_older(inp["min_epoch"])
            return dict(epoch=e, evicted=n, size=pk.index_size())
        if op == "trim":
            n = pk.index_trim_pods(inp["cap"])
            return dict(removed=n, size=pk.index_size())
        if op == "set_assumed_load":
            self.sync()
            pk.set_assumed_load(s["E"])
            return dict()
        if op in ("pick", "pick_masked"):
            p, sc_ = pk.pick(inp["reqs"], inp["mask"])
            return dict(picks=p, scores=sc_)
        if op == "pick_device":
            R = inp["reqs"].shape[0]
            d_reqs, d_mask = _dev(t, inp["reqs"]), _dev(t, inp["mask"])
            d_pick, d_score, _ = self.outs(R)
            self.sync()
            pk.pick_device(d_reqs.data_ptr(), R, _ptr(d_mask), d_pick.data_ptr(), d_score.data_ptr(), self.stream(s))
            self.sync()
            return dict(picks=d_pick.cpu().numpy(), scores=d_score.cpu().numpy())
        if op == "pick_staged":
            R = inp["reqs"].shape[0]
            st_reqs, _ = pk.staging()
            st_reqs[:R] = inp["reqs"]
            p, sc_ = pk.pick_staged(R)
            return dict(picks=p, scores=sc_)
        if op in ("pick_topk", "pick_topk_masked"):
            p, sc_ = pk.pick_topk(inp["reqs"], s["k"], inp["mask"])
            return dict(picks=p, scores=sc_)
        if op == "pick_candidates":
            p, sc_ = pk.pick_candidates(inp["reqs"], inp["mask"], s["k"])
            return dict(picks=p, scores=sc_)
        if op == "learn_then_pick":
            R = inp["reqs"].shape[0]
            d_reqs = _dev(t, inp["reqs"])
            d_pick, d_score, _ = self.outs(R)
            self.sync()
            pk.pick_learn_device(d_reqs.data_ptr(), R, None, d_pick.data_ptr(), d_score.data_ptr(), self.stream(s))
            self.sync()
            p2, s2 = pk.pick(inp["reqs"])
            return dict(picks=d_pick.cpu().numpy(), scores=d_score.cpu().numpy(), picks2=p2, scores2=s2, size=pk.index_size())
        if op == "stage_pair":
            R = inp["reqs"].shape[0]
            a, _ = pk.stage_buffers(0)
            b, mb = pk.stage_buffers(1, with_mask=True)
            a[:R] = inp["reqs"]
            b[:R] = inp["reqs2"]
            mb[:R * J].reshape(R, J)[:] = inp["mask2"]
            pk.stage_begin(0, R, learn=True)
            pk.stage_begin(1, R, use_mask=True)
            p0, s0 = pk.stage_end(0)
            p1, s1 = pk.stage_end(1)
            return dict(picks=p0, scores=s0, picks2=p1, scores2=s1, size=pk.index_size())
        if op in ("random_topk", "random_topk_masked"):
            p, sc_ = pk.pick_random_topk(inp["reqs"], s["k"], s["seed"], inp["mask"])
            return dict(picks=p, scores=sc_)
        if op in ("weighted_random", "weighted_random_masked"):
            p, sc_ = pk.pick_weighted_random(inp["reqs"], s["seed"], s["k"], inp["mask"])
            return dict(picks=p, scores=sc_)
        if op in ("set_filters", "set_filters_none", "too_many_programs"):
            pk.set_filters(inp["programs"])
            return dict()
        if op in ("filter_masks", "bad_class"):
            m, v = pk.filter_masks(inp["reqs"], inp.get("cls"), inp.get("mask"))
            return dict(masks=m, verdict=v)
        if op == "filter_masks_device":
            R = inp["reqs"].shape[0]
            d_reqs, d_cls, d_mask = _dev(t, inp["reqs"]), _dev(t, inp["cls"]), _dev(t, inp["mask"])      # the mask rows are filtered in place
            d_verdict = t.full((R,), 0x5A, dtype=t.uint8, device=self.dev)
            self.sync()
            pk.filter_masks_device(d_reqs.data_ptr(), R, _ptr(d_cls), d_mask.data_ptr(), d_mask.data_ptr(), d_verdict.data_ptr(), self.stream(s))
            self.sync()
            return dict(masks=d_mask.cpu().numpy().view(np.uint64), verdict=d_verdict.cpu().numpy())
        if op == "pick_filtered":
            p, sc_, v = pk.pick_filtered(inp["reqs"], s["k"], inp["cls"], inp["mask"])
            return dict(picks=p, scores=sc_, verdict=v)
        if op in sc.RESOLVE_OPS:
            return self.resolve(s, inp)
        if op == "bad_policy":
            return pk.pick_bounded(inp["reqs"], 2, 3, policy=7)
        if op == "bad_reserves":
            return pk.pick_bounded_banded(inp["reqs"], 2, 3, inp["bands"])
        if op == "bad_band":
            return pk.pick_bounded_costed(inp["reqs"], 2, inp["cost"], 3, inp["bands"], inp["band"])
        if op == "bad_row":
            return pk.pick(inp["reqs"])
        if op == "end_without_begin":
            return pk.stage_end(0)                             # (set 0 is idle: every stage_begin of the session has had its stage_end)
        raise ValueError(op)

    def resolve(self, s, inp):
        pk, op, t = self.pk, s["op"], self.torch
        kind, k, R = inp["kind"], inp["k"], inp["R"]
        cap = inp["cap"] if inp["cap"] is not None else inp["cap_all"]
        if op in ("pick_bounded", "pick_banded", "pick_costed"):
            if kind == "bounded":
                got = pk.pick_bounded(inp["reqs"], k, cap, inp["policy"], inp["load"], inp["mask"])
            elif kind == "banded":
                got = pk.pick_bounded_banded(inp["reqs"], k, cap, inp["bands"], inp["band"], inp["load"], inp["mask"])
            else:
                got = pk.pick_bounded_costed(inp["reqs"], k, inp["cost"], cap, inp["bands"], inp["band"], inp["load"], inp["mask"])
            return dict(picks=got[0], scores=got[1], ranks=got[2], load=got[3])
        d_cap, d_load, d_band, d_cost = _dev(t, inp["cap"]), _dev(t, inp["load"]), _dev(t, inp["band"]), _dev(t, inp["cost"])
        d_pick, d_score, d_rank = self.outs(R)
        st = self.stream(s)
        if op.startswith("resolve_"):
            d_lists, d_ls = _dev(t, inp["lists"]), _dev(t, inp["list_scores"])
            self.sync()
            if kind == "bounded":
                pk.bounded_resolve_device(d_lists.data_ptr(), d_ls.data_ptr(), R, k, _ptr(d_cap), inp["cap_all"], inp["policy"], _ptr(d_load), d_pick.data_ptr(),
                                          d_score.data_ptr(), d_rank.data_ptr(), st)
            elif kind == "banded":
                pk.bounded_resolve_banded_device(d_lists.data_ptr(), d_ls.data_ptr(), R, k, _ptr(d_band), inp["bands"], _ptr(d_cap), inp["cap_all"], _ptr(d_load),
                                                 d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr(), st)
            else:
                pk.bounded_resolve_costed_device(d_lists.data_ptr(), d_ls.data_ptr(), R, k, d_cost.data_ptr(), sc.PER_ENTRY if inp["per_entry"] else 0, _ptr(d_band),
                                                 inp["bands"], _ptr(d_cap), inp["cap_all"], _ptr(d_load), d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr(), st)
        else:
            d_reqs, d_mask = _dev(t, inp["reqs"]), _dev(t, inp["mask"])
            self.sync()
            if kind == "bounded":
                pk.pick_bounded_device(d_reqs.data_ptr(), R, _ptr(d_mask), k, _ptr(d_cap), inp["cap_all"], inp["policy"], _ptr(d_load), d_pick.data_ptr(),
                                       d_score.data_ptr(), d_rank.data_ptr(), st)
            elif kind == "banded":
                pk.pick_bounded_banded_device(d_reqs.data_ptr(), R, _ptr(d_mask), k, _ptr(d_band), inp["bands"], _ptr(d_cap), inp["cap_all"], _ptr(d_load),
                                              d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr(), st)
            else:
                pk.pick_bounded_costed_device(d_reqs.data_ptr(), R, _ptr(d_mask), k, d_cost.data_ptr(), _ptr(d_band), inp["bands"], _ptr(d_cap), inp["cap_all"],
                                              _ptr(d_load), d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr(), st)
        self.sync()
        return dict(picks=d_pick.cpu().numpy(), scores=d_score.cpu().numpy(), ranks=d_rank.cpu().numpy(),
                    load=None if d_load is None else d_load.cpu().numpy().view(np.uint32))


def _scores_as_bits(d):
    return {k: (np.ascontiguousarray(v).view(np.uint64) if k.startswith("scores") else v) for k, v in d.items()}


def run_session(pkg, orc, seed, env, steps=None, checks=True):
    """Session `seed` (or the step list given) on one context against the model; returns what was observed on the way.  Fails at the
    first step whose answer differs, naming seed, step, operation, arguments and the operations before it."""
    steps = sc.make_session(seed) if steps is None else steps
    model = sc.Model(seed, orc, pkg.workload)
    cfg = sc.config(seed)
    chunk = int(env.get("EPPK_BOUND_CHUNK", 512))
    quad = env.get("EPPK_QUAD_MIN") == "4" and env.get("EPPK_LISTS") != "0"
    seen = dict(sides=set(), quad=[], ran=0)
    ses = Session(pkg, cfg)
    try:
        pk = ses.pk
        assert pk.bounded_geometry() == (chunk, chunk)
        for s in steps:
            at = sc.where(seed, steps, s["i"]) if "i" in s else f"session seed {seed}: {sc.describe(s)}"
            try:
                inp, want = model.apply(s)
            except sc.Refused as e:
                inp, want = e.args[0], None
            q0 = pk.quad_stats() if quad and s.get("quad") else None
            if want is None:
                with pytest.raises(pkg.EppkError):
                    ses.run(s, inp)
                    pytest.fail(f"{at}: not refused")
            else:
                got = ses.run(s, inp)
                assert sorted(got) == sorted(want), at
                bad = [m for m in (_same(g, w, key) for (key, g), (_, w) in zip(sorted(_scores_as_bits(got).items()), sorted(_scores_as_bits(want).items()))) if m]
                assert not bad, f"{at}: " + "; ".join(bad)
            assert pk.launch_status() == 0, f"{at}: launch status"
            seen["ran"] += 1
            if not checks:
                continue
            if s["fam"] in ("index", "snapshot") or "size" in (want or {}):
                assert pk.index_size() == model.oix.size() and pk.index_selfcheck() == 0, f"{at}: index size / selfcheck"
            if s["op"] in sc.RESOLVE_OPS and want is not None:
                assert pk.bounded_geometry() == (chunk, chunk), f"{at}: the resolve's geometry moved"      # (one launch takes `chunk` rows, as at the start)
                seen["sides"].add(inp["R"] <= pk.bounded_geometry()[1])
            if q0 is not None:
                q1 = pk.quad_stats()
                seen["quad"].append((s["quad"], q1[0] - q0[0], q1[1] - q0[1], s["R"]))
            if env.get("EPPK_MAX_CU") == "1" and want is not None:
                g = pk.launch_geometry()
                if s["op"].startswith("weighted"):
                    assert g == (0, 0, 1, 1024), f"{at}: weighted-random geometry {g} under EPPK_MAX_CU=1"
                elif s["op"] == "pick_candidates":
                    assert g == (0, 0, min(-(-s["R"] // 4), 8), 256), f"{at}: candidates geometry {g} under EPPK_MAX_CU=1"
                elif s["op"] in ("pick", "pick_masked", "pick_topk", "random_topk") and s["R"] >= 256:
                    assert 1 <= max(g[0], g[2]) <= 8, f"{at}: a grid of {g} workgroups on one CU"
        assert pk.index_size() == model.oix.size() and pk.index_selfcheck() == 0 and pk.index_dropped() == 0
        seen["resident"] = pk.resident_stats()
    finally:
        ses.close()
    return seen


@pytest.mark.parametrize("seed", sc.SEEDS)
@pytest.mark.parametrize("switches", list(SWITCHES))
def test_session(pkg, orc, monkeypatch, switches, seed):
    env = SWITCHES[switches]
    _setenv(monkeypatch, env)
    seen = run_session(pkg, orc, seed, env)
    assert seen["ran"] == len(sc.make_session(seed))
    assert seen["sides"] == {True, False}, "batches on both sides of one launch of the bounded resolve"
    if env.get("EPPK_QUAD_MIN") == "4" and env.get("EPPK_LISTS") != "0":
        _check_quad(seen["quad"])
    else:
        assert seen["quad"] == []


def _check_quad(quad):
    """The route taken, then not taken on an eligible batch behind one that deferred above its pause threshold: n/4 of an unmasked batch,
    n/8 of a masked one (a share between the two leaves the route on behind the unmasked batch)."""
    by = {kind: (launches, deferred, n) for kind, launches, deferred, n in quad}
    l, d, n = by["eligible"]
    assert l == 1 and d <= n // 4, f"the quad route takes an eligible batch: {quad}"
    if "heavy" in by:
        assert [q[0] for q in quad] == ["eligible", "heavy", "after"]
        l, d, n = by["heavy"]
        assert l == 1 and d > n // 4, f"... and the heavily deferring one, which it defers: {quad}"
    else:
        assert [q[0] for q in quad] == ["eligible", "moderate", "heavy_masked", "after"]
        l, d, n = by["moderate"]
        assert l == 1 and n // 8 < d <= n // 4, f"... and an unmasked batch that defers less than a quarter: {quad}"
        l, d, n = by["heavy_masked"]
        assert l == 1 and d > n // 8, f"... is still on for the masked batch behind it, which defers more than an eighth: {quad}"
    assert by["after"][:2] == (0, 0), f"... and is paused for the eligible batch behind it: {quad}"


def test_session_at_4096_pods(pkg, orc, monkeypatch):
    """max_pods 4096 / max_blocks 32: the u64 lane word and another LDS footprint."""
    _setenv(monkeypatch, SWITCHES["quadmin4"])
    seen = run_session(pkg, orc, sc.BIG_SEED, SWITCHES["quadmin4"])
    assert seen["ran"] == len(sc.make_session(sc.BIG_SEED))
    _check_quad(seen["quad"])


@pytest.mark.timeout(120)
def test_session_with_resident_units(pkg, orc, monkeypatch):
    """EPPK_RESIDENT=1: the small unmasked batches of the session ring the resident units between launched calls."""
    env = {"EPPK_RESIDENT": "1"}
    _setenv(monkeypatch, env)
    steps = sc.make_session(sc.SEEDS[0])
    small = sum(1 for s in steps if s["op"] in ("pick", "pick_topk", "pick_staged") and s["R"] <= 32 and not s.get("assumed"))
    assert small >= 2
    seen = run_session(pkg, orc, sc.SEEDS[0], env)
    on, batches, starts = seen["resident"]
    assert on and batches >= 1 and starts >= 1, seen["resident"]


def test_two_contexts_share_a_process(pkg, orc, monkeypatch):
    """A (max_pods 4096, max_blocks 32) and B (max_pods 64, max_blocks 4) alive together, each created first once: masked and unmasked
    picks, a filter call and a bounded call alternate between them, one is destroyed midway and the other goes on.  Each is held to its
    own model: what this crosses is the process-wide dynamic-LDS limit and the occupancy caches."""
    _setenv(monkeypatch, {})
    shapes = {"A": dict(max_pods=4096, max_blocks=32, P=4096, groups=64), "B": dict(max_pods=64, max_blocks=4, P=64, groups=64)}

    def make(name, seed):
        c = shapes[name]
        cfg = dict(sc.config(seed), max_pods=c["max_pods"], max_blocks=c["max_blocks"], groups=c["groups"], index_slots=4096, pods=(c["P"],))
        m = sc.Model(seed, orc, pkg.workload)
        m.cfg, m.pool, m.B = cfg, sc.Pool(cfg), cfg["max_blocks"]
        ses = Session(pkg, cfg)
        return m, ses

    def step(name, m, ses, s, tag):
        inp, want = m.apply(s)
        got = ses.run(s, inp)
        bad = [x for x in (_same(g, w, key) for (key, g), (_, w) in zip(sorted(_scores_as_bits(got).items()), sorted(_scores_as_bits(want).items()))) if x]
        assert not bad, f"{tag}, context {name}: {sc.describe(s)}: " + "; ".join(bad)
        assert ses.pk.launch_status() == 0, f"{tag}, context {name}: {sc.describe(s)}"

    def rounds(i):
        base = dict(seed=900 + i, stream=i % 3, assumed=0)
        return [dict(base, fam="picks", op="pick", R=256), dict(base, fam="picks", op="pick_masked", R=65),
                dict(base, fam="filter", op="filter_masks", R=64, masked=True, k=1, local=True, case=0),
                dict(base, fam="resolve", op="pick_bounded", R=700, k=4, policy=sc.SHED, cap_array=False, load="fresh", bands=((sc.SHED, 0),), masked=False,
                     per_entry=False, refused=False),
                dict(base, fam="picks", op="pick_topk", R=5, k=8)]

    for order in ("AB", "BA"):
        live = {}
        try:
            for j, name in enumerate(order):
                live[name] = make(name, 8000 + j)
            for name, (m, ses) in live.items():
                P = shapes[name]["P"]
                step(name, m, ses, dict(fam="snapshot", op="publish", seed=5 + P, P=P, kind="workload", holes=False, qmode="a", kvmode="a"), order)
                step(name, m, ses, dict(fam="index", op="seed_index", seed=1, call=0, of=1), order)
                step(name, m, ses, dict(fam="filter", op="set_filters", seed=1, local=True, case=0), order)
            for i in range(2):
                for s in rounds(i):
                    for name in order:                             # the same operation on one context, then on the other
                        step(name, *live[name], s, f"{order} round {i}")
            gone = order[0]
            live.pop(gone)[1].close()                              # one context goes; the other carries on
            for s in rounds(2):
                step(order[1], *live[order[1]], s, f"{order} after {gone} was destroyed")
        finally:
            for _, ses in live.values():
                ses.close()
