"""GPU: every buffer of a context that grows on demand, taken small -> large -> small -> larger through the entry point that sizes it.

One long-lived context per case (tests/buffer_growth_cases.py: max_pods 130, published at 130 pods and then at 60, max_blocks 8,
max_batch 64, index_slots 32768, EPPK_QUAD_MIN=4, EPPK_BOUND_CHUNK=64).  The second and the fourth step REPLACE the buffer (the
library parks its resident units and drains the device first), the third reuses it; where the header allows more than one stream the
work of a step is still queued on a second stream when the next call replaces.  Every output equals the reference model's byte for
byte (tests/session_cases.py and the *_ref.py models behind it) and the launch status is 0 after every step.  Each case runs under the
default switches and under EPPK_RESIDENT=1 with a resident pick of 8 requests in front of and behind every step: a unit is running at
the moment of each replacement, and eppk_resident_stats, read on both sides of every replacing step, shows that the unit was parked and
started again.  The load resolves go on for two more steps (200 and 3100 rows): a batch of one chunk asks for no chunk scratch, so the
four steps alone would replace that scratch once; and each of their steps ends with a resolve that takes no ranks, the one call that
sizes the library's own request states.  The CPU twin
(tests/test_buffer_growth_cpu.py) recomputes the capacities, so that this module cannot quietly stop crossing them."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


bg = _load("buffer_growth_cases")
tg = _load("test_gpu_session")
sc = bg.sc
_dev, _ptr = tg._dev, tg._ptr


def _check(got, want, at):
    assert sorted(got) == sorted(want), at
    bad = [m for m in (tg._same(g, w, key) for (key, g), (_, w) in zip(sorted(tg._scores_as_bits(got).items()), sorted(tg._scores_as_bits(want).items()))) if m]
    assert not bad, f"{at}: " + "; ".join(bad)


class Case:
    """One context, its model and two streams."""

    def __init__(self, pkg, orc, cfg=None, seed=bg.SEED):
        self.pkg, self.orc = pkg, orc
        self.m = bg.make_model(orc, pkg.workload, cfg, seed)
        self.ses = tg.Session(pkg, self.m.cfg)
        self.pk, self.t = self.ses.pk, self.ses.torch
        self.endpoints = None

    def close(self):
        self.ses.close()

    def model_step(self, s, at):
        inp, want = self.m.apply(s)
        _check(self.ses.run(s, inp), want, at)
        assert self.pk.launch_status() == 0, f"{at}: launch status"

    def publish(self, P, at):
        self.ses.sync()
        self.model_step(bg.publish_step(P), f"{at}: publish {P}")
        self.endpoints = [self.pkg.picker.Endpoint(f"10.1.{p >> 8}.{p & 255}", str(8000 + p % 3)) for p in range(P)]
        self.pk.set_addresses(self.endpoints)

    def resident_pick(self, i, at):
        s = bg.step("pick", i, R=bg.RESIDENT_ROWS, seed=bg.SEED + 900 + i)
        self.model_step(s, f"{at}: resident pick of {bg.RESIDENT_ROWS}")

    # -- the entry points ------------------------------------------------------------------------------------------------------------------
    def stage(self, op, s, inp, stream):
        """Upload the inputs of a *_device call; returns (go, outs): go() enqueues the call on `stream` WITHOUT waiting, outs are the tensors
        to read once the device is idle.  The caller synchronises once behind its uploads (they are torch's), then calls every go()."""
        pk, t = self.pk, self.t
        R = inp["reqs"].shape[0]
        k = s["k"] if op in ("filtered",) else 1
        d_reqs, d_mask, d_cls = _dev(t, inp["reqs"]), _dev(t, inp.get("mask")), _dev(t, inp.get("cls"))
        d_pick, d_score, d_verdict = self.ses.outs(R, None if k == 1 and op != "filtered" else k)
        keep = (d_reqs, d_mask, d_cls)
        if op == "pick":
            go = lambda: pk.pick_device(d_reqs.data_ptr(), R, _ptr(d_mask), d_pick.data_ptr(), d_score.data_ptr(), stream)
        elif op == "random":
            go = lambda: pk._check(pk._lib.eppk_pick_random_topk_device(pk._ctx, d_reqs.data_ptr(), R, _ptr(d_mask), s["k"], s["seed"], d_pick.data_ptr(), d_score.data_ptr(), stream),
                      "pick_random_topk_device")
        elif op == "learn":
            go = lambda: pk.pick_learn_device(d_reqs.data_ptr(), R, _ptr(d_mask), d_pick.data_ptr(), d_score.data_ptr(), stream)
        elif op == "filtered":
            go = lambda: pk.pick_filtered_device(d_reqs.data_ptr(), R, _ptr(d_cls), _ptr(d_mask), s["k"], d_pick.data_ptr(), d_score.data_ptr(), d_verdict.data_ptr(), stream)
        return (lambda: (go(), keep)[0]), (d_pick, d_score, d_verdict)

    def read(self, outs, verdict=False):
        d = dict(picks=outs[0].cpu().numpy(), scores=outs[1].cpu().numpy())
        if verdict:
            d["verdict"] = outs[2].cpu().numpy()
        return d


def _streams(case):
    return case.ses.streams[0].cuda_stream, case.ses.streams[1].cuda_stream


def run_work_list(case, i, at):
    """An unmasked batch on one stream and a masked one on another, neither waited for: each stream's work list is sized by its own
    batch, and the second call finds the first one's launch still queued."""
    a, b = _streams(case)
    q0 = case.pk.quad_stats()[0]
    su, sm = bg.step("pick", i), bg.step("pick_masked", i)
    iu, wu = case.m.apply(su)
    # (masked, every pod a candidate: the masked kernel and its work list of parked rows, and nothing that makes the route pause itself)
    im = dict(reqs=case.m.rows(sm), mask=sc.vc.mask_words(np.ones((bg.ALL_ROWS[i], case.m.P), dtype=bool)))
    wm = dict(zip(("picks", "scores"), case.m._pick(im["reqs"], im["mask"])))
    go_u, ou = case.stage("pick", su, iu, a)
    go_m, om = case.stage("pick", sm, im, b)
    case.ses.sync()
    go_u()
    go_m()
    case.ses.sync()
    _check(case.read(ou), wu, f"{at}: unmasked on stream 0")
    _check(case.read(om), wm, f"{at}: masked on stream 1")
    assert case.pk.quad_stats()[0] == q0 + 2, f"{at}: both batches took the quad route, whose work list this is"


def run_fallback_lists(case, i, at):
    a, b = _streams(case)
    s0, s1 = bg.step("random_topk", i, stream=0), bg.step("pick", i, seed=bg.SEED + 500 + i)
    i0, w0 = case.m.apply(s0)
    i1, w1 = case.m.apply(s1)
    go1, o1 = case.stage("pick", s1, i1, b)
    go0, o0 = case.stage("random", s0, i0, a)
    case.ses.sync()
    go1()                                                      # a plain pick queued on the other stream while the lists are replaced
    go0()
    case.ses.sync()
    _check(case.read(o0), w0, f"{at}: random-top-{s0['k']}")
    _check(case.read(o1), w1, f"{at}: the pick queued beside it")


def run_learn_words(case, i, at):
    a, b = _streams(case)
    s0, s1 = bg.step("pick", i, seed=bg.SEED + 300 + i), bg.step("learn_then_pick", i)
    i0, w0 = case.m.apply(s0)                                  # a plain pick first, on the other stream, finished before the update (a caller orders its index
                                                               # updates against its own picks: include/eppk.h)
    reqs = case.m.rows(s1)
    p1, sc1 = case.orc.pick_batch(sc.CHAIN, case.m.pods, case.m.oix, reqs, case.m.B)[:2]
    go0, o0 = case.stage("pick", s0, i0, b)
    go1, o1 = case.stage("learn", s1, dict(reqs=reqs), a)
    case.ses.sync()
    go0()
    case.ses.sync()
    go1()
    case.ses.sync()
    case.m._learn(reqs, np.ascontiguousarray(p1, dtype=np.int32))
    _check(case.read(o0), w0, f"{at}: the pick in front")
    _check(case.read(o1), dict(picks=p1, scores=sc1), f"{at}: pick + learn")
    assert case.pk.index_size() == case.m.oix.size() and case.pk.index_selfcheck() == 0, f"{at}: the index after the update"
    s2 = bg.step("pick", i, R=48, seed=s1["seed"])            # rows of the same pool again: they find what was learnt
    case.model_step(dict(s2, op="pick_device"), f"{at}: a pick behind the update")


def run_filter_mask(case, i, at):
    a, b = _streams(case)
    if i in (0, 2):                                            # programs from the gauges of the snapshot just published
        case.model_step(dict(bg.step("set_filters", i), fam="filter"), f"{at}: set_filters")
    s0, s1 = dict(bg.step("pick_filtered", i, masked=bool(i & 1)), fam="filter"), bg.step("pick", i, seed=bg.SEED + 700 + i)
    i0, w0 = case.m.apply(s0)
    i1, w1 = case.m.apply(s1)
    assert case.m.programs and i0["cls"] is not None
    go1, o1 = case.stage("pick", s1, i1, b)
    go0, o0 = case.stage("filtered", s0, i0, a)
    case.ses.sync()
    go1()                                                      # a plain pick queued on the other stream while the mask rows are replaced
    go0()
    case.ses.sync()
    _check(case.read(o0, verdict=True), w0, f"{at}: pick_filtered_device with programs")
    _check(case.read(o1), w1, f"{at}: the pick queued beside it")


def run_subset_keys(case, i, at):
    filters = bg.subset_filters(case.endpoints, i)
    keys, off = case.pkg.picker.subset_entries_csr(filters)
    assert int(off[-1]) == bg.SUBSET_ROWS_ENTRIES[i][0] * bg.SUBSET_ROWS_ENTRIES[i][1], f"{at}: entries in all"
    R = len(filters)
    reqs = case.m.rows(bg.step("pick", i, R=R))
    mask = np.stack([case.pkg.picker.subset_mask(case.endpoints, f)[0] for f in filters])
    want = case.orc.pick_batch(sc.CHAIN, case.m.pods, case.m.oix, reqs, case.m.B, mask)[:2]
    assert np.array_equal(case.pk.subset_masks(filters), mask), f"{at}: the masks"
    p, s = case.pk.pick_subset(reqs, filters)
    _check(dict(picks=p, scores=s), dict(picks=want[0], scores=want[1]), f"{at}: pick_subset")


def run_index_insert(case, i, at):
    a, b = _streams(case)
    s1 = bg.step("pick", i, R=700, seed=bg.SEED + 800 + i)
    i1, w1 = case.m.apply(s1)
    go1, o1 = case.stage("pick", s1, i1, b)
    case.ses.sync()
    go1()
    case.ses.sync()                                            # (finished before the update: a caller orders its index updates against its own picks)
    h, p = bg.insert_pairs(case.m, i)
    case.m._insert(h, p)
    case.pk.index_insert(h, p)
    assert case.pk.index_size() == case.m.oix.size() and case.pk.index_selfcheck() == 0 and case.pk.index_dropped() == 0, f"{at}: the index after {h.size} pairs"
    _check(case.read(o1), w1, f"{at}: the pick in front")
    case.model_step(dict(bg.step("pick", i, R=48, seed=bg.SEED + 850 + i), op="pick_device"), f"{at}: a pick behind the insert")


def run_resolves(case, i, at):
    """bounded, banded (three bands) and costed one behind the other, on three streams: the scratch one grows is what the next reuses.
    Then a bounded resolve that takes NO ranks: the one call that sizes the library's own request states."""
    for j, form in enumerate(bg.resolve_forms(i)):
        s = bg.resolve_step(form, i, j)
        if form.startswith("resolve_"):                        # the resolve alone: over the lists the model makes for these rows
            rows = case.m.rows(s, R=bg.ALL_ROWS[i])
            case.m.lists = case.m._topk(rows, s["k"])
        inp, want = case.m.resolve(s)
        _check(case.ses.resolve(s, inp), want, f"{at}: {form}")
        assert case.pk.launch_status() == 0, f"{at}: {form}: launch status"
    s = dict(bg.resolve_step("resolve_bounded_device", i, 0), seed=bg.SEED + 100 * i + 7, load="fresh")
    case.m.lists = case.m._topk(case.m.rows(s, R=bg.ALL_ROWS[i]), s["k"])
    inp, want = case.m.resolve(s)
    t, R = case.t, inp["R"]
    d_lists, d_ls, d_cap, d_load = _dev(t, inp["lists"]), _dev(t, inp["list_scores"]), _dev(t, inp["cap"]), _dev(t, inp["load"])
    d_pick, d_score, _ = case.ses.outs(R)
    case.ses.sync()
    case.pk.bounded_resolve_device(d_lists.data_ptr(), d_ls.data_ptr(), R, inp["k"], _ptr(d_cap), inp["cap_all"], inp["policy"], d_load.data_ptr(), d_pick.data_ptr(),
                                   d_score.data_ptr(), None, case.ses.stream(s))
    case.ses.sync()
    got = dict(picks=d_pick.cpu().numpy(), scores=d_score.cpu().numpy(), load=d_load.cpu().numpy().view(np.uint32))
    _check(got, {key: want[key] for key in got}, f"{at}: resolve_bounded_device without ranks")
    assert case.pk.launch_status() == 0, f"{at}: without ranks: launch status"


RUN = dict(work_list=run_work_list, fallback_lists=run_fallback_lists, learn_words=run_learn_words, filter_mask=run_filter_mask, subset_keys=run_subset_keys,
           index_insert=run_index_insert, resolves=run_resolves)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("resident", (False, True), ids=("default", "resident"))
@pytest.mark.parametrize("buffer", bg.BUFFERS)
def test_small_large_small_larger(pkg, orc, monkeypatch, buffer, resident):
    tg._setenv(monkeypatch, dict(bg.ENV, **({"EPPK_RESIDENT": "1"} if resident else {})))
    case = Case(pkg, orc)
    try:
        assert case.pk.bounded_geometry() == (bg.CHUNK, bg.CHUNK)
        history = bg.growth(buffer)
        for i in range(bg.steps_of(buffer)):
            at = f"{buffer}, step {i} ({bg.ALL_ROWS[i]} rows at {bg.PODS[i]} pods{', resident' if resident else ''})"
            if i == 0 or bg.PODS[i] != bg.PODS[i - 1]:
                case.publish(bg.PODS[i], at)
                if i == 0:
                    case.model_step(bg.seed_step(), f"{at}: the index")
            if resident:                                       # a unit is running when the step replaces its buffer
                case.resident_pick(i, at)
                before = case.pk.resident_stats()
            RUN[buffer](case, i, at)
            assert case.pk.launch_status() == 0, f"{at}: launch status"
            if resident:                                       # ... and is started again by the next small batch: the step had parked it
                case.resident_pick(i, f"{at}: behind the step")
                on, batches, starts = case.pk.resident_stats()
                assert on and batches >= before[1] + 1, f"{at}: the small batch behind the step was answered by a resident unit: {before} -> {(on, batches, starts)}"
                if any(h[i] == "replace" for h in history.values()):
                    assert starts > before[2], f"{at}: a replacement parks the running unit, the next batch starts it again: {before} -> {(on, batches, starts)}"
        assert case.pk.index_size() == case.m.oix.size() and case.pk.index_selfcheck() == 0
    finally:
        case.close()


def test_two_contexts_grow_and_one_goes(pkg, orc, monkeypatch):
    """Two contexts of different shapes alive at once, each grown once; one is destroyed and the other goes on answering."""
    tg._setenv(monkeypatch, bg.ENV)
    other = dict(bg.CFG, max_pods=64, max_blocks=4, max_batch=32, index_slots=4096, groups=32, pods=(60,))
    a, b = Case(pkg, orc), Case(pkg, orc, other, bg.SEED + 1)
    live = [a, b]
    try:
        for name, c, P in (("A", a, 130), ("B", b, 60)):
            c.publish(P, name)
            c.model_step(bg.seed_step(), f"{name}: the index")
        for i in (0, 1):                                       # small, then large: every buffer of the three cases is replaced once in each context
            for name, c in (("A", a), ("B", b)):
                for run in (run_work_list, run_fallback_lists, run_resolves):
                    run(c, i, f"context {name}, step {i}, {run.__name__}")
        live.remove(a)
        a.close()
        for run in (run_work_list, run_fallback_lists, run_resolves):
            run(b, 2, f"context B after A was destroyed, {run.__name__}")
            run(b, 3, f"context B after A was destroyed, {run.__name__}")
        assert b.pk.launch_status() == 0 and b.pk.index_selfcheck() == 0
    finally:
        for c in live:
            c.close()
