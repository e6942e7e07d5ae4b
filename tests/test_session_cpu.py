"""CPU twin of tests/test_gpu_session.py: the session generator (tests/session_cases.py) delivers the coverage the GPU module relies on,
and its reference model is deterministic.  Every condition is evaluated on the generator and the model alone; no GPU."""
import importlib.util
import os
import zlib
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


sc = _load("session_cases")
ALL_SEEDS = tuple(sc.SEEDS) + (sc.BIG_SEED,)
FILTER_USES = ("filter_masks", "filter_masks_device", "pick_filtered")
UPDATES = ("seed_index", "insert", "insert_picks_device", "remove_pod", "tick_evict", "trim", "clear", "learn_then_pick", "stage_pair")


@pytest.fixture(scope="module")
def runs(pkg, orc):
    """Every committed session through the model, once: seed -> (steps with inputs and wanted outputs, what was observed on the way)."""
    out = {}
    for seed in ALL_SEEDS:
        seen = []

        def observe(m, s):
            o = dict(i=s["i"], updates=m.updates, P=m.P, assumed=m.assumed, nprog=len(m.programs), size=m.oix.size(), pods=zlib.crc32(m.pods.tobytes()),
                     sets=m.listed_sets() if s["op"] in UPDATES else None)
            if s["op"] == "pick_filtered":
                o.update(filtered=m.filtered, unfiltered=m.unfiltered)
            if s["op"] in FILTER_USES:
                o.update(stale=m.stale)
            seen.append(o)

        out[seed] = (sc.run_model(seed, orc, pkg.workload, observe), seen)
    return out


def _walk_families(steps):
    """The families of the walk: what lies between the prologue and the epilogue."""
    return [s["fam"] for s in steps if s["part"] == "walk"]


def test_the_walk_visits_every_ordered_pair_of_families():
    n = len(sc.FAMILIES)
    for rot in range(n):
        w = sc.euler_walk(n, rot)
        assert len(w) == n * n + 1 and len(set(zip(w, w[1:]))) == n * n
    pairs = Counter()
    for seed in sc.SEEDS:
        fams = _walk_families(sc.make_session(seed))
        assert len(fams) == n * n + 1
        pairs.update(zip(fams, fams[1:]))
    assert len(pairs) == n * n and min(pairs.values()) >= 2, sorted(pairs.items(), key=lambda kv: kv[1])[:4]
    assert all(pairs[(f, f)] >= 2 for f in sc.FAMILIES)


@pytest.mark.parametrize("seed", ALL_SEEDS)
def test_sizes_and_snapshots(seed):
    steps = sc.make_session(seed)
    cfg = sc.config(seed)
    assert 80 <= len(steps) <= 150
    pubs = [s for s in steps if s["op"] == "publish"]
    assert {65, 130, 1000} <= {s["P"] for s in pubs} and all(s["P"] <= cfg["max_pods"] for s in pubs)
    J = [-(-s["P"] // 64) for s in pubs]
    assert any(b < a for a, b in zip(J, J[1:])) and any(b > a for a, b in zip(J, J[1:])), "J shrinks and grows"
    assert all(a != b for a, b in zip(J, J[1:])), "every publish changes J"
    assert 0.25 <= np.mean([s["holes"] for s in pubs]) <= 0.45
    assert all(a["kind"] != b["kind"] for a, b in zip(pubs, pubs[1:]))
    assert all(s["R"] in sc.SIZES + sc.SMALL_SIZES for s in steps if "R" in s) and all(s["R"] <= cfg["max_batch"] for s in steps if "R" in s)
    assert all(s["R"] <= 64 for s in steps if s["op"].startswith("weighted"))
    assert {s["E"] for s in steps if s["op"] == "set_assumed_load"} == {0, 1, 3} or seed == sc.BIG_SEED


def test_every_operation_occurs(runs):
    ops = Counter(s["op"] for seed in ALL_SEEDS for s, _, want in runs[seed][0] if want is not None)
    for op in sc.RESOLVE_OPS + sc.PICK_OPS + sc.RANDOM_OPS + tuple(set(sc.FILTER_OPS)) + tuple(set(sc.INDEX_OPS)):
        assert ops[op] >= 1, op
    refused = Counter(s["op"] for seed in ALL_SEEDS for s, _, want in runs[seed][0] if want is None)
    for op in sc.REFUSALS:
        assert refused[op] >= 1, op
    assert sum(refused[op] for op in sc.RESOLVE_OPS) >= 3, "load resolves while assumed load is on"
    loads = Counter(s["load"] for seed in ALL_SEEDS for s, _, want in runs[seed][0] if want is not None and s["op"] in sc.RESOLVE_OPS)
    assert loads["none"] >= 3 and loads["fresh"] >= 3 and loads["carried"] >= 3, loads
    for seed in ALL_SEEDS:
        walk = [(s, inp) for s, inp, want in runs[seed][0] if want is not None and s["op"] in sc.RESOLVE_OPS and s["part"] == "walk"]
        assert any(s["load"] == "carried" and inp["load"].any() for s, inp in walk), f"{seed}: a carried load inside the walk"
        assert any(s["op"] in sc.OWN_FORMS and inp["R"] > 512 for s, inp in walk), f"{seed}: a resolve of many chunks inside the walk"
        assert any(s["op"] in sc.OWN_FORMS and inp["R"] <= 64 for s, inp in walk), f"{seed}: ... and one of a single chunk"
    srcs = set()
    for seed in ALL_SEEDS:
        last = None
        for s, _, want in runs[seed][0]:
            if s["op"].startswith("pick_topk") or s["op"] == "pick_filtered" or (s["op"].startswith("weighted") and s["k"] > 1):
                last = s["op"].split("_masked")[0]
            if s["op"] == "publish":
                last = None
            if s["op"].startswith("resolve_") and want is not None:
                assert last is not None
                srcs.add(last)
    assert srcs == {"pick_topk", "pick_filtered", "weighted_random"}, srcs


@pytest.mark.parametrize("seed", ALL_SEEDS)
def test_pick_filtered_runs_with_programs(runs, seed):
    """pick_filtered with programs set, in every session: planes built through this entry point, d_fmask allocated, grown and reused."""
    run, seen = runs[seed]
    uses, pairs, bumped, taken = [], 0, False, 0
    prev, bump, lists_from = None, False, None
    for (s, inp, want), o in zip(run, seen):
        op = s["op"]
        if op.startswith("set_filters"):
            prev = None                                        # (set_filters makes the planes stale by itself: such a pair shows nothing about the publish)
        if op == "publish":
            bump, lists_from = False, None
        if op in ("pick", "pick_masked") and s.get("assumed") and want is not None:
            bump = True
        if op.startswith("pick_topk") or (op.startswith("weighted") and s["k"] > 1):
            lists_from = op
        if op.startswith("resolve_") and want is not None and lists_from == "pick_filtered":
            taken += 1
        if op != "pick_filtered" or want is None:
            continue
        lists_from = op
        if not o["nprog"]:
            continue
        assert inp["cls"] is not None and o["filtered"].shape == o["unfiltered"].shape
        assert (o["filtered"] != o["unfiltered"]).any(), f"step {s['i']}: the programs filter nothing"
        uses.append(s["R"])
        J = -(-o["P"] // 64)
        if prev is not None and prev != J:
            pairs += 1
        prev = J
        bumped |= bump and not o["assumed"]
    assert len(uses) >= 6, uses
    assert any(b > a for a, b in zip(uses, uses[1:])) and any(b < a for a, b in zip(uses, uses[1:])), f"a larger batch behind a smaller one, and back: {uses}"
    assert pairs >= 1, "pick_filtered on each side of a publish that changes J, no set_filters between them"
    assert bumped, "pick_filtered behind an assumed-load bump of the same snapshot"
    assert taken >= 2, "resolves alone over filtered lists"


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_resolve_batches_fall_on_both_sides_of_a_chunk(runs, seed):
    R = [inp["R"] for s, inp, want in runs[seed][0] if s["op"] in sc.RESOLVE_OPS and want is not None]
    for chunk in (64, 512):
        assert min(R) <= chunk < max(R), (chunk, R)
    assert -(-max(R) // 64) >= 17, "17 chunks under EPPK_BOUND_CHUNK=64"
    assert any(b > a for a, b in zip(R, R[1:])) and any(b < a for a, b in zip(R, R[1:])), R
    grew = R.index(max(R))
    assert any(r < max(R) for r in R[grew + 1:]), "a smaller batch reuses the grown scratch"


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_a_publish_changes_J_between_two_uses(runs, seed):
    run, seen = runs[seed]
    kinds = {"bounded": lambda s: "bounded" in s["op"], "banded": lambda s: "banded" in s["op"], "costed": lambda s: "costed" in s["op"],
             "filter": lambda s: s["op"] in FILTER_USES, "masked pick": lambda s: s["op"] == "pick_masked"}
    for name, is_use in kinds.items():
        J = [-(-o["P"] // 64) for (s, _, want), o in zip(run, seen) if want is not None and is_use(s)]
        assert len(set(J)) >= 2 and any(a != b for a, b in zip(J, J[1:])), (name, J)
    # the filter: only uses WITH programs count, and only a pair with no set_filters between them (which makes the planes stale by itself)
    changed, prev = 0, None
    for (s, _, want), o in zip(run, seen):
        if s["op"].startswith("set_filters"):
            prev = None
        elif s["op"] in FILTER_USES and want is not None and o["nprog"]:
            J = -(-o["P"] // 64)
            changed += prev is not None and prev != J
            prev = J
    assert changed >= 2, "two filter uses with programs, a publish that changes J and no set_filters between them"


@pytest.mark.parametrize("seed", ALL_SEEDS)
def test_assumed_load_goes_on_and_off_between_filter_calls(runs, seed):
    run = runs[seed][0]
    ops = [s["op"] for s, _, _ in run]
    tail = ops[-18:-1]
    assert tail[:5] == ["set_filters", "pick_filtered", "publish", "pick_filtered", "set_filters"]
    tail = tail[1:]
    assert tail[4:10] == ["filter_masks", "set_assumed_load", "pick", "filter_masks", "set_assumed_load", "filter_masks"]
    assert tail[10:] == ["pick_filtered", "resolve_costed_device", "pick_masked", "pick_bounded", "pick_banded_device", "pick_costed"]
    steps = [s for s, _, _ in runs[seed][0]][-17:-1]
    assert steps[5]["E"] == 3 and steps[8]["E"] == 0 and steps[6]["assumed"] == 3
    seen = runs[seed][1][-17:-1]
    for j in (7, 9, 10):                                       # the filter calls behind the bump, pick_filtered among them
        want = run[-17:-1][j][2]
        masks = want["masks"] if "masks" in want else seen[j]["filtered"]
        assert seen[j]["stale"] is not None and (seen[j]["stale"] != masks).any(), f"step {seen[j]['i']}: planes of the rows before the bump would give the same masks"
    assert all(o["nprog"] > 0 for o in seen[1:]), "programs are set through all of it"
    assert seen[6]["pods"] != seen[5]["pods"], "the pick bumps the rows"
    assert seen[4]["pods"] == seen[5]["pods"] and len({o["pods"] for o in seen[6:]}) == 1, "... and nothing else does: the later filter calls read the bumped rows"
    assert all(want is not None for _, _, want in runs[seed][0][-6:]), "the resolves behind it are not refused"


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_the_set_table_is_rebuilt_with_picks_on_both_sides(runs, seed):
    run, seen = runs[seed]
    cfg = sc.config(seed)
    sets_cap = max(1024, cfg["index_slots"] // 16)
    assert seen[-1]["updates"] >= 17
    full = [o for o in seen if o["sets"] is not None and o["sets"] > sets_cap // 2]
    assert len(full) >= 17, "updates while the listed sets fill more than half of the set table"
    first, last = full[0]["i"], full[-1]["i"]
    picks = [s["i"] for s, _, want in run if s["fam"] in ("picks", "random") and want is not None]
    assert any(i > last for i in picks) and sum(full[15]["i"] < i < last for i in picks) >= 2, "picks between the updates and behind them"


@pytest.mark.parametrize("seed", ALL_SEEDS)
def test_a_heavily_deferring_batch_and_eligible_ones(runs, seed):
    by = {s.get("quad"): inp for s, inp, _ in runs[seed][0] if s.get("quad")}
    order = [s["quad"] for s, _, _ in runs[seed][0] if s.get("quad")]
    assert set(order) <= set(sc.QUAD_KINDS)
    if seed % 2:                                               # an unmasked batch above n/4
        assert order == ["eligible", "heavy", "after"]
        n = by["heavy"]["reqs"].shape[0]
        assert n >= 4 and by["heavy"]["mask"] is None and sc.deferring(by["heavy"]["reqs"]).sum() > n // 4, "above the pause threshold of an unmasked batch"
    else:                                                      # a share between n/8 and n/4: unmasked it leaves the route on, masked it pauses it
        assert order == ["eligible", "moderate", "heavy_masked", "after"]
        for kind in ("moderate", "heavy_masked"):
            n = by[kind]["reqs"].shape[0]
            assert n >= 4 and n // 8 < sc.deferring(by[kind]["reqs"]).sum() <= n // 4, kind
        assert by["moderate"]["mask"] is None and by["heavy_masked"]["mask"] is not None
        bits = np.unpackbits(by["heavy_masked"]["mask"].view(np.uint8), axis=1).sum(axis=1)
        assert (bits == runs[seed][1][0]["P"]).all(), "every pod a candidate: the reserved hashes alone defer"
    assert not sc.deferring(by["eligible"]["reqs"]).any() and not sc.deferring(by["after"]["reqs"]).any()


def test_live_hashes_stay_below_the_capacity(runs):
    for seed in ALL_SEEDS:
        cfg = sc.config(seed)
        top = max(o["size"] for o in runs[seed][1])
        assert top < cfg["index_slots"] // 2 * 3 // 4, (seed, top)


def test_the_model_is_deterministic(pkg, orc, runs):
    for seed in (sc.SEEDS[0], sc.BIG_SEED):
        again = sc.run_model(seed, orc, pkg.workload)
        assert sc.digest(again) == sc.digest(runs[seed][0])
        assert [s for s, _, _ in again] == sc.make_session(seed)
    assert sc.digest(runs[sc.SEEDS[0]][0]) != sc.digest(runs[sc.SEEDS[1]][0])


def test_a_failure_names_seed_step_operation_and_trail():
    steps = sc.make_session(sc.SEEDS[1])
    i = next(s["i"] for s in steps if s["op"] in sc.RESOLVE_OPS and s["i"] > 40)
    msg = sc.where(sc.SEEDS[1], steps, i)
    assert f"seed {sc.SEEDS[1]}" in msg and f"step {i} " in msg and steps[i]["op"] + "(" in msg and f"seed={steps[i]['seed']}" in msg
    assert f"{i - 1}:{steps[i - 1]['op']}" in msg and f"{i - 12}:{steps[i - 12]['op']}" in msg


def test_refused_steps_leave_the_model_unchanged(pkg, orc):
    seed = sc.SEEDS[0]
    m = sc.Model(seed, orc, pkg.workload)
    for s in sc.make_session(seed):
        before = (m.pods.tobytes(), m.oix.size(), repr(m.programs), m.assumed, None if m.load is None else m.load.tobytes(), m.lists is None)
        try:
            m.apply(s)
        except sc.Refused:
            assert before == (m.pods.tobytes(), m.oix.size(), repr(m.programs), m.assumed, None if m.load is None else m.load.tobytes(), m.lists is None), s
