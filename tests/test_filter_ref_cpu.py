"""CPU: the numpy restatement of the Filter phase's metric predicates (tests/filter_ref.py, SEMANTICS.md §2c) on hand-computed cases, and
the seeded case generator (tests/filter_cases.py) held to the coverage the GPU tests rely on -- on the restatement alone."""
import importlib.util
import os

import numpy as np
import pytest


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fc = _load("filter_cases")
ref = fc.ref
vc = fc.vc
U32 = (1 << 32) - 1
NAN = float("nan")


def _pods(queue, running=None, kv=None, max_lora=None, active=None, waiting=None, holes=()):
    P = len(queue)
    pods = np.zeros(P, dtype=vc.POD_DTYPE)
    pods["queue"] = queue
    pods["running"] = running if running is not None else 0
    pods["kv_util"] = kv if kv is not None else 0.0
    pods["max_lora"] = max_lora if max_lora is not None else 0
    for name, sets in (("active", active), ("waiting", waiting)):
        for p, ids in enumerate(sets or []):
            for a in ids:
                pods[name][p, a >> 6] |= np.uint64(1) << np.uint64(a & 63)
    for p in holes:
        pods["flags"][p] = 1
    return pods


def _run(pods, prog, adapter=-1, mask=None, cls=None, programs=None):
    cand, v = ref.filter_masks(pods, programs if programs is not None else [prog], [adapter], cls, mask)
    return [int(p) for p in np.nonzero(cand[0])[0]], int(v[0])


# four pods; the gauges are chosen so that every kind has a threshold that passes all, some and none of them
PODS4 = _pods(queue=[5, 9, 9, 20], running=[1, 2, 3, 4], kv=[0.25, 0.5, 0.75, 1.0], max_lora=[2, 2, 1, 0],
              active=[[7], [64], [], []], waiting=[[], [7], [3], []])
# LORA_LOADED for adapter 7: pods 0 (active) and 1 (waiting).  LORA_SERVABLE for adapter 7: those two; pod 2 holds one adapter of
# max_lora 1 (no room), pod 3 has max_lora 0 -> no.  For adapter 64: loaded on pod 1 only; servable on 0 (1 < 2: room) and 1.
# the same pods with every adapter slot taken: pod 0 holds 1 of 1, pod 1 2 of 2, pod 2 1 of 1, pod 3 has none -- an adapter nobody holds is
# servable nowhere
PODS4_FULL = PODS4.copy()
PODS4_FULL["max_lora"] = [1, 2, 1, 0]
ALL, SOME, NONE = "all", "some", "none"
KIND_CASES = [
    (ref.QUEUE_LE, 20, -1, ALL, [0, 1, 2, 3]), (ref.QUEUE_LE, 9, -1, SOME, [0, 1, 2]), (ref.QUEUE_LE, 4, -1, NONE, []),
    (ref.RUNNING_LE, 4, -1, ALL, [0, 1, 2, 3]), (ref.RUNNING_LE, 1, -1, SOME, [0]), (ref.RUNNING_LE, 0, -1, NONE, []),
    (ref.KV_LE, 1.0, -1, ALL, [0, 1, 2, 3]), (ref.KV_LE, 0.5, -1, SOME, [0, 1]), (ref.KV_LE, 0.2499, -1, NONE, []),
    (ref.LORA_LOADED, 0, -1, ALL, [0, 1, 2, 3]), (ref.LORA_LOADED, 0, 7, SOME, [0, 1]), (ref.LORA_LOADED, 0, 127, NONE, []),
    (ref.LORA_SERVABLE, 0, -1, ALL, [0, 1, 2, 3]), (ref.LORA_SERVABLE, 0, 64, SOME, [0, 1]), (ref.LORA_SERVABLE, 0, 3, SOME, [0, 2]),
    (ref.LORA_SERVABLE, 0, 100, NONE, [], PODS4_FULL), (ref.LORA_SERVABLE, 0, 7, SOME, [0, 1], PODS4_FULL),
    (ref.QUEUE_WITHIN, 15, -1, ALL, [0, 1, 2, 3]), (ref.QUEUE_WITHIN, 4, -1, SOME, [0, 1, 2]), (ref.QUEUE_WITHIN, 0, -1, SOME, [0]),
]


@pytest.mark.parametrize("policy", [ref.REQUIRE, ref.PREFER])
@pytest.mark.parametrize("case", KIND_CASES)
def test_each_kind_each_policy_each_outcome(case, policy):
    kind, thr, adapter, outcome, want = case[:5]
    pods = case[5] if len(case) > 5 else PODS4
    got, v = _run(pods, [(kind, policy, thr)], adapter)
    if outcome == NONE:
        assert v == (1 | ref.SHED if policy == ref.REQUIRE else 1)
        assert got == ([] if policy == ref.REQUIRE else [0, 1, 2, 3])
    else:
        assert (got, v) == (want, 0)


def test_servable_with_no_pod_that_can_serve_passes_none():
    # adapter 100 is nowhere; only pod 0 (1 of 2) and pod 1 (2 of 2: full) ... pod 0 has room -> SOME; with pod 0 masked out: none
    mask = ref.pack(np.array([[False, True, True, True]]))
    assert _run(PODS4, [(ref.LORA_SERVABLE, ref.REQUIRE, 0)], 100, mask) == ([], 1 | ref.SHED)
    assert _run(PODS4, [(ref.LORA_SERVABLE, ref.PREFER, 0)], 100, mask) == ([1, 2, 3], 1)
    assert _run(PODS4, [(ref.LORA_SERVABLE, ref.REQUIRE, 0)], 100) == ([0], 0)


def test_queue_within_never_empties_a_set():
    for u in (0, 1, U32):
        got, v = _run(PODS4, [(ref.QUEUE_WITHIN, ref.REQUIRE, u)])
        assert got and v == 0


def test_verdict_bits_name_their_stage_and_an_empty_c0_reports_nothing():
    prog = [(ref.QUEUE_LE, ref.PREFER, 4), (ref.RUNNING_LE, ref.PREFER, 2), (ref.KV_LE, ref.PREFER, 0.0), (ref.QUEUE_LE, ref.REQUIRE, 0)]
    # stage 0 passes none (waived), stage 1 keeps pods 0 and 1, stage 2 passes none of them (waived), stage 3 sheds
    assert _run(PODS4, prog) == ([], 0b0001 | 0b0100 | 0b1000 | ref.SHED)
    assert _run(PODS4, prog[:3]) == ([0, 1], 0b0101)
    empty = ref.pack(np.zeros((1, 4), dtype=bool))
    assert _run(PODS4, prog, mask=empty) == ([], 0)                          # C_0 empty: no stage runs, no bit
    holes = _pods(queue=[5, 9], holes=(0, 1))
    assert _run(holes, [(ref.QUEUE_LE, ref.REQUIRE, 0)]) == ([], 0)          # ... whoever emptied it


def test_a_shed_request_skips_the_stages_behind_it():
    prog = [(ref.QUEUE_LE, ref.REQUIRE, 0), (ref.RUNNING_LE, ref.PREFER, 0)]
    assert _run(PODS4, prog) == ([], 1 | ref.SHED)                           # stage 1 finds C_1 empty: no bit 1


def test_classes_select_programs_and_a_bad_class_has_no_candidates():
    programs = [[(ref.QUEUE_LE, ref.REQUIRE, 5)], [(ref.QUEUE_LE, ref.REQUIRE, 9)]]
    cand, v = ref.filter_masks(PODS4, programs, [-1, -1, -1, -1], cls=np.array([0, 1, 2, 255], dtype=np.uint8))
    assert [list(np.nonzero(c)[0]) for c in cand] == [[0], [0, 1, 2], [], []]
    assert list(v) == [0, 0, ref.BAD_CLASS, ref.BAD_CLASS]
    cand, v = ref.filter_masks(PODS4, programs, [-1, -1])                    # no class array: program 0
    assert [list(np.nonzero(c)[0]) for c in cand] == [[0], [0]] and list(v) == [0, 0]


def test_no_programs_is_the_identity_on_c0():
    pods = _pods(queue=[1, 2, 3], holes=(1,))
    mask = np.array([[0xFFFFFFFFFFFFFFFF]], dtype=np.uint64)                 # bits >= n_pods are dropped
    cand, v = ref.filter_masks(pods, [], [5], None, mask)
    assert list(np.nonzero(cand[0])[0]) == [0, 2] and int(v[0]) == 0
    words, _ = ref.filter_mask_words(pods, [], [5], None, mask)
    assert words.tolist() == [[0b101]]


def test_queue_within_after_a_narrowing_stage_at_the_top_of_u32():
    pods = _pods(queue=[0, U32 - 1, U32, U32], running=[9, 1, 1, 1])
    # alone, the minimum is pod 0's 0 and `within 1` keeps only it; behind RUNNING_LE 1 the stage FINDS {1, 2, 3}: minimum 2^32 - 2
    assert _run(pods, [(ref.QUEUE_WITHIN, ref.REQUIRE, 1)]) == ([0], 0)
    assert _run(pods, [(ref.RUNNING_LE, ref.REQUIRE, 1), (ref.QUEUE_WITHIN, ref.REQUIRE, 1)]) == ([1, 2, 3], 0)
    assert _run(pods, [(ref.RUNNING_LE, ref.REQUIRE, 1), (ref.QUEUE_WITHIN, ref.REQUIRE, 0)]) == ([1], 0)
    assert _run(pods, [(ref.QUEUE_WITHIN, ref.REQUIRE, U32)]) == ([0, 1, 2, 3], 0)          # 2^32 - 1 - 0 does not wrap
    assert _run(pods, [(ref.QUEUE_WITHIN, ref.REQUIRE, U32 - 1)]) == ([0, 1], 0)


def test_kv_compare_is_raw_ieee():
    pods = _pods(queue=[0, 0, 0, 0], kv=[NAN, -0.0, 0.0, float("inf")])
    assert _run(pods, [(ref.KV_LE, ref.REQUIRE, 0.0)]) == ([1, 2], 0)        # -0.0 <= 0.0; a NaN gauge passes nothing
    assert _run(pods, [(ref.KV_LE, ref.REQUIRE, -0.0)]) == ([1, 2], 0)
    assert _run(pods, [(ref.KV_LE, ref.REQUIRE, NAN)]) == ([], 1 | ref.SHED)  # a NaN threshold passes nothing
    assert _run(pods, [(ref.KV_LE, ref.PREFER, NAN)]) == ([0, 1, 2, 3], 1)
    assert _run(pods, [(ref.KV_LE, ref.REQUIRE, float("inf"))]) == ([1, 2, 3], 0)
    assert _run(pods, [(ref.KV_LE, ref.REQUIRE, 2.0)]) == ([1, 2], 0)        # no clamp: inf stays above 2


def test_lora_popcounts_and_compare_are_those_of_the_scorer():
    ones = list(range(128))
    pods = _pods(queue=[0, 0, 0], max_lora=[256, 257, U32], active=[ones, ones, []], waiting=[ones, ones, [5]])
    pods["active"][2] = 0
    # 256 adapters loaded: no room under max_lora 256, room under 257; adapter 9 is held by pods 0 and 1 anyway
    assert _run(pods, [(ref.LORA_SERVABLE, ref.REQUIRE, 0)], 9) == ([0, 1, 2], 0)
    pods["active"][:2] = 0
    pods["waiting"][:2, 1] = 0
    pods["waiting"][:2, 0] = np.uint64(0xFFFFFFFFFFFFFFFF) & ~np.uint64(1 << 9)          # 63 held, not adapter 9
    pods["max_lora"][:2] = (63, 64)
    assert _run(pods, [(ref.LORA_SERVABLE, ref.REQUIRE, 0)], 9) == ([1, 2], 0)
    assert _run(pods, [(ref.LORA_LOADED, ref.REQUIRE, 0)], 63) == ([0, 1], 0)            # the last bit of word 0


# ---- the generator ---------------------------------------------------------------------------------------------------------------------

SEEDS = list(range(fc.SEED0, fc.SEED0 + fc.N_SEEDS))


@pytest.fixture(scope="module")
def generated():
    out = []
    for seed in SEEDS:
        c = fc.make_case(seed)
        cand, verdict = ref.filter_masks(c["pods"], c["programs"], c["adapter"], c["cls"], c["mask"])
        out.append((c, cand, verdict))
    return out


def test_every_generated_case_holds_every_outcome_class(generated):
    for c, cand, verdict in generated:
        oc = fc.outcomes(c, cand, verdict)
        for name, rows in oc.items():
            assert rows.any(), f"{fc.info(c)}: no {name} request"
            assert rows.sum() <= 0.9 * c["R"], f"{fc.info(c)}: {rows.sum()} of {c['R']} rows are {name}"
        assert not np.any(verdict & ref.BAD_CLASS)
        # the constructed rows are what the generator says they are
        assert oc["untouched"][0] and oc["narrowed"][1] and oc["waived"][2] and oc["shed"][3]
        assert not cand[4].any() and verdict[4] == 0


def test_every_pair_appears_in_every_stage_position(generated):
    seen = set()
    for c, _, _ in generated:
        assert len(c["programs"]) == 4 and len(c["programs"][0]) == 4
        for s, (kind, pol, _) in enumerate(c["programs"][0]):
            seen.add((kind, pol, s))
    assert seen == {(k, pol, s) for k, pol in fc.PAIRS for s in range(4)}


def test_generated_values_are_at_the_edges(generated):
    qmodes, kvmodes, holes, tails, adapters, shapes = set(), set(), set(), 0, set(), set()
    for c, _, _ in generated:
        qmodes.add(c["qmode"]); kvmodes.add(c["kvmode"]); holes.add(c["holes"]); shapes.add(c["P"])
        adapters.update(int(a) for a in c["adapter"])
        if c["P"] % 64:
            assert int(c["mask"][5, -1]) >> (c["P"] % 64), fc.info(c)        # bits that name no pod
            tails += 1
        assert c["reqs"].shape == (c["R"], 1) and c["R"] >= fc.MIN_ROWS
    assert qmodes == set(vc.QUEUE_MODES) and kvmodes == set(vc.KV_MODES) and holes == {False, True}
    assert adapters == set(vc.SEAM_ADAPTERS) and shapes == set(fc.PODS) and tails >= 8


def test_generated_thresholds_flip_compares(generated):
    """The fuzz program's thresholds sit at the gauges: over the seeds, every kind both keeps and rejects candidates somewhere."""
    kept, lost = set(), set()
    for c, _, _ in generated:
        live = (c["pods"]["flags"] & 1) == 0
        for kind, _, thr in c["programs"][0]:
            for a in (-1, 0):
                ok = ref.predicate(c["pods"], kind, thr, a, live)[live]
                if ok.any():
                    kept.add(kind)
                if not ok.all():
                    lost.add(kind)
    assert kept == set(ref.KINDS) and lost == set(ref.KINDS)


def test_the_restatement_agrees_with_a_bitwise_formulation(generated):
    """An independent formulation of the pod-only kinds on packed words: a cross-check of pack / unpack and of the stage loop."""
    for c, cand, verdict in generated[:6]:
        pods, P = c["pods"], c["P"]
        live = (pods["flags"] & 1) == 0
        for r in range(c["R"]):
            prog = c["programs"][int(c["cls"][r])]
            if any(k in (ref.LORA_LOADED, ref.LORA_SERVABLE, ref.QUEUE_WITHIN) for k, _, _ in prog):
                continue
            C = {p for p in range(P) if live[p] and (int(c["mask"][r, p // 64]) >> (p % 64)) & 1}
            v = 0
            for s, (kind, pol, thr) in enumerate(prog):
                if not C:
                    break
                gauge = {ref.QUEUE_LE: "queue", ref.RUNNING_LE: "running", ref.KV_LE: "kv_util"}[kind]
                K = {p for p in C if pods[gauge][p] <= thr}
                if K:
                    C = K
                else:
                    v |= 1 << s
                    if pol == ref.REQUIRE:
                        C, v = set(), v | ref.SHED
            assert sorted(C) == list(np.nonzero(cand[r])[0]) and v == verdict[r], (fc.info(c), r)
