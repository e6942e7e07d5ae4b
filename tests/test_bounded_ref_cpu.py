"""CPU: the numpy restatement of the bounded resolve (tests/bounded_ref.py, SEMANTICS.md §3d) against a second, naive statement of the
rule -- a loop per round and per request -- on the generator's cases (tests/bounded_cases.py); the invariants §3d states; the generator's
coverage; and the new names in the header against the Python binding's list."""
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (64, 512)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


bc = _load("bounded_cases")
ref = bc.ref


@pytest.fixture(scope="module")
def cases():
    return {chunk: [(c, bc.want(c)) for c in bc.make_cases(chunk)] for chunk in CHUNKS}


def naive(lists, scores, n_pods, cap, cap_all, policy, load):
    """§3d word for word: round by round, request by request."""
    R, k = lists.shape
    capv = [cap_all] * n_pods if cap is None else [int(x) for x in cap]
    ld = [0] * n_pods if load is None else [int(x) for x in load]
    pick, score, rank = [ref.NO_PICK] * R, [0.0] * R, [None] * R
    valid = lambda e: 0 <= e < n_pods                                    # noqa: E731
    bad = any(not valid(int(e)) and int(e) != ref.NO_PICK for e in lists.ravel())
    for j in range(k):
        room = [max(capv[p] - ld[p], 0) for p in range(n_pods)]          # all of round j on the loads round j - 1 left
        seen = [0] * n_pods
        for r in range(R):
            e = int(lists[r, j])
            if rank[r] is not None or not valid(e):
                continue
            if seen[e] < room[e]:
                pick[r], rank[r] = e, j
                score[r] = 0.0 if scores is None else scores[r, j]
                ld[e] += 1
            seen[e] += 1
    for r in range(R):
        if rank[r] is not None:
            continue
        firsts = [i for i in range(k) if valid(int(lists[r, i]))]
        if not firsts:
            rank[r] = ref.RANK_NONE
        elif policy == ref.SHED:
            rank[r] = ref.RANK_OVERFLOW
        else:
            f = firsts[0]
            pick[r], rank[r] = int(lists[r, f]), ref.RANK_OVERFLOW | f
            score[r] = 0.0 if scores is None else scores[r, f]
            ld[pick[r]] = (ld[pick[r]] + 1) & 0xFFFFFFFF
    return (np.array(pick, dtype=np.int32), np.array(score, dtype=np.float64), np.array(rank, dtype=np.uint8),
            np.array(ld, dtype=np.uint64).astype(np.uint32), bad)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_the_restatement_equals_the_naive_loop(cases, chunk):
    for c, got in cases[chunk]:
        want = naive(c["lists"], c["scores"], c["n_pods"], c["cap"], c["cap_all"], c["policy"], c["load"])
        for g, w, what in zip(got[:4], want[:4], ("picks", "scores", "ranks", "loads")):
            if what == "scores":
                g, w = g.view(np.uint64), w.view(np.uint64)
            assert np.array_equal(g, w), f"{bc.info(c)}: {what}"
        assert got[4] == want[4], bc.info(c)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_invariants(cases, chunk):
    for c, (pick, score, rank, load_out, bad) in cases[chunk]:
        L, P, k = c["lists"], c["n_pods"], c["lists"].shape[1]
        valid = (L >= 0) & (L < P)
        load_in = np.zeros(P, dtype=np.int64) if c["load"] is None else c["load"].astype(np.int64)
        capv = np.full(P, c["cap_all"], dtype=np.int64) if c["cap"] is None else c["cap"].astype(np.int64)
        placed = rank < k
        # a placed request holds exactly the entry its rank names; nobody is assigned twice (one pick, one rank per request)
        rows = np.nonzero(placed)[0]
        assert np.array_equal(pick[rows], L[rows, rank[rows]]) and np.all(valid[rows, rank[rows]]), bc.info(c)
        spilled = (rank & ref.RANK_OVERFLOW) != 0
        none = rank == ref.RANK_NONE
        assert np.all(placed ^ spilled ^ none) and not np.any(placed & spilled), bc.info(c)
        assert np.array_equal(none, ~valid.any(axis=1)), bc.info(c)
        if c["policy"] == ref.SHED:
            assert np.all(pick[spilled] == ref.NO_PICK) and np.all(rank[spilled] == ref.RANK_OVERFLOW), bc.info(c)
            assert np.all(load_out.astype(np.int64) <= np.maximum(capv, load_in)), f"{bc.info(c)}: SHED went above max(cap, load_in)"
        else:
            f = rank[spilled] & 0x3F
            assert np.array_equal(pick[spilled], L[spilled, f]) and np.array_equal(f, np.argmax(valid[spilled], axis=1)), bc.info(c)
        # every pick is counted once (modulo 2^32, as the loads are)
        grown = (load_out.astype(np.int64) - load_in) % (1 << 32)
        assert grown.sum() == np.count_nonzero(pick != ref.NO_PICK), bc.info(c)
        assert np.array_equal(grown, np.bincount(pick[pick >= 0], minlength=P)), bc.info(c)
        assert np.all(score[pick == ref.NO_PICK] == 0.0), bc.info(c)
        assert bad == ("out-of-range" in c["tags"]), bc.info(c)


@pytest.mark.parametrize("policy", [ref.SHED, ref.SPILL])
def test_caps_that_bind_nothing_give_column_0(policy):
    rng = np.random.default_rng(bc.SEED0)
    for R, P, k in ((1, 1, 1), (300, 5, 4), (1000, 64, 8)):
        lists = rng.integers(0, P, size=(R, k)).astype(np.int32)           # (column 0 always valid: what a picker's list looks like)
        lists[:, 1:][rng.random((R, k - 1)) < 0.2] = ref.NO_PICK
        scores = rng.standard_normal((R, k))
        pick, score, rank, load_out, bad = ref.resolve(lists, scores, P, None, R, policy, None)
        assert np.array_equal(pick, lists[:, 0]) and np.array_equal(score.view(np.uint64), scores[:, 0].view(np.uint64))
        assert not rank.any() and not bad and np.array_equal(load_out, np.bincount(lists[:, 0], minlength=P))


def test_order_by_round_is_not_the_sequential_greedy():
    """Row 1 loses pod 0 to row 0 and falls to pod 1 in round 1 -- but row 2 took pod 1 in round 0: a per-request loop would have let
    row 1 have it."""
    lists = np.array([[0, 1], [0, 1], [1, 0]], dtype=np.int32)
    pick, _, rank, load_out, _ = ref.resolve(lists, None, 2, None, 1, ref.SHED, None)
    assert pick.tolist() == [0, -1, 1] and rank.tolist() == [0, ref.RANK_OVERFLOW, 0] and load_out.tolist() == [1, 1]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_the_generator_covers_every_required_shape(cases, chunk):
    have = set().union(*(c["tags"] for c, _ in cases[chunk]))
    assert not set(bc.REQUIRED) - have, sorted(set(bc.REQUIRED) - have)
    by = {c["name"]: c for c, _ in cases[chunk]}
    assert len(by) == len(cases[chunk]), "case names are unique"
    sizes = {c["lists"].shape[0] for c, _ in cases[chunk]}
    assert {0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 7} <= sizes
    assert {c["lists"].shape[1] for c, _ in cases[chunk]} >= {1, 8}
    for P in (1, 63, 64, 65, 4096):
        assert np.any(by[f"pods-{P}"]["lists"] == P - 1)
    # the shapes that are about WHERE a row sits do sit there: both sides of the one-launch threshold, contended past a chunk boundary
    assert by["cascade-chunks"]["lists"].shape[0] > chunk >= by["cascade"]["lists"].shape[0]
    _, (pick, _, rank, _, _) = next(x for x in cases[chunk] if x[0]["name"] == "cascade")
    assert pick[2] == 2 and rank[2] == 2, "row 2 finds pod 1 filled by round 0, and goes on to round 2"
    assert pick[5] == ref.NO_PICK and rank[5] == ref.RANK_OVERFLOW
    c = by[f"one-pod-n{chunk + 1}-cap{chunk}"]
    pick = bc.want(c)[0]
    assert pick[chunk - 1] == 0 and pick[chunk] == 1, "room ends exactly at the chunk boundary"
    assert any(c["policy"] == ref.SPILL and int(bc.want(c)[3].min()) == 0 and c["load"] is not None and int(c["load"].max()) == 0xFFFFFFFF
               for c, _ in cases[chunk]), "a load of 2^32 - 1 wraps to 0"
    contended = [np.count_nonzero(w[2] != 0) / max(1, w[2].size) for c, w in cases[chunk] if "random" in c["tags"]]
    assert np.mean(contended) > 0.3, "the random cases are contended"


def test_symbols_and_header_agree_on_the_new_names():
    with open(os.path.join(ROOT, "include", "eppk.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    with open(os.path.join(ROOT, "gateway-api-inference-extension_amd", "_lib.py")) as f:
        src = f.read()
    syms = set(re.findall(r'"(eppk_[a-z0-9_]+)"', re.search(r"SYMBOLS = \[(.*?)\]", src, re.S).group(1)))
    new = {"eppk_bounded_resolve_device", "eppk_pick_bounded_device", "eppk_pick_bounded", "eppk_group_pick_bounded", "eppk_bounded_geometry"}
    declared = set(re.findall(r"\b(eppk_[a-z0-9_]+)\s*\(", hdr))
    assert new <= declared and new <= syms
    assert {s for s in declared if "bounded" in s} == {s for s in syms if "bounded" in s} == new
    for name in new:
        assert re.search(r"lib\.%s\.argtypes = \[" % name, src), f"{name} has no argtypes"
    for name, value in (("EPPK_BOUNDED_SHED", ref.SHED), ("EPPK_BOUNDED_SPILL", ref.SPILL), ("EPPK_RANK_OVERFLOW", ref.RANK_OVERFLOW),
                        ("EPPK_RANK_NONE", ref.RANK_NONE), ("EPPK_LAUNCH_BAD_PICK", ref.LAUNCH_BAD_PICK), ("EPPK_MAX_TOPK", ref.MAX_TOPK)):
        m = re.search(r"#define\s+%s\s+\(?(0x[0-9A-Fa-f]+|\d+)u?" % name, hdr)
        assert m and int(m.group(1), 0) == value, name
    assert re.search(r"#define EPPK_ABI_VERSION 4u", hdr), "additions only: the ABI version stays"
