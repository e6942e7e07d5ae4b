"""Inputs for the bounded resolve (SEMANTICS.md §3d): the smallest shapes that can break it, placed by the chunk size of the context under
test (BatchedPicker.bounded_geometry), and seeded random cases with few pods and many requests, so that most rounds are contended.

A case is a dict: name, tags (what it covers: tests/test_bounded_ref_cpu.py holds the generator to the list in REQUIRED), lists [R, k] i32,
scores [R, k] f64 (or None), n_pods, cap (u32 [n_pods] or None), cap_all, policy, load (u32 [n_pods] or None), and the outputs the caller
does NOT ask for: no_score, no_rank."""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("bounded_ref")
SEED0 = 0xB0D5
NO = ref.NO_PICK

REQUIRED = (
    ["n=0", "n=1", "n=63", "n=64", "n=65", "n=chunk-1", "n=chunk", "n=chunk+1", "n=3chunk+7"] +
    ["pods=1", "pods=63", "pods=64", "pods=65", "pods=4096", "last-pod"] +
    ["one-trip-64", "rows-63-64", "rows-chunk-1-chunk", "room-ends-at-trip", "room-ends-at-chunk", "room-0", "cap-all-0-shed", "cap-all-0-spill"] +
    ["k=1", "k=8", "trailing-no-pick", "middle-no-pick", "empty-list", "duplicate-pod", "out-of-range", "cascade", "load-above-cap",
     "load-wraps", "cap-array", "null-load", "null-score", "null-rank", "random"])


def _scores(rng, shape):
    """Totals with every kind of bit pattern a score can have short of NaN: the resolve copies them, it does not compute."""
    t = rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 4, size=shape)
    t[rng.random(shape) < 0.05] = -0.0
    return t


def _case(name, tags, lists, n_pods, cap_all=0, cap=None, policy=ref.SHED, load=None, scores="random", no_score=False, no_rank=False, seed=0):
    lists = np.ascontiguousarray(lists, dtype=np.int32)
    assert lists.ndim == 2
    if isinstance(scores, str):
        scores = _scores(np.random.default_rng(SEED0 + seed + lists.size), lists.shape)
    return dict(name=name, tags=set(tags), lists=lists, scores=scores, n_pods=int(n_pods),
                cap=None if cap is None else np.ascontiguousarray(cap, dtype=np.uint32), cap_all=int(cap_all), policy=int(policy),
                load=None if load is None else np.ascontiguousarray(load, dtype=np.uint32), no_score=no_score, no_rank=no_rank)


def _random_lists(rng, n, k, n_pods, p_no=0.1, hot=None):
    lists = rng.integers(0, n_pods, size=(n, k)).astype(np.int32)
    if hot is not None:
        lists[rng.random((n, k)) < 0.4] = hot
    lists[rng.random((n, k)) < p_no] = NO
    return lists


def _spread(rows, at, k):
    """The given rows at the given batch positions, every other row an empty list (no bid in any round)."""
    n = max(at) + 1
    lists = np.full((n, k), NO, dtype=np.int32)
    for r, row in zip(at, rows):
        lists[r, : len(row)] = row
    return lists


def want(c):
    """The restatement's answer for a case: (pick, score, rank, load_out, bad)."""
    return ref.resolve(c["lists"], c["scores"], c["n_pods"], c["cap"], c["cap_all"], c["policy"], c["load"])


def info(c):
    return f"{c['name']} (R {c['lists'].shape[0]} k {c['lists'].shape[1]} pods {c['n_pods']} policy {c['policy']})"


def make_cases(chunk):
    """Every case, for a context whose chunk holds `chunk` rows (a power of two >= 64; the one-launch kernel takes up to `chunk` rows)."""
    rng = np.random.default_rng(SEED0 + chunk)
    out = []
    # -- batch sizes around a trip, a chunk, and several chunks with a ragged end; few pods, every round contended
    sizes = [("0", 0), ("1", 1), ("63", 63), ("64", 64), ("65", 65), ("chunk-1", chunk - 1), ("chunk", chunk), ("chunk+1", chunk + 1),
             ("3chunk+7", 3 * chunk + 7)]
    for i, (label, n) in enumerate(sizes):
        P = 7
        out.append(_case(f"size-{label}", [f"n={label}"], _random_lists(rng, n, 3, P), P, cap_all=max(1, n // 12), policy=i & 1,
                         load=rng.integers(0, 3, size=P), seed=i))
    # -- pod counts around a mask word and the largest snapshot; the last pod takes bids on both sides of a chunk boundary
    for P in (1, 63, 64, 65, 4096):
        lists = _random_lists(rng, 2 * chunk + 3, 2, P, hot=P - 1)
        out.append(_case(f"pods-{P}", [f"pods={P}", "last-pod"], lists, P, cap_all=5, policy=ref.SPILL, load=np.zeros(P), seed=P))
        out.append(_case(f"pods-{P}-one-launch", [f"pods={P}", "last-pod"], lists[:61], P, cap_all=5, load=np.zeros(P), seed=P + 1))
    # -- one pod's bidders: all 64 lanes of one trip; rows 63 and 64 (the counter carried from trip to trip); rows chunk-1 and chunk (the
    #    prefix over the chunks); room that ends exactly at a trip and at a chunk boundary, or one row later
    P = 3
    for n, cap, tags in ((64, 64, ["one-trip-64", "room-ends-at-trip"]), (64, 63, ["one-trip-64"]), (65, 64, ["rows-63-64", "room-ends-at-trip"]),
                         (65, 65, ["rows-63-64"]), (130, 128, ["room-ends-at-trip"]), (chunk + 1, chunk, ["rows-chunk-1-chunk", "room-ends-at-chunk"]),
                         (chunk + 1, chunk + 1, ["rows-chunk-1-chunk"]), (chunk + 1, chunk - 1, ["rows-chunk-1-chunk"]),
                         (2 * chunk + 5, 2 * chunk, ["room-ends-at-chunk"]), (2 * chunk + 5, chunk + 64, ["room-ends-at-trip"])):
        lists = np.tile(np.array([[0, 1]], dtype=np.int32), (n, 1))
        same = [c for c in out if c["name"] == f"one-pod-n{n}-cap{cap}"]       # (a chunk of 64 rows: a trip is a chunk)
        if same:
            same[0]["tags"] |= set(tags)
            continue
        out.append(_case(f"one-pod-n{n}-cap{cap}", tags, lists, P, cap_all=cap, load=np.zeros(P), seed=n + cap))
    # -- no room at all
    lists = _random_lists(rng, chunk + 9, 2, 5)
    out.append(_case("room-0", ["room-0"], lists, 5, cap=[3, 0, 4, 2, 0], load=[3, 0, 1, 7, 0], policy=ref.SPILL))
    for pol, tag in ((ref.SHED, "cap-all-0-shed"), (ref.SPILL, "cap-all-0-spill")):
        for n in (40, chunk + 9):
            out.append(_case(f"{tag}-n{n}", [tag, "room-0"], lists[:n], 5, cap_all=0, policy=pol, load=np.zeros(5), seed=n))
    # -- list lengths
    for k in (1, 8):
        for n in (50, 2 * chunk + 1):
            out.append(_case(f"k{k}-n{n}", [f"k={k}"], _random_lists(rng, n, k, 6), 6, cap_all=max(2, n // 10), policy=k & 1, load=np.zeros(6), seed=k + n))
    # -- list entries: EPPK_NO_PICK behind, in the middle, everywhere; a pod twice; values outside [0, n_pods)
    rows = [[0, 1, NO, NO], [0, NO, 1, 2], [NO, NO, NO, NO], [0, 0, 1, 1], [0, 1, 2, 2], [NO, 0, NO, 0], [0, 1, 2, 3]]
    tags = ["trailing-no-pick", "middle-no-pick", "empty-list", "duplicate-pod"]
    out.append(_case("entries", tags, np.array(rows * 3, dtype=np.int32), 4, cap_all=2, policy=ref.SPILL, load=np.zeros(4)))
    out.append(_case("entries-chunks", tags, _spread(rows * 3, [i * (chunk // 4) + (i % 3) for i in range(21)], 4), 4, cap_all=2, load=np.zeros(4)))
    bad = np.array([[4, 0, 1], [-2, 1, 0], [0, 1 << 30, 2], [np.iinfo(np.int32).min, NO, 3], [0, 1, 2], [5, 6, 7]], dtype=np.int32)
    out.append(_case("out-of-range", ["out-of-range"], bad, 4, cap_all=1, policy=ref.SPILL, load=np.zeros(4)))
    out.append(_case("out-of-range-chunks", ["out-of-range"], _spread(bad.tolist(), [0, 63, 64, chunk - 1, chunk, 2 * chunk + 1], 3), 4, cap_all=1,
                     load=np.zeros(4)))
    # -- cascade: rows 0, 1 fill pod 0; row 2 is refused there, and its round-1 pod 1 has been filled by the round-0 acceptances of rows 3, 4
    rows = [[0, 1, 2], [0, 1, 2], [0, 1, 2], [1, 2, 0], [1, 2, 0], [1, 0, NO]]
    out.append(_case("cascade", ["cascade"], np.array(rows, dtype=np.int32), 3, cap_all=2, load=np.zeros(3)))
    out.append(_case("cascade-chunks", ["cascade"], _spread(rows, [1, 64, chunk - 1, chunk, chunk + 70, 3 * chunk], 3), 3, cap_all=2, policy=ref.SPILL,
                     load=np.zeros(3)))
    # -- loads handed in above the cap; a load of 2^32 - 1 that takes a spilled request wraps to 0
    lists = _random_lists(rng, chunk + 30, 3, 4)
    out.append(_case("load-above-cap", ["load-above-cap"], lists, 4, cap=[5, 9, 2, 6], load=[7, 1, 2, 100]))
    out.append(_case("load-above-cap-one", ["load-above-cap"], lists[:33], 4, cap=[5, 9, 2, 6], load=[7, 1, 2, 100], policy=ref.SPILL))
    for n in (3, chunk + 3):
        lists = np.full((n, 2), NO, dtype=np.int32)
        lists[n - 1] = [1, NO]
        lists[0] = [0, 1]
        out.append(_case(f"load-wraps-n{n}", ["load-wraps", "load-above-cap"], lists, 2, cap_all=0xFFFFFFFF, load=[0xFFFFFFFE, 0xFFFFFFFF], policy=ref.SPILL))
    # -- a cap per pod against one cap for all; outputs and loads the caller does not ask for
    for n in (90, 2 * chunk + 11):
        lists = _random_lists(rng, n, 4, 9)
        caps = rng.integers(0, max(2, n // 6), size=9)
        out.append(_case(f"cap-array-n{n}", ["cap-array"], lists, 9, cap=caps, load=rng.integers(0, 4, size=9), policy=ref.SPILL, seed=n))
        out.append(_case(f"cap-all-n{n}", ["cap-array"], lists, 9, cap_all=int(caps.max()), load=np.zeros(9), seed=n))
        out.append(_case(f"null-load-n{n}", ["null-load"], lists, 9, cap=caps, policy=ref.SPILL, seed=n))
        out.append(_case(f"null-score-n{n}", ["null-score"], lists, 9, cap=caps, load=np.zeros(9), no_score=True, seed=n))
        out.append(_case(f"null-rank-n{n}", ["null-rank"], lists, 9, cap=caps, load=np.zeros(9), no_rank=True, policy=ref.SPILL, seed=n))
        out.append(_case(f"null-list-scores-n{n}", ["null-score"], lists, 9, cap=caps, load=np.zeros(9), scores=None, seed=n))
    # -- seeded random: few pods, many requests
    for i in range(8):
        P = int(rng.integers(2, 24))
        n = int(rng.integers(1, 4 * chunk + 100)) if i < 6 else int(rng.integers(1, chunk + 1))
        k = int(rng.integers(1, 9))
        lists = _random_lists(rng, n, k, P, p_no=float(rng.random()) * 0.3, hot=int(rng.integers(0, P)))
        caps = rng.integers(0, 2 * max(1, n // P), size=P)
        out.append(_case(f"random-{i}", ["random"], lists, P, cap=caps, load=rng.integers(0, 5, size=P), policy=i & 1, seed=1000 + i))
    return out
