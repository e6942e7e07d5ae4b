"""Inputs for the banded resolve (SEMANTICS.md §3e): the smallest shapes that can break it, placed by the chunk size of the context under
test (BatchedPicker.bounded_geometry), and seeded random cases with few pods, so that most rounds of most bands are contended.

A case is a dict: name, tags (what it covers: tests/test_banded_ref_cpu.py holds the generator to the list in REQUIRED), lists [R, k] i32,
scores [R, k] f64 (or None), n_pods, bands [(policy, reserve)], band (u8 [R] or None), cap (u32 [n_pods] or None), cap_all, load (u32
[n_pods] or None), and the outputs the caller does NOT ask for: no_score, no_rank.  A case tagged `order-matters` has an answer that
differs from the plain bounded resolve's on the same lists: a device that ignored the band bytes would fail it."""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("banded_ref")
bc = _load("bounded_cases")
SEED0 = 0xBA2D
NO, SHED, SPILL = ref.NO_PICK, ref.SHED, ref.SPILL

REQUIRED = (
    ["n=0", "n=1", "n=63", "n=64", "n=65", "n=chunk-1", "n=chunk", "n=chunk+1", "n=3chunk+7"] +
    [f"{form}-{nb}-bands" for form in ("one-launch", "chunked") for nb in (2, 3, 8)] +
    ["interleaved-trip", "boundary-at-64", "boundary-at-chunk", "band-of-chunk", "band-of-chunk+1", "empty-first", "empty-middle", "empty-last",
     "all-in-last", "stable-3chunk-apart", "pods=1", "pods=65", "pods=4096", "last-pod", "reserve>=cap", "reserve-0", "load-above-cap-b",
     "spill-over-shed", "shed-over-spill", "spill-then-later-bid", "bad-band-alone-in-chunk", "bad-band-between", "k=1", "k=8", "null-band",
     "null-load", "null-score", "null-rank", "load-wraps", "random", "order-matters"])


def _case(name, tags, lists, n_pods, bands, band, cap_all=0, cap=None, load=None, scores="random", no_score=False, no_rank=False, seed=0):
    lists = np.ascontiguousarray(lists, dtype=np.int32)
    assert lists.ndim == 2
    if isinstance(scores, str):
        scores = bc._scores(np.random.default_rng(SEED0 + seed + lists.size), lists.shape)
    return dict(name=name, tags=set(tags), lists=lists, scores=scores, n_pods=int(n_pods), bands=[(int(p), int(r)) for p, r in bands],
                band=None if band is None else np.ascontiguousarray(band, dtype=np.uint8),
                cap=None if cap is None else np.ascontiguousarray(cap, dtype=np.uint32), cap_all=int(cap_all),
                load=None if load is None else np.ascontiguousarray(load, dtype=np.uint32), no_score=no_score, no_rank=no_rank)


def _table(rng, n_bands, top):
    """n_bands entries with mixed policies and non-decreasing reserves up to about `top`."""
    reserves = np.sort(rng.integers(0, max(1, top) + 1, size=n_bands))
    return [(int(rng.integers(0, 2)), int(r)) for r in reserves]


def want(c):
    """The restatement's answer for a case: (pick, score, rank, load_out, launch-status flags)."""
    return ref.resolve(c["lists"], c["scores"], c["n_pods"], c["bands"], c["band"], c["cap"], c["cap_all"], c["load"])


def host_ok(c):
    """False: a band byte >= n_bands -- the host-buffer forms refuse the batch, only the *_device forms take it."""
    return c["band"] is None or not np.any(c["band"] >= len(c["bands"]))


def info(c):
    return f"{c['name']} (R {c['lists'].shape[0]} k {c['lists'].shape[1]} pods {c['n_pods']} bands {c['bands']})"


def operator_case():
    """One slot per pod, SHED; rows 0-1 sheddable (band 1), rows 2-3 critical (band 0).  Batch order gives [0, -1, -1, 1]; the bands
    give [-1, -1, 0, 1]."""
    return np.array([[0, 1], [0, 1], [0, 1], [1, 0]], dtype=np.int32), np.array([1, 1, 0, 0], dtype=np.uint8)


def make_cases(chunk):
    """Every case, for a context whose chunk holds `chunk` rows (a power of two >= 64; the one-launch kernel takes up to `chunk` rows)."""
    rng = np.random.default_rng(SEED0 + chunk)
    out = []
    form = lambda n: "one-launch" if n <= chunk else "chunked"          # noqa: E731
    # -- batch sizes around a trip, a chunk, and several chunks with a ragged end; few pods, every round contended
    sizes = [("0", 0), ("1", 1), ("63", 63), ("64", 64), ("65", 65), ("chunk-1", chunk - 1), ("chunk", chunk), ("chunk+1", chunk + 1),
             ("3chunk+7", 3 * chunk + 7)]
    for i, (label, n) in enumerate(sizes):
        P, nb = 7, (2, 3, 8)[i % 3]
        out.append(_case(f"size-{label}", [f"n={label}", f"{form(n)}-{nb}-bands"], bc._random_lists(rng, n, 3, P), P, _table(rng, nb, n // 24),
                         rng.integers(0, nb, size=n), cap_all=max(1, n // 12), load=rng.integers(0, 3, size=P), seed=i))
    # -- 2, 3 and 8 bands through the one-launch and the chunked form
    for nb in (2, 3, 8):
        for n in (50, 2 * chunk + 9):
            P = 6
            out.append(_case(f"bands-{nb}-n{n}", [f"{form(n)}-{nb}-bands"], bc._random_lists(rng, n, 4, P), P, _table(rng, nb, n // 20),
                             rng.integers(0, nb, size=n), cap_all=max(2, n // 8), load=np.zeros(P), seed=nb + n))
    # -- bands interleaved inside one 64-row trip
    for n in (64, chunk + 64):
        out.append(_case(f"interleaved-n{n}", ["interleaved-trip"], bc._random_lists(rng, n, 3, 5), 5, [(SHED, 0), (SPILL, 1), (SHED, 3)],
                         np.arange(n) % 3, cap_all=max(4, n // 10), load=np.zeros(5), seed=n))
    # -- a band boundary exactly at place 64 and at place `chunk` of the band order; a band of exactly chunk and chunk + 1 rows
    for in_band0, n, tags in ((64, chunk + 40, ["boundary-at-64"]), (chunk, 2 * chunk + 5, ["boundary-at-chunk", "band-of-chunk"]),
                              (chunk + 1, 2 * chunk + 5, ["band-of-chunk+1"])):
        band = np.ones(n, dtype=np.uint8)
        band[rng.permutation(n)[:in_band0]] = 0
        out.append(_case(f"band0-of-{in_band0}-n{n}", tags, bc._random_lists(rng, n, 2, 4), 4, [(SHED, 0), (SHED, 2)], band, cap_all=n // 6,
                         load=np.zeros(4), seed=in_band0 + n))
    # -- an empty first, middle and last band; all rows in the last band
    for n in (40, chunk + 30):
        lists = bc._random_lists(rng, n, 3, 5)
        out.append(_case(f"empty-first-middle-n{n}", ["empty-first", "empty-middle"], lists, 5, [(SHED, 0), (SPILL, 0), (SHED, 1), (SHED, 2)],
                         rng.choice([1, 3], size=n), cap_all=max(3, n // 9), load=np.zeros(5), seed=n))
        out.append(_case(f"empty-last-n{n}", ["empty-last"], lists, 5, [(SPILL, 0), (SHED, 1), (SHED, 1)], rng.integers(0, 2, size=n),
                         cap_all=max(3, n // 9), load=np.zeros(5), seed=n + 1))
        out.append(_case(f"all-in-last-n{n}", ["all-in-last"], lists, 5, [(SHED, 0), (SHED, 0), (SPILL, 2)], np.full(n, 2), cap_all=max(3, n // 9),
                         load=np.zeros(5), seed=n + 2))
    # -- two rows of one band 3 * chunk apart bid for one slot (the order is stable across chunks); a band-0 row between them bids elsewhere
    n = 3 * chunk + 2
    lists = np.full((n, 2), NO, dtype=np.int32)
    lists[1], lists[3 * chunk + 1], lists[2 * chunk] = [0, NO], [0, NO], [1, 0]
    band = np.ones(n, dtype=np.uint8)
    band[2 * chunk] = 0
    out.append(_case("stable", ["stable-3chunk-apart"], lists, 2, [(SHED, 0), (SHED, 0)], band, cap_all=1, load=np.zeros(2)))
    # -- pod counts around a mask word and the largest snapshot; the last pod takes bids of both bands on both sides of a chunk boundary
    for P in (1, 65, 4096):
        lists = bc._random_lists(rng, 2 * chunk + 3, 2, P, hot=P - 1)
        band = rng.integers(0, 2, size=lists.shape[0])
        out.append(_case(f"pods-{P}", [f"pods={P}", "last-pod"], lists, P, [(SPILL, 0), (SHED, 2)], band, cap_all=5, load=np.zeros(P), seed=P))
        out.append(_case(f"pods-{P}-one-launch", [f"pods={P}", "last-pod"], lists[:61], P, [(SHED, 1), (SPILL, 2)], band[:61], cap_all=5,
                         load=np.zeros(P), seed=P + 1))
    # -- reserves: at or above the cap (the band gets nothing: its policy decides), and 0, 0, ...
    for n in (45, chunk + 21):
        lists = bc._random_lists(rng, n, 3, 4)
        band = rng.integers(0, 3, size=n)
        out.append(_case(f"reserve-cap-n{n}", ["reserve>=cap"], lists, 4, [(SHED, 0), (SPILL, 6), (SHED, 0xFFFFFFFF)], band, cap_all=6, load=np.zeros(4), seed=n))
        out.append(_case(f"reserve-0-n{n}", ["reserve-0"], lists, 4, [(SHED, 0), (SPILL, 0), (SHED, 0)], band, cap=[6, 2, 9, 1], load=np.zeros(4), seed=n))
        # a load handed in above cap_1 = cap - 4 but below cap
        out.append(_case(f"load-above-cap-b-n{n}", ["load-above-cap-b"], lists, 4, [(SHED, 0), (SHED, 4)], band % 2, cap=[8, 9, 6, 7], load=[5, 6, 3, 7], seed=n))
        # SPILL above SHED and the reverse
        out.append(_case(f"spill-over-shed-n{n}", ["spill-over-shed"], lists, 4, [(SPILL, 0), (SHED, 1)], band % 2, cap_all=n // 10, load=np.zeros(4), seed=n))
        out.append(_case(f"shed-over-spill-n{n}", ["shed-over-spill"], lists, 4, [(SHED, 0), (SPILL, 1)], band % 2, cap_all=n // 10, load=np.zeros(4), seed=n))
    # -- band 0 spills onto pod 0, which band 1 then bids for (and finds full), one row per chunk
    rows = [[0, NO], [0, NO], [0, NO], [0, 1], [0, 1], [1, 0]]
    for name, at in (("one", list(range(6))), ("chunks", [3, 64, chunk - 1, chunk, chunk + 65, 2 * chunk + 1])):
        lists = bc._spread(rows, at, 2)
        band = np.ones(lists.shape[0], dtype=np.uint8)
        band[at[:3]] = 0
        out.append(_case(f"spill-then-bid-{name}", ["spill-then-later-bid"], lists, 2, [(SPILL, 0), (SHED, 0)], band, cap_all=2, load=np.zeros(2)))
    # -- a spill of band 0 carries a load past 2^32 - 1: the load wraps in what is handed back, band 1 finds no room there
    for n in (4, chunk + 4):
        lists = np.full((n, 2), NO, dtype=np.int32)
        lists[0], lists[1], lists[n - 2], lists[n - 1] = [0, NO], [0, NO], [0, 1], [1, NO]
        band = np.ones(n, dtype=np.uint8)
        band[:2] = 0
        out.append(_case(f"load-wraps-n{n}", ["load-wraps"], lists, 2, [(SPILL, 0), (SPILL, 0)], band, cap_all=0xFFFFFFFF, load=[0xFFFFFFFE, 0xFFFFFFFE]))
    # -- a band byte >= n_bands (the *_device forms): alone in its chunk, and between valid rows; its list is still checked
    for n, at, tag in ((chunk + 1, chunk, "bad-band-alone-in-chunk"), (20, 5, "bad-band-between"), (2 * chunk + 20, chunk + 5, "bad-band-between")):
        lists = bc._random_lists(rng, n, 3, 4)
        band = rng.integers(0, 2, size=n).astype(np.uint8)
        band[at] = 2 if n != 20 else 255
        out.append(_case(f"bad-band-n{n}", [tag], lists, 4, [(SHED, 0), (SPILL, 1)], band, cap_all=max(2, n // 10), load=np.zeros(4), seed=n))
        lists = lists.copy()
        lists[at] = [0, 9, 1]
        out.append(_case(f"bad-band-bad-pick-n{n}", [tag], lists, 4, [(SHED, 0), (SPILL, 1)], band, cap_all=max(2, n // 10), load=np.zeros(4), seed=n))
    # -- list lengths
    for k in (1, 8):
        for n in (50, 2 * chunk + 1):
            out.append(_case(f"k{k}-n{n}", [f"k={k}"], bc._random_lists(rng, n, k, 6), 6, _table(rng, 3, 2), rng.integers(0, 3, size=n),
                             cap_all=max(3, n // 10), load=np.zeros(6), seed=k + n))
    # -- no band array; outputs and loads the caller does not ask for
    for n in (90, 2 * chunk + 11):
        lists = bc._random_lists(rng, n, 4, 9)
        caps = rng.integers(0, max(2, n // 6), size=9)
        band = rng.integers(0, 3, size=n)
        tab = [(SHED, 0), (SPILL, 1), (SHED, 2)]
        out.append(_case(f"null-band-n{n}", ["null-band"], lists, 9, [(SPILL, 1), (SHED, 2)], None, cap=caps, load=np.zeros(9), seed=n))
        out.append(_case(f"null-load-n{n}", ["null-load"], lists, 9, tab, band, cap=caps, seed=n))
        out.append(_case(f"null-score-n{n}", ["null-score"], lists, 9, tab, band, cap=caps, load=np.zeros(9), no_score=True, seed=n))
        out.append(_case(f"null-rank-n{n}", ["null-rank"], lists, 9, tab, band, cap=caps, load=np.zeros(9), no_rank=True, seed=n))
        out.append(_case(f"null-list-scores-n{n}", ["null-score"], lists, 9, tab, band, cap=caps, load=np.zeros(9), scores=None, seed=n))
    # -- the operator's case (the batch-order answer sheds the critical rows), as it is and one row per chunk
    lists, band = operator_case()
    out.append(_case("operator", ["order-matters"], lists, 2, [(SHED, 0), (SHED, 0)], band, cap_all=1, load=np.zeros(2)))
    at = [5, 70, chunk + 1, 2 * chunk + 3]
    spread = np.zeros(at[-1] + 1, dtype=np.uint8)
    spread[at] = band
    out.append(_case("operator-chunks", ["order-matters"], bc._spread(lists.tolist(), at, 2), 2, [(SHED, 0), (SHED, 0)], spread, cap_all=1, load=np.zeros(2)))
    # -- seeded random: few pods, many requests, tight caps
    for i in range(8):
        P = int(rng.integers(2, 24))
        n = int(rng.integers(chunk + 1, 4 * chunk + 100)) if i < 5 else int(rng.integers(8, chunk + 1))
        k = int(rng.integers(1, 9))
        nb = int(rng.integers(1, 9))
        lists = bc._random_lists(rng, n, k, P, p_no=float(rng.random()) * 0.3, hot=int(rng.integers(0, P)))
        caps = rng.integers(1, 2 * max(1, n // P) + 1, size=P)
        out.append(_case(f"random-{i}", ["random"], lists, P, _table(rng, nb, int(caps.min())),
                         rng.integers(0, nb, size=n), cap=caps, load=rng.integers(0, 5, size=P), seed=1000 + i))
    return out
