"""Inputs for the costed resolve (SEMANTICS.md §3f): the smallest shapes that can break it, placed by the chunk size of the context under
test (BatchedPicker.bounded_geometry), and seeded random cases with few pods and mixed costs, so that most rounds are contended.

A case is a dict: the fields of tests/banded_cases.py (name, tags, lists, scores, n_pods, bands, band, cap, cap_all, load, no_score,
no_rank) and cost (u32 [R], or [R, k] with per_entry) and per_entry.  The tags say what a case is FOR; what actually happens in a case
-- where a taker boundary falls, which sums pass 2^32 -- is observed by the row-by-row loop of tests/test_costed_ref_cpu.py, which
holds the generator to SITUATIONS."""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("costed_ref")
bc = _load("bounded_cases")
SEED0 = 0xC057
NO, SHED, SPILL = ref.NO_PICK, ref.SHED, ref.SPILL
MAX_COST, FULL = ref.MAX_COST, ref.FULL

# what the generator's cases are for (every tag must be on a case) ...
REQUIRED = (
    [f"n={s}" for s in ("0", "1", "63", "64", "65", "127", "129", "chunk-1", "chunk", "chunk+1", "2chunk+3", "9chunk+5")] +
    [f"pods={p}" for p in (1, 2, 64, 65, 4096)] + [f"k={k}" for k in (1, 2, 4, 8)] + [f"bands={b}" for b in (1, 3, 8)] +
    ["all-one-pod", "64-pods-per-trip", "two-pods-alternating", "null-list-scores", "null-score", "null-rank", "null-cap", "null-load", "null-band",
     "per-entry", "random", "one-launch", "chunked"])
# ... and what has to HAPPEN in some case (observed, not declared: tests/test_costed_ref_cpu.py)
SITUATIONS = (
    "boundary-in-trip", "boundary-between-trips", "boundary-at-chunk", "boundary-at-chunk-of-ragged-segment", "ineligible-between-takers",
    "S+c==room", "S+c==room+1", "c==MAX", "2^32-in-trip", "2^32-in-chunk", "2^32-across-chunks", "load+takers==cap==FULL", "spill-wraps",
    "deferred-differs", "cost-0", "cost-MAX+1", "band>=n_bands", "bad-cost-behind-invalid-entry")


def _case(name, tags, lists, n_pods, cost, bands=((SHED, 0),), band=None, cap_all=0, cap=None, load=None, scores="random", no_score=False,
          no_rank=False, per_entry=False, seed=0):
    lists = np.ascontiguousarray(lists, dtype=np.int32)
    assert lists.ndim == 2
    cost = np.ascontiguousarray(cost, dtype=np.uint32)
    assert cost.shape == (lists.shape if per_entry else lists.shape[:1])
    if isinstance(scores, str):
        scores = bc._scores(np.random.default_rng(SEED0 + seed + lists.size), lists.shape)
    return dict(name=name, tags=set(tags), lists=lists, scores=scores, n_pods=int(n_pods), cost=cost, per_entry=bool(per_entry),
                bands=[(int(p), int(r)) for p, r in bands], band=None if band is None else np.ascontiguousarray(band, dtype=np.uint8),
                cap=None if cap is None else np.ascontiguousarray(cap, dtype=np.uint32), cap_all=int(cap_all),
                load=None if load is None else np.ascontiguousarray(load, dtype=np.uint32), no_score=no_score, no_rank=no_rank)


def _costs(rng, shape, top=4096):
    """Heavy-tailed costs in 1 .. top: most requests are small, a few are hundreds of times larger."""
    return np.clip(np.floor((rng.pareto(1.1, size=shape) + 1.0) * 2.0), 1, top).astype(np.uint32)


def _table(rng, n_bands, top):
    reserves = np.sort(rng.integers(0, max(1, top) + 1, size=n_bands))
    return [(int(rng.integers(0, 2)), int(r)) for r in reserves]


def want(c, **kw):
    """The restatement's answer for a case: (pick, score, rank, load_out, launch-status flags)."""
    return ref.resolve(c["lists"], c["scores"], c["n_pods"], c["cost"], c["bands"], c["band"], c["cap"], c["cap_all"], c["load"], c["per_entry"], **kw)


def host_ok(c):
    """False: per-entry costs, or a bad row -- the host-buffer forms take per-request costs and refuse a batch with a bad row."""
    return not c["per_entry"] and not ref.bad_rows(c["lists"], c["n_pods"], c["cost"], False, len(c["bands"]), c["band"]).any()


def unit_cost(c):
    """The case with every cost 1 (per request): what eppk_banded_resolve_device answers bit for bit."""
    return dict(c, cost=np.ones(c["lists"].shape[0], dtype=np.uint32), per_entry=False)


def info(c):
    return (f"{c['name']} (R {c['lists'].shape[0]} k {c['lists'].shape[1]} pods {c['n_pods']} bands {c['bands']}"
            f"{' per-entry' if c['per_entry'] else ''})")


def two_request_case():
    """§3f's example: one pod with cap 10.  Row 0 (band 0, SPILL) costs 20 and can never fit; row 1 (band 1, SHED) costs 10.  The rule
    -- ONE finish behind the last band -- gives row 1 the pod's room and then spills row 0 on top: picks [0, 0], load 30.  A finish
    inside band 0 would spill row 0 first (load 20 >= cap) and shed row 1."""
    return np.array([[0], [0]], dtype=np.int32), np.array([20, 10], dtype=np.uint32), np.array([0, 1], dtype=np.uint8), [(SPILL, 0), (SHED, 0)], 10


def make_cases(chunk):
    """Every case, for a context whose chunk holds `chunk` rows (a power of two >= 64; the one-launch kernel takes up to `chunk` rows)."""
    rng = np.random.default_rng(SEED0 + chunk)
    out = []
    form = lambda n: "one-launch" if n <= chunk else "chunked"          # noqa: E731
    # -- batch sizes around a trip, a chunk, and several chunks with a ragged end; few pods, every round contended
    sizes = [("0", 0), ("1", 1), ("63", 63), ("64", 64), ("65", 65), ("127", 127), ("129", 129), ("chunk-1", chunk - 1), ("chunk", chunk),
             ("chunk+1", chunk + 1), ("2chunk+3", 2 * chunk + 3), ("9chunk+5", 9 * chunk + 5)]
    for i, (label, n) in enumerate(sizes):
        P, nb, k = 7, (1, 3, 8)[i % 3], (1, 2, 4, 8)[i % 4]
        cost = _costs(rng, n, 64)
        out.append(_case(f"size-{label}", [f"n={label}", f"bands={nb}", f"k={k}", form(n)], bc._random_lists(rng, n, k, P), P, cost,
                         _table(rng, nb, 8), rng.integers(0, nb, size=n), cap_all=max(8, int(cost.sum()) // 10), load=rng.integers(0, 9, size=P), seed=i))
    # -- pod counts around a mask word and the largest snapshot; the last pod takes bids of both bands on both sides of a chunk boundary
    for P in (1, 2, 64, 65, 4096):
        lists = bc._random_lists(rng, 2 * chunk + 3, 2, P, hot=P - 1)
        n = lists.shape[0]
        cost = _costs(rng, n, 32)
        band = rng.integers(0, 2, size=n)
        out.append(_case(f"pods-{P}", [f"pods={P}"], lists, P, cost, [(SPILL, 0), (SHED, 5)], band, cap_all=40, load=np.zeros(P), seed=P))
        out.append(_case(f"pods-{P}-one-launch", [f"pods={P}"], lists[:61], P, cost[:61], [(SHED, 2), (SPILL, 9)], band[:61], cap_all=25, load=np.zeros(P),
                         seed=P + 1))
    # -- every row bids one pod, cost 2: the longest carry.  The cap puts the taker boundary inside a trip, between two trips, and at a
    #    chunk boundary; a band whose segment starts at place 37 has its chunk boundary where no multiple of the chunk is
    n = 3 * chunk + 7
    for label, takers in (("in-trip", 64 + 20), ("between-trips", 64), ("at-chunk", chunk), ("past-2-chunks", 2 * chunk + 1)):
        if takers < n:
            out.append(_case(f"one-pod-{label}", ["all-one-pod"], np.zeros((n, 1)), 3, np.full(n, 2), cap_all=2 * takers, load=np.zeros(3)))
    for label, takers in (("in-trip", 20), ("between-trips", 64)):
        out.append(_case(f"one-pod-{label}-one-launch", ["all-one-pod"], np.zeros((min(chunk, 100), 2)), 3, np.full(min(chunk, 100), 2), cap_all=2 * takers,
                         load=np.zeros(3)))
    n = 37 + 2 * chunk + 5
    band = np.ones(n, dtype=np.uint8)
    band[rng.permutation(n)[:37]] = 0
    out.append(_case("ragged-segment", ["all-one-pod"], band[:, None].astype(np.int32), 2, np.where(band == 0, 1, 2), [(SHED, 0), (SHED, 0)], band,
                     cap_all=2 * chunk, load=np.zeros(2)))
    # -- 64 distinct pods in every trip (64 trips of the ballot loop), and two pods on alternating lanes (the interleaved prefix)
    for P in (64, 65, 4096):
        for n in (64, 2 * chunk + 3):
            lists = np.stack([(np.arange(n) * 7 + 3) % 64 + (P - 64), (np.arange(n) + 1) % 64], axis=1)
            cost = _costs(rng, n, 16)
            out.append(_case(f"64-pods-P{P}-n{n}", ["64-pods-per-trip", f"pods={P}"], lists, P, cost, cap_all=max(6, int(cost.sum()) // 100),
                             load=np.zeros(P), seed=P + n))
    for n in (64, 127, 2 * chunk + 3):
        lists = np.stack([np.arange(n) % 2, (np.arange(n) + 1) % 2, np.full(n, 2)], axis=1)
        cost = rng.integers(1, 6, size=n)
        out.append(_case(f"alternating-n{n}", ["two-pods-alternating"], lists, 3, cost, [(SHED, 0), (SPILL, 3), (SHED, 4)], rng.integers(0, 3, size=n),
                         cap_all=max(9, int(cost.sum()) // 5), load=np.zeros(3), seed=n))
    # -- room 10: a request of 50 between takers (it could not fit alone: no bidder, it counts for nothing), S + c == room, == room + 1;
    #    side by side, and one row per trip and per chunk
    rows, costs = [[0], [0], [0], [0], [0], [0]], [3, 50, 3, 4, 1, 1]
    for name, at in (("one", list(range(6))), ("spread", [3, 64, 70, chunk, chunk + 65, 2 * chunk + 1])):
        lists = bc._spread(rows, at, 1)
        cost = np.ones(lists.shape[0], dtype=np.uint32)
        cost[at] = costs
        out.append(_case(f"exact-fit-{name}", ["all-one-pod"], lists, 1, cost, cap_all=10, load=np.zeros(1)))
    # -- cap 2^32 - 1, costs of EPPK_MAX_COST: the bidders' sum passes 2^32 at bidder 256 -- inside a trip (behind 20 requests of cost 1),
    #    between two trips, and between two chunks; 256 of them fit, the load ends at 0xFFFFFF00 + the small ones
    lead = chunk - 255 if chunk >= 512 else chunk if chunk < 256 else 0     # behind `lead` small ones bidder 256 (or 255) is first in its chunk
    for name, ones, n in (("in-trip", 20, 300), ("between-trips", 0, 300), ("between-chunks", lead, lead + 300)):
        cost = np.full(n, MAX_COST, dtype=np.uint32)
        cost[:ones] = 1
        out.append(_case(f"pass-2^32-{name}", ["all-one-pod"], np.zeros((n, 1)), 2, cost, cap_all=FULL, load=np.zeros(2)))
    # -- load + takers == cap == 2^32 - 1, and the next request misses by one
    out.append(_case("fills-to-full", ["all-one-pod"], np.zeros((4, 1)), 1, [4, 6, 1, 1], [(SPILL, 0)], cap_all=FULL, load=[FULL - 10]))
    for n in (5, chunk + 9):
        lists = np.full((n, 2), NO, dtype=np.int32)
        lists[0], lists[1], lists[n - 2], lists[n - 1] = [0, NO], [0, NO], [NO, 0], [1, 0]
        cost = np.ones(n, dtype=np.uint32)
        cost[[0, 1, n - 2, n - 1]] = [6, 0x100, MAX_COST, 3]
        # row 0 fills pod 0 to FULL - 4; row 1 (0x100) and row n-2 (MAX_COST) cannot fit and spill: the load wraps twice over
        out.append(_case(f"spill-wraps-n{n}", [], lists, 2, cost, [(SPILL, 0), (SPILL, 0)], np.arange(n) % 2, cap_all=FULL, load=[FULL - 10, FULL - 1]))
    # -- §3f's example: the deferred finish and a finish per band differ; as it is and with the rows three chunks apart
    lists, cost, band, table, cap = two_request_case()
    out.append(_case("two-requests", [], lists, 1, cost, table, band, cap_all=cap, load=np.zeros(1)))
    at = [70, 3 * chunk + 1]
    wide = np.zeros(at[-1] + 1, dtype=np.uint8)
    wide[at] = band
    wcost = np.ones(at[-1] + 1, dtype=np.uint32)
    wcost[at] = cost
    out.append(_case("two-requests-chunks", [], bc._spread(lists.tolist(), at, 1), 1, wcost, table, wide, cap_all=cap, load=np.zeros(1)))
    # -- bad rows (the *_device forms): cost 0, cost EPPK_MAX_COST + 1, 2^32 - 1, a band byte >= n_bands; between valid rows and alone in a chunk;
    #    the row takes no room, its list is still checked
    for n, at in ((20, 5), (chunk + 1, chunk), (2 * chunk + 20, chunk + 5)):
        lists = bc._random_lists(rng, n, 3, 4)
        band = rng.integers(0, 2, size=n).astype(np.uint8)
        for label, value in (("0", 0), ("max+1", MAX_COST + 1), ("full", FULL)):
            cost = _costs(rng, n, 8)
            cost[at] = value
            out.append(_case(f"bad-cost-{label}-n{n}", [], lists, 4, cost, [(SHED, 0), (SPILL, 2)], band, cap_all=max(6, n // 3), load=np.zeros(4), seed=n))
        cost = _costs(rng, n, 8)
        bad_band = band.copy()
        bad_band[at] = 2 if n != 20 else 255
        out.append(_case(f"bad-band-n{n}", [], lists, 4, cost, [(SHED, 0), (SPILL, 2)], bad_band, cap_all=max(6, n // 3), load=np.zeros(4), seed=n))
        bad_list = lists.copy()
        bad_list[at] = [0, 9, 1]
        cost[at] = 0
        out.append(_case(f"bad-cost-bad-pick-n{n}", [], bad_list, 4, cost, [(SHED, 0), (SPILL, 2)], band, cap_all=max(6, n // 3), load=np.zeros(4), seed=n))
    # -- per-entry costs: random; a bad cost behind an invalid entry alone (the row is NOT bad) and at a valid one (it is)
    for n in (50, 129, 2 * chunk + 3):
        for k in (2, 4):
            lists = bc._random_lists(rng, n, k, 6, p_no=0.2)
            cost = _costs(rng, (n, k), 32)
            tab = [(SHED, 0), (SPILL, 4), (SHED, 6)]
            band = rng.integers(0, 3, size=n)
            out.append(_case(f"per-entry-n{n}-k{k}", ["per-entry", f"k={k}", "bands=3"], lists, 6, cost, tab, band, cap_all=max(12, int(cost.sum()) // 24),
                             load=np.zeros(6), per_entry=True, seed=n + k))
            lists, cost = lists.copy(), cost.copy()
            lists[n // 2, 0], cost[n // 2, 0] = NO, 0                 # invalid entry, cost 0: not looked at
            lists[n // 3, 1], cost[n // 3, 1] = 77, MAX_COST + 1      # out of range (EPPK_LAUNCH_BAD_PICK), cost too large: not looked at either
            out.append(_case(f"per-entry-behind-invalid-n{n}-k{k}", ["per-entry"], lists, 6, cost, tab, band, cap_all=max(12, int(cost.sum()) // 24),
                             load=np.zeros(6), per_entry=True, seed=n + k))
            lists, cost = lists.copy(), cost.copy()
            lists[n - 1, k - 1], cost[n - 1, k - 1] = 2, 0            # a valid entry with cost 0: the row is bad, whichever entry it would take
            out.append(_case(f"per-entry-bad-n{n}-k{k}", ["per-entry"], lists, 6, cost, tab, band, cap_all=max(12, int(cost.sum()) // 24),
                             load=np.zeros(6), per_entry=True, seed=n + k))
    # -- no band array; outputs, caps and loads the caller does not ask for
    for n in (90, 2 * chunk + 11):
        lists = bc._random_lists(rng, n, 4, 9)
        cost = _costs(rng, n, 64)
        caps = rng.integers(0, max(8, int(cost.sum()) // 14), size=9)
        band = rng.integers(0, 3, size=n)
        tab = [(SHED, 0), (SPILL, 3), (SHED, 7)]
        out.append(_case(f"null-band-n{n}", ["null-band"], lists, 9, cost, [(SPILL, 1)], None, cap=caps, load=np.zeros(9), seed=n))
        out.append(_case(f"null-load-n{n}", ["null-load"], lists, 9, cost, tab, band, cap=caps, seed=n))
        out.append(_case(f"null-cap-n{n}", ["null-cap"], lists, 9, cost, tab, band, cap_all=int(cost.sum()) // 20, load=np.zeros(9), seed=n))
        out.append(_case(f"null-score-n{n}", ["null-score"], lists, 9, cost, tab, band, cap=caps, load=np.zeros(9), no_score=True, seed=n))
        out.append(_case(f"null-rank-n{n}", ["null-rank"], lists, 9, cost, tab, band, cap=caps, load=np.zeros(9), no_rank=True, seed=n))
        out.append(_case(f"null-list-scores-n{n}", ["null-list-scores"], lists, 9, cost, tab, band, cap=caps, load=np.zeros(9), scores=None, seed=n))
    # -- seeded random: few pods, many requests, heavy-tailed costs, caps of a few mean costs
    for i in range(8):
        P = int(rng.integers(2, 24))
        n = int(rng.integers(chunk + 1, 4 * chunk + 100)) if i < 5 else int(rng.integers(8, chunk + 1))
        k = int(rng.integers(1, 9))
        nb = int(rng.integers(1, 9))
        lists = bc._random_lists(rng, n, k, P, p_no=float(rng.random()) * 0.3, hot=int(rng.integers(0, P)))
        per_entry = i % 4 == 3
        cost = _costs(rng, (n, k) if per_entry else n)
        caps = rng.integers(1, 2 * max(1, int(cost.mean()) * n // P) + 1, size=P)
        out.append(_case(f"random-{i}", ["random"] + (["per-entry"] if per_entry else []), lists, P, cost, _table(rng, nb, int(caps.min())),
                         rng.integers(0, nb, size=n), cap=caps, load=rng.integers(0, 40, size=P), per_entry=per_entry, seed=1000 + i))
    return out
