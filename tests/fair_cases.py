"""Inputs for the fair resolve (SEMANTICS.md §3g): the smallest shapes that can break the fair order, placed by the chunk size of the
context under test (BatchedPicker.bounded_geometry), and seeded random cases with few pods, so that most rounds are contended and the
order decides who is placed.

A case is a dict: the fields of tests/costed_cases.py (name, lists, scores, n_pods, cost, per_entry, bands, band, cap, cap_all, load,
no_score, no_rank) with cost None for "every cost 1", and flow (u16 [R] or None) and n_flows.  What a case is FOR is not declared:
coverage() reads from the cases themselves (and from the restatement's answers) which of the REQUIRED situations occur, and
tests/test_fair_ref_cpu.py holds the generator to all of them."""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("fair_ref")
bc = _load("bounded_cases")
SEED0 = 0xFA12
NO, SHED, SPILL = ref.NO_PICK, ref.SHED, ref.SPILL
MAX_COST, MAX_FLOWS = ref.MAX_COST, ref.MAX_FLOWS

# every situation the corpus must contain (observed by coverage(), not declared)
REQUIRED = (
    ["pair-in-one-trip", "pair-in-adjacent-trips", "pair-in-different-chunks", "trip-of-64-distinct-flows", "trip-of-one-flow",
     "flow-gap", "flow-with-one-row", "flow=n_flows-1", "bad-flow=n_flows-good-band", "bad-flow=0xFFFF-good-band", "bad-band-good-flow",
     "bad-cost-holds-a-turn", "same-flow-in-two-bands-different-counts", "band-ends-mid-chunk", "empty-band-between-used",
     "q==cnt-of-lower-flow", "q==cnt-1-of-lower-flow", "q==cnt-of-higher-flow", "q==cnt-1-of-higher-flow",
     "null-flow", "null-cost", "null-load", "null-score", "null-rank", "null-band"] +
    [f"n_flows={n}:{side}" for n in (1, 2, 1024) for side in ("rows<flows", "rows>flows")] +
    [f"R={s}" for s in ("0", "1", "63", "64", "65", "chunk", "chunk+1")])


def _case(name, lists, n_pods, flow, n_flows, cost, bands=((SHED, 0),), band=None, cap_all=0, cap=None, load=None, scores="random", no_score=False,
          no_rank=False, seed=0):
    lists = np.ascontiguousarray(lists, dtype=np.int32)
    assert lists.ndim == 2
    if isinstance(scores, str):
        scores = bc._scores(np.random.default_rng(SEED0 + seed + lists.size), lists.shape)
    return dict(name=name, lists=lists, scores=scores, n_pods=int(n_pods), flow=None if flow is None else np.ascontiguousarray(flow, dtype=np.uint16),
                n_flows=int(n_flows), cost=None if cost is None else np.ascontiguousarray(cost, dtype=np.uint32), per_entry=False,
                bands=[(int(p), int(r)) for p, r in bands], band=None if band is None else np.ascontiguousarray(band, dtype=np.uint8),
                cap=None if cap is None else np.ascontiguousarray(cap, dtype=np.uint32), cap_all=int(cap_all),
                load=None if load is None else np.ascontiguousarray(load, dtype=np.uint32), no_score=no_score, no_rank=no_rank)


def _costs(rng, n, top=64):
    return np.clip(np.floor((rng.pareto(1.1, size=n) + 1.0) * 2.0), 1, top).astype(np.uint32)


def _table(rng, n_bands, top):
    reserves = np.sort(rng.integers(0, max(1, top) + 1, size=n_bands))
    return [(int(rng.integers(0, 2)), int(r)) for r in reserves]


def want(c):
    """The restatement's answer for a case: (pick, score, rank, load_out, launch-status flags)."""
    return ref.resolve(c["lists"], c["scores"], c["n_pods"], c["flow"], c["n_flows"], c["cost"], c["bands"], c["band"], c["cap"], c["cap_all"], c["load"])


def info(c):
    return (f"{c['name']} (R {c['lists'].shape[0]} k {c['lists'].shape[1]} pods {c['n_pods']} flows {c['n_flows']} bands {c['bands']}"
            f"{' no cost' if c['cost'] is None else ''})")


def tenant_case():
    """§3g's example: one pod with cap 6, k = 1, SHED, cost 1; rows 0-8 of flow 0, 9-11 of flow 1, 12-14 of flow 2.  Batch order gives
    the flows 6 / 0 / 0 slots; the fair order gives 2 / 2 / 2: rows 0, 1, 9, 10, 12 and 13."""
    flow = np.array([0] * 9 + [1] * 3 + [2] * 3, dtype=np.uint16)
    return np.zeros((15, 1), dtype=np.int32), flow, 3, 6, [0, 1, 9, 10, 12, 13]


def heavy_flows(rng, n, n_flows, share=1.0 / 3.0):
    """Flow ids drawn heavy-tailed: flow 0 holds about `share` of the rows, the others follow a Zipf-like tail."""
    if n_flows == 1:
        return np.zeros(n, dtype=np.uint16)
    w = 1.0 / np.arange(1, n_flows, dtype=np.float64)
    p = np.concatenate([[share], (1.0 - share) * w / w.sum()])
    return rng.choice(n_flows, size=n, p=p).astype(np.uint16)


def _contended(rng, n, k, P, cost):
    """(lists, cap_all): few pods, one of them hot, room for about a third of the batch."""
    lists = bc._random_lists(rng, n, k, P, p_no=0.1, hot=int(rng.integers(0, P)))
    total = n if cost is None else int(np.asarray(cost, dtype=np.int64).sum())
    return lists, max(2, total // (3 * P))


def make_cases(chunk):
    """Every case, for a context whose chunk holds `chunk` rows (a power of two >= 64)."""
    rng = np.random.default_rng(SEED0 + chunk)
    out = []
    # -- batch sizes around a trip and a chunk; three flows, so that every trip holds pairs of one flow
    for i, n in enumerate((0, 1, 63, 64, 65, chunk, chunk + 1)):
        P, nb, k = 5, (1, 3, 8)[i % 3], (1, 2, 4, 8)[i % 4]
        cost = _costs(rng, n) if i % 2 else None
        lists, cap_all = _contended(rng, n, k, P, cost)
        out.append(_case(f"size-{n}", lists, P, rng.integers(0, 3, size=n), 3, cost, _table(rng, nb, 2), rng.integers(0, nb, size=n), cap_all=cap_all,
                         load=rng.integers(0, 3, size=P), seed=i))
    # -- n_flows 1, 2 and 1 024 with fewer rows than flows and with more (R = 0 is the only batch with fewer rows than one flow)
    for n_flows, n in ((1, 0), (1, 100), (2, 1), (2, 200), (1024, 300), (1024, 1100)):
        cost = _costs(rng, n)
        lists, cap_all = _contended(rng, n, 2, 7, cost)
        flow = rng.integers(0, n_flows, size=n)
        if n:
            flow[n // 2] = n_flows - 1
        out.append(_case(f"flows-{n_flows}-n{n}", lists, 7, flow, n_flows, cost, [(SHED, 0), (SPILL, 1)], rng.integers(0, 2, size=n), cap_all=cap_all,
                         load=np.zeros(7), seed=n_flows + n))
    # -- 64 distinct flows in every trip (64 trips of the ballot loop), one flow per trip (the longest carry), flow ids with gaps
    n = 2 * chunk + 3 if chunk <= 512 else chunk + 67
    lists, cap_all = _contended(rng, n, 2, 3, None)
    out.append(_case("64-flows-per-trip", lists, 3, (np.arange(n) * 7 + 3) % 64, 64, None, cap_all=cap_all, load=np.zeros(3)))
    n = chunk + 70
    lists, cap_all = _contended(rng, n, 2, 3, None)
    out.append(_case("one-flow-per-trip", lists, 3, np.array([0, 2, 4])[(np.arange(n) // 64) % 3], 6, _costs(rng, n, 4), cap_all=3 * cap_all, load=np.zeros(3)))
    out.append(_case("all-one-flow-of-many", lists, 3, np.full(n, 700), 1024, None, [(SHED, 0), (SHED, 2)], (np.arange(n) // 100) % 2, cap_all=cap_all,
                     load=np.zeros(3)))
    # -- §3g's example, as it is and with the rows spread over three chunks
    lists, flow, n_flows, cap, _ = tenant_case()
    out.append(_case("tenants", lists, 1, flow, n_flows, None, cap_all=cap, load=np.zeros(1)))
    at = np.sort(rng.permutation(2 * chunk + 40)[:15])
    wide_flow = np.zeros(at[-1] + 1, dtype=np.uint16)
    wide_flow[at] = flow
    out.append(_case("tenants-chunks", bc._spread(lists.tolist(), list(at), 1), 1, wide_flow, n_flows, np.ones(at[-1] + 1), cap_all=cap, load=np.zeros(1)))
    # -- rows that are not in the order: flow = n_flows and 0xFFFF under a good band, a bad band under a good flow; between good rows and
    #    behind a chunk boundary; the row takes no room and no turn, its list is still checked
    n = chunk + 20
    for label, cost in (("costed", _costs(rng, n, 8)), ("counted", None)):
        lists, cap_all = _contended(rng, n, 3, 4, cost)
        flow, band = rng.integers(0, 7, size=n), rng.integers(0, 2, size=n)
        flow[5], flow[chunk + 3] = 7, 0xFFFF
        band[9], band[chunk + 7], band[5] = 2, 255, 1
        lists[5] = [0, 9, 1]                                               # (EPPK_LAUNCH_BAD_PICK from a row that is not in the order)
        out.append(_case(f"bad-rows-{label}", lists, 4, flow, 7, cost, [(SHED, 0), (SPILL, 1)], band, cap_all=cap_all, load=np.zeros(4)))
    # -- a bad cost holds its turn: everybody else fits, so the rows behind it in its flow are takers; one inside a trip, one behind a chunk
    n = chunk + 66
    cost = _costs(rng, n, 8)
    cost[3], cost[chunk + 1], cost[70] = 0, MAX_COST + 1, 0xFFFFFFFF
    out.append(_case("bad-cost-holds-turn", bc._random_lists(rng, n, 2, 6), 6, rng.integers(0, 4, size=n), 4, cost, [(SHED, 0), (SHED, 0)],
                     rng.integers(0, 2, size=n), cap_all=int(cost[cost <= MAX_COST].sum()), load=np.zeros(6)))
    # -- an empty band between two used ones, a band that ends mid-chunk, the same flow in two bands
    n = 2 * chunk + 37
    lists, cap_all = _contended(rng, n, 4, 6, None)
    out.append(_case("empty-band", lists, 6, rng.integers(0, 5, size=n), 5, None, [(SPILL, 0), (SHED, 1), (SHED, 2)], rng.choice([0, 2], size=n, p=[0.3, 0.7]),
                     cap_all=cap_all, load=np.zeros(6)))
    # -- no flow array, no cost array, no band array; outputs and loads the caller does not ask for
    for n in (90, chunk + 11):
        cost = _costs(rng, n)
        lists, cap_all = _contended(rng, n, 4, 9, cost)
        flow, band, tab = heavy_flows(rng, n, 6), rng.integers(0, 3, size=n), [(SHED, 0), (SPILL, 3), (SHED, 7)]
        caps = rng.integers(1, 2 * cap_all, size=9)
        out.append(_case(f"null-flow-n{n}", lists, 9, None, 6, cost, tab, band, cap=caps, load=np.zeros(9), seed=n))
        out.append(_case(f"null-cost-n{n}", lists, 9, flow, 6, None, tab, band, cap_all=max(2, n // 27), load=np.zeros(9), seed=n))
        out.append(_case(f"null-flow-null-cost-n{n}", lists, 9, None, 1, None, tab, band, cap_all=max(2, n // 27), load=np.zeros(9), seed=n))
        out.append(_case(f"null-band-n{n}", lists, 9, flow, 6, cost, [(SPILL, 1)], None, cap=caps, load=np.zeros(9), seed=n))
        out.append(_case(f"null-load-n{n}", lists, 9, flow, 6, cost, tab, band, cap=caps, seed=n))
        out.append(_case(f"null-score-n{n}", lists, 9, flow, 6, cost, tab, band, cap=caps, load=np.zeros(9), no_score=True, seed=n))
        out.append(_case(f"null-rank-n{n}", lists, 9, flow, 6, cost, tab, band, cap=caps, load=np.zeros(9), no_rank=True, seed=n))
        out.append(_case(f"null-list-scores-n{n}", lists, 9, flow, 6, cost, tab, band, cap=caps, load=np.zeros(9), scores=None, seed=n))
    # -- seeded random: few pods, heavy-tailed flows and costs, caps of a few mean costs
    for i in range(10):
        P = int(rng.integers(1, 65)) if i % 3 else int(rng.integers(1, 6))
        n = int(rng.integers(chunk + 1, min(2 * chunk + 100, 1100) + 1)) if i < 6 and chunk < 1100 else int(rng.integers(8, min(chunk, 1100) + 1))
        k, nb = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        n_flows = int((1, 2, 3, 17, 64, 100, 1024)[int(rng.integers(0, 7))])
        cost = _costs(rng, n, 4096) if i % 2 else None
        lists, cap_all = _contended(rng, n, k, P, cost)
        caps = rng.integers(1, 2 * cap_all + 1, size=P)
        out.append(_case(f"random-{i}", lists, P, heavy_flows(rng, n, n_flows), n_flows, cost, _table(rng, nb, int(caps.min())), rng.integers(0, nb, size=n),
                         cap=caps, load=rng.integers(0, 3, size=P), seed=1000 + i))
    return out


def coverage(cases, chunk, wants=None):
    """The REQUIRED situations that occur in `cases` under a chunk of `chunk` rows; `wants`: the restatement's answers (computed if None)."""
    seen = set()
    for i, c in enumerate(cases):
        R, k = c["lists"].shape
        nb, nf = len(c["bands"]), c["n_flows"]
        for label, n in (("0", 0), ("1", 1), ("63", 63), ("64", 64), ("65", 65), ("chunk", chunk), ("chunk+1", chunk + 1)):
            if R == n:
                seen.add(f"R={label}")
        if nf in (1, 2, 1024) and R != nf:
            seen.add(f"n_flows={nf}:rows{'<' if R < nf else '>'}flows")
        for field in ("flow", "cost", "load", "band"):
            if c[field] is None and R:
                seen.add(f"null-{field}")
        if R and c["no_score"]:
            seen.add("null-score")
        if R and c["no_rank"]:
            seen.add("null-rank")
        bb, ff, in_order = ref.keys(R, nb, nf, c["band"], c["flow"])
        if c["flow"] is not None:
            good_band = bb < nb
            if np.any(good_band & (ff == nf)):
                seen.add("bad-flow=n_flows-good-band")
            if np.any(good_band & (ff == 0xFFFF) & (ff >= nf)):
                seen.add("bad-flow=0xFFFF-good-band")
            if c["band"] is not None and np.any(~good_band & (ff < nf)):
                seen.add("bad-band-good-flow")
            if np.any(in_order & (ff == nf - 1)) and nf > 1:
                seen.add("flow=n_flows-1")
        rows = np.nonzero(in_order)[0]
        if rows.size == 0:
            continue
        q = ref.turns(bb, ff, in_order, nf)
        g = bb.astype(np.int64) * nf + ff
        cnt = np.zeros((nb, nf), dtype=np.int64)
        np.add.at(cnt, (bb[rows].astype(np.int64), ff[rows]), 1)
        # pairs of one key: the row and the next row of its key
        by_key = rows[np.argsort(g[rows], kind="stable")]
        a, b = by_key[:-1], by_key[1:]
        same = g[a] == g[b]
        a, b = a[same], b[same]
        ca, cb, ta, tb = a // chunk, b // chunk, (a % chunk) // 64, (b % chunk) // 64
        if np.any((ca == cb) & (ta == tb)):
            seen.add("pair-in-one-trip")
        if np.any((ca == cb) & (tb == ta + 1)):
            seen.add("pair-in-adjacent-trips")
        if np.any(ca != cb):
            seen.add("pair-in-different-chunks")
        # whole trips
        for c0 in range(0, R, chunk):
            for t0 in range(c0, min(c0 + chunk, R) - 63, 64):
                trip = np.arange(t0, t0 + 64)
                if in_order[trip].all():
                    distinct = np.unique(g[trip]).size
                    if distinct == 64:
                        seen.add("trip-of-64-distinct-flows")
                    if distinct == 1:
                        seen.add("trip-of-one-flow")
        used_bands = np.nonzero(cnt.sum(axis=1))[0]
        if np.any(cnt.sum(axis=1)[used_bands.min():used_bands.max()] == 0):
            seen.add("empty-band-between-used")
        seg = np.concatenate([[0], np.cumsum(cnt.sum(axis=1))])
        if any(seg[b + 1] % chunk and seg[b + 1] < seg[-1] for b in used_bands):
            seen.add("band-ends-mid-chunk")
        for b in used_bands:
            used = np.nonzero(cnt[b])[0]
            if np.any(cnt[b][used.min():used.max()] == 0):
                seen.add("flow-gap")
            if np.any(cnt[b] == 1):
                seen.add("flow-with-one-row")
        both = (cnt > 0).sum(axis=0) >= 2
        if np.any(both & (cnt.max(axis=0) != np.where(cnt > 0, cnt, cnt.max() + 1).min(axis=0))):
            seen.add("same-flow-in-two-bands-different-counts")
        # the two sides of the min and of the > in the closed form
        for r in rows:
            row, f = cnt[bb[r]], ff[r]
            lo, hi = row[:f], row[f + 1:]
            if np.any(lo == q[r]) and q[r]:
                seen.add("q==cnt-of-lower-flow")
            if np.any(lo == q[r] + 1):
                seen.add("q==cnt-1-of-lower-flow")
            if np.any(hi == q[r]) and q[r]:
                seen.add("q==cnt-of-higher-flow")
            if np.any(hi == q[r] + 1):
                seen.add("q==cnt-1-of-higher-flow")
        if c["cost"] is not None:
            bad_cost = in_order & ((c["cost"] < 1) | (c["cost"] > MAX_COST))
            if bad_cost.any():
                rank = (wants[i] if wants is not None else want(c))[2]
                for r in np.nonzero(bad_cost)[0]:
                    if np.any((g == g[r]) & in_order & (np.arange(R) > r) & (rank < k)):
                        seen.add("bad-cost-holds-a-turn")
    return seen
