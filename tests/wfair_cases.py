"""Inputs for the weighted fair resolve (SEMANTICS.md §3h): every case of tests/fair_cases.py with weights and carried turns laid over it
(so the batch sizes, the flow counts and the null forms of §3g come along), and the smallest shapes that can break the weighted order
and the carry: cycle boundaries, a flow a whole cycle behind, turns at the top of 32 bits, weight 0, the two sides of the carry rule.

A case is a dict: the fields of tests/fair_cases.py and weight (u16 [n_flows] or None) and turns (u32 [n_bands][n_flows] or None).  What a
case is FOR is not declared: coverage() reads from the cases themselves (and from the restatement's answers) which of the REQUIRED
situations occur, and tests/test_wfair_ref_cpu.py holds the generator to all of them."""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("wfair_ref")
fc = _load("fair_cases")
SEED0 = 0x3FA1
NO, SHED, SPILL = ref.NO_PICK, ref.SHED, ref.SPILL
MAX_COST, MAX_FLOWS, TOP = ref.MAX_COST, ref.MAX_FLOWS, ref.TOP

# every situation the corpus must contain (observed by coverage(), not declared)
REQUIRED = (
    [f"{at}-vs-{side}-flow" for at in ("on-cycle-boundary", "one-below-cycle-boundary") for side in ("lower", "higher")] +
    ["flow-wholly-in-a-later-cycle", "flow-with-turns-and-no-rows", "weight=1", "weight=2", "weight=64", "weight=65535",
     "t=2^32-1-with-q>0", "carry-saturates", "weight-0-good-band", "same-flow-in-two-bands-different-turns",
     "shed-and-spilled-rows-under-a-carry", "bad-cost-holds-a-turn-and-takes-none",
     "null-weight", "null-turns", "null-weight-and-turns", "null-flow", "null-cost", "null-load", "null-score", "null-rank", "null-band"] +
    [f"n_flows={n}:{side}" for n in (1, 2, 1024) for side in ("rows<flows", "rows>flows")] +
    [f"R={s}" for s in ("0", "1", "63", "64", "65", "chunk", "chunk+1")])


def _with(c, weight, turns, name=None):
    nb, nf = len(c["bands"]), c["n_flows"]
    out = dict(c, weight=None if weight is None else np.ascontiguousarray(weight, dtype=np.uint16),
               turns=None if turns is None else np.ascontiguousarray(np.asarray(turns, dtype=np.uint32).reshape(nb, nf)))
    if name:
        out["name"] = name
    assert out["weight"] is None or out["weight"].shape == (nf,)
    return out


def want(c):
    """The restatement's answer for a case: (pick, score, rank, load_out, launch-status flags, turns_out | None)."""
    return ref.resolve(c["lists"], c["scores"], c["n_pods"], c["flow"], c["n_flows"], c["weight"], c["turns"], c["cost"], c["bands"], c["band"], c["cap"],
                       c["cap_all"], c["load"])


def info(c):
    return fc.info(c) + f"{' no weight' if c['weight'] is None else ''}{' no turns' if c['turns'] is None else ''}"


def shares_case():
    """§3h's first example: one pod, cap_all 5, k = 1, SHED, three flows of five rows each, weights (3, 1, 1): the placed rows are
    3 / 1 / 1 -- rows 0, 1, 2, 5 and 10."""
    flow = np.repeat(np.arange(3), 5).astype(np.uint16)
    return np.zeros((15, 1), dtype=np.int32), flow, np.array([3, 1, 1], dtype=np.uint16), 5, [0, 1, 2, 5, 10]


def _one_band(name, lists, P, flow, nf, weight, turns, cap_all, cost=None, bands=((SHED, 0),), band=None, seed=0):
    return _with(fc._case(name, lists, P, flow, nf, cost, bands, band, cap_all=cap_all, load=np.zeros(P), seed=seed), weight, turns)


def make_cases(chunk):
    """Every case, for a context whose chunk holds `chunk` rows (a power of two >= 64)."""
    rng = np.random.default_rng(SEED0 + chunk)
    out = []
    # -- §3g's corpus under weights and turns: none, weights alone, turns alone, both; small weights, so that every cycle boundary is met
    for i, c in enumerate(fc.make_cases(chunk)):
        nb, nf = len(c["bands"]), c["n_flows"]
        weight = rng.integers(1, 5, size=nf) if i % 4 in (1, 3) else None
        top = (weight if weight is not None else np.ones(nf, dtype=np.int64)) * 3
        turns = rng.integers(0, top + 1, size=(nb, nf)) if i % 4 in (2, 3) else None
        out.append(_with(c, weight, turns))
    # -- the worked examples
    lists, flow, weight, cap, _ = shares_case()
    out.append(_one_band("shares-3-1-1", lists, 1, flow, 3, weight, None, cap))
    for batch, turns in enumerate(([0, 0, 0], [1, 0, 0], [1, 1, 0])):
        out.append(_one_band(f"one-slot-batch-{batch}", np.zeros((3, 1), dtype=np.int32), 1, [0, 1, 2], 3, None, turns, 1))
    # -- a flow a whole cycle behind everybody; a flow with turns and no rows; the same flow in two bands with different turns
    n = chunk + 9
    lists, cap_all = fc._contended(rng, n, 2, 3, None)
    flow = rng.integers(0, 3, size=n)
    out.append(_one_band("flow-2-comes-last", lists, 3, flow, 4, [1, 2, 1, 3], [0, 3, 4 * n, 17], cap_all))
    band = rng.integers(0, 2, size=n)
    out.append(_one_band("two-bands-different-turns", lists, 3, flow, 4, [2, 1, 3, 1], [[0, 5, 2, 9], [7, 0, 0, 1]], cap_all, bands=[(SHED, 0), (SPILL, 1)], band=band))
    # -- weights 1, 2, 64 and 65535 side by side, turns of the size of the weights
    n = 2 * chunk + 31
    lists, cap_all = fc._contended(rng, n, 3, 4, None)
    weight = np.array([1, 2, 64, 65535, 3], dtype=np.uint16)
    out.append(_one_band("weights-1-2-64-65535", lists, 4, fc.heavy_flows(rng, n, 5, 0.25), 5, weight, [0, 1, 63, 65534, 2], cap_all))
    out.append(_one_band("weights-1-2-64-65535-later", lists, 4, rng.integers(0, 5, size=n), 5, weight, [5, 11, 64 * 5 + 1, 65535 * 5 - 2, 14], cap_all,
                         cost=fc._costs(rng, n, 8)))
    # -- the top of 32 bits: t = 2^32 - 1 with q > 0 (the cycle needs 33 bits), heavy and light flows next to it (the product needs 49),
    #    room for everybody, so that the carry saturates
    n = 70
    lists = fc.bc._random_lists(rng, n, 2, 5)
    flow = rng.integers(0, 4, size=n)
    for label, weight, turns in (("light", [1, 65535, 2, 1], [TOP, TOP - 3, TOP - 1, TOP - 40]), ("heavy", [65535, 1, 65535, 7], [TOP, 65536, TOP - 65535 * 2, TOP - 1]),
                                 ("mixed", [1, 65535, 1, 3], [TOP, 0, 5, TOP // 2])):
        out.append(_one_band(f"top-of-32-bits-{label}", lists, 5, flow, 4, weight, turns, n))
    # -- weight 0 under a good band: out of the order, answered as a bad flow; between good rows and behind a chunk boundary
    n = chunk + 20
    for label, cost in (("costed", fc._costs(rng, n, 8)), ("counted", None)):
        lists, cap_all = fc._contended(rng, n, 3, 4, cost)
        flow, band = rng.integers(0, 6, size=n), rng.integers(0, 2, size=n)
        flow[5], flow[chunk + 3], flow[7] = 2, 2, 6
        lists[5] = [0, 9, 1]                                               # (EPPK_LAUNCH_BAD_PICK from a row that is not in the order)
        out.append(_one_band(f"weight-0-{label}", lists, 4, flow, 6, [2, 1, 0, 3, 0, 1], rng.integers(0, 4, size=(2, 6)), cap_all, cost=cost,
                             bands=[(SHED, 0), (SPILL, 1)], band=band))
    # -- both sides of the carry rule: a SHED band and a SPILL band that overflow, rows without a valid entry, a bad cost that holds its turn
    n = chunk + 66
    cost = fc._costs(rng, n, 8)
    cost[3], cost[chunk + 1], cost[70] = 0, MAX_COST + 1, 0xFFFFFFFF
    out.append(_one_band("bad-cost-holds-turn", fc.bc._random_lists(rng, n, 2, 6), 6, rng.integers(0, 4, size=n), 4, [1, 2, 1, 3], rng.integers(0, 6, size=(2, 4)),
                         int(cost[cost <= MAX_COST].sum()), cost=cost, bands=[(SHED, 0), (SHED, 0)], band=rng.integers(0, 2, size=n)))
    # -- seeded random: few pods, heavy-tailed flows, any weight, turns up to a few cycles
    for i in range(8):
        P = int(rng.integers(1, 9))
        n = int(rng.integers(chunk + 1, min(2 * chunk + 100, 1100) + 1)) if i < 4 and chunk < 1100 else int(rng.integers(8, min(chunk, 1100) + 1))
        k, nb = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        nf = int((2, 3, 17, 64, 100, 1024)[int(rng.integers(0, 6))])
        cost = fc._costs(rng, n, 4096) if i % 2 else None
        lists, cap_all = fc._contended(rng, n, k, P, cost)
        caps = rng.integers(1, 2 * cap_all + 1, size=P)
        weight = np.where(rng.random(nf) < 0.7, rng.integers(1, 6, size=nf), rng.integers(1, 65536, size=nf))
        turns = (rng.random((nb, nf)) * 4 * weight).astype(np.int64)
        c = fc._case(f"random-{i}", lists, P, fc.heavy_flows(rng, n, nf), nf, cost, fc._table(rng, nb, int(caps.min())), rng.integers(0, nb, size=n), cap=caps,
                     load=rng.integers(0, 3, size=P), seed=2000 + i)
        out.append(_with(c, weight, turns))
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
        for field in ("weight", "turns", "flow", "cost", "load", "band"):
            if c[field] is None and R:
                seen.add(f"null-{field}")
        if c["weight"] is None and c["turns"] is None and R:
            seen.add("null-weight-and-turns")
        if R and c["no_score"]:
            seen.add("null-score")
        if R and c["no_rank"]:
            seen.add("null-rank")
        w, t = ref.tables(nb, nf, c["weight"], c["turns"])
        bb, ff, in_order = ref.keys(R, nb, nf, c["band"], c["flow"], c["weight"])
        if np.any((bb < nb) & (ff < nf) & ~in_order):
            seen.add("weight-0-good-band")
        rows = np.nonzero(in_order)[0]
        if rows.size == 0:
            continue
        q, cyc = ref.cycles(bb, ff, in_order, nf, w, t)
        n = np.zeros((nb, nf), dtype=np.int64)
        np.add.at(n, (bb[rows].astype(np.int64), ff[rows]), 1)
        g = bb.astype(np.int64) * nf + ff
        for wv in (1, 2, 64, 65535):
            if np.any((w == wv) & (n.sum(axis=0) > 0)) and np.any((n > 0).sum(axis=1) >= 2):
                seen.add(f"weight={wv}")
        if np.any((n.sum(axis=1, keepdims=True) > 0) & (n == 0) & (t > 0) & (w >= 1)):
            seen.add("flow-with-turns-and-no-rows")
        if np.any((t[bb[rows].astype(np.int64), ff[rows]] == TOP) & (q[rows] > 0)):
            seen.add("t=2^32-1-with-q>0")
        both = (n > 0).sum(axis=0) >= 2
        if c["turns"] is not None and np.any(both & (np.where(n > 0, t, -1).max(axis=0) != np.where(n > 0, t, 2 ** 40).min(axis=0))):
            seen.add("same-flow-in-two-bands-different-turns")
        for b in np.nonzero(n.sum(axis=1))[0]:
            br = rows[bb[rows] == b]
            flows = np.unique(ff[br])
            lo = {int(f): int(cyc[br][ff[br] == f].min()) for f in flows}
            hi = {int(f): int(cyc[br][ff[br] == f].max()) for f in flows}
            for f in flows:
                others = [x for x in flows if x != f]
                if others and lo[int(f)] > max(hi[int(x)] for x in others):
                    seen.add("flow-wholly-in-a-later-cycle")
            # a row at the first turn of a cycle / at the last turn of one, with a lower / a higher flow that has a row in that very cycle
            at = (t[b, ff[br]] + q[br]) % w[ff[br]]
            have = set(zip(ff[br].tolist(), cyc[br].tolist()))
            for r, a in zip(br, at):
                wf = w[ff[r]]
                if wf < 2 or a not in (0, wf - 1):
                    continue
                label = "on-cycle-boundary" if a == 0 else "one-below-cycle-boundary"
                if any((int(x), int(cyc[r])) in have for x in flows if x < ff[r]):
                    seen.add(f"{label}-vs-lower-flow")
                if any((int(x), int(cyc[r])) in have for x in flows if x > ff[r]):
                    seen.add(f"{label}-vs-higher-flow")
        if c["turns"] is None:
            continue
        pick, _, rank, _, _, turns_out = wants[i] if wants is not None else want(c)
        took = in_order & (pick != NO)
        taken = np.zeros((nb, nf), dtype=np.int64)
        np.add.at(taken, (bb[took].astype(np.int64), ff[took]), 1)
        if np.any(t + taken > TOP):
            assert np.all(turns_out[t + taken > TOP] == TOP)
            seen.add("carry-saturates")
        valid = ((c["lists"] >= 0) & (c["lists"] < c["n_pods"])).any(axis=1)
        if np.any(in_order & valid & (pick == NO)) and np.any(took & ((rank & ref.RANK_OVERFLOW) != 0)) and np.any(in_order & ~valid):
            seen.add("shed-and-spilled-rows-under-a-carry")
        if c["cost"] is not None:
            bad_cost = in_order & ((c["cost"] < 1) | (c["cost"] > MAX_COST))
            for r in np.nonzero(bad_cost)[0]:
                if pick[r] == NO and np.any((g == g[r]) & in_order & (np.arange(R) > r) & (rank < k)):
                    seen.add("bad-cost-holds-a-turn-and-takes-none")
    return seen
