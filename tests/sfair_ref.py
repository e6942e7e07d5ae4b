"""Fair shares between flows in cost units, the rows ordered by carried service (SEMANTICS.md §3i; include/eppk.h
eppk_sfair_resolve_device) restated in numpy: what the GPU tests hold the device against, exactly -- picks, ranks, loads, service,
scores as bit patterns, and the launch status.

As tests/wfair_ref.py the rule is a permutation in front of §3f: every row's charge (its cost, or 0 for a bad one), its start tag
(service[band][flow] + the charges of the rows of its key in front of it) // weight[flow] in Python integers, the rows that are in the
order sorted by (band, tag - the band's least tag, flow, q), tests/costed_ref.py (without costs tests/banded_ref.py) over the permuted
batch, the answers scattered back; then the carry, service += the charges of the rows of the key that hold an endpoint, saturating.
Test infrastructure: the product does not import it."""
import importlib.util
import os

import numpy as np

_spec = importlib.util.spec_from_file_location("wfair_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "wfair_ref.py"))
wfair = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(wfair)
fair, costed, banded = wfair.fair, wfair.costed, wfair.banded
NO_PICK, SHED, SPILL, BAD_BAND, MAX_COST, TOP = wfair.NO_PICK, wfair.SHED, wfair.SPILL, wfair.BAD_BAND, wfair.MAX_COST, wfair.TOP
RANK_OVERFLOW, RANK_NONE, LAUNCH_BAD_REQUEST_ROW = wfair.RANK_OVERFLOW, wfair.RANK_NONE, wfair.LAUNCH_BAD_REQUEST_ROW
MAX_REQS = 131072


def charges(R, cost):
    """i64 [R]: the cost where it is 1 .. MAX_COST, 0 elsewhere; no costs: ones."""
    c = np.ones(R, dtype=np.int64) if cost is None else np.asarray(cost, dtype=np.uint32).astype(np.int64)
    return np.where((c >= 1) & (c <= MAX_COST), c, 0)


def order(bb, ff, in_order, n_flows, w, s, charge):
    """The rows in the order, band by band, each band by (tag - least tag of the band, flow, q) ascending: place -> row."""
    rows = np.nonzero(in_order)[0]
    q = fair.turns(bb, ff, in_order, n_flows)
    run, d = {}, np.zeros(bb.size, dtype=object)
    for r in rows:                                                         # Python integers: no width to overflow
        g = (int(bb[r]), int(ff[r]))
        run.setdefault(g, int(s[g]))
        d[r] = run[g] // int(w[g[1]])
        run[g] += int(charge[r])
    for b in set(int(x) for x in bb[rows]):
        of_band = rows[bb[rows] == b]
        d[of_band] -= min(d[of_band])
    assert all(0 <= int(x) < 1 << 42 for x in d[rows])
    return rows[np.lexsort((q[rows], ff[rows], d[rows].astype(np.int64), bb[rows]))]


def resolve(lists, scores, n_pods, flow, n_flows, weight, service, cost, bands, band=None, cap=None, cap_all=0, load=None):
    """weight: u16 [n_flows] or None (ones); service: u32 [n_bands][n_flows] or None (zeros, nothing handed back); cost: u32 [R] or None
    (ones).  Returns (pick, score, rank, load_out, flags, service_out | None)."""
    L = np.asarray(lists, dtype=np.int32)
    R, k = L.shape
    assert R <= MAX_REQS
    nb = len(bands)
    w, s = wfair.tables(nb, n_flows, weight, service)
    bb, ff, in_order = wfair.keys(R, nb, n_flows, band, flow, weight)
    charge = charges(R, cost)
    perm = np.concatenate([order(bb, ff, in_order, n_flows, w, s, charge), np.nonzero(~in_order)[0]]).astype(np.int64)
    assert np.array_equal(np.sort(perm), np.arange(R))
    eff = np.where(in_order, bb, BAD_BAND).astype(np.uint8)
    T = None if scores is None else np.asarray(scores, dtype=np.float64)[perm]
    if cost is None:
        got = banded.resolve(L[perm], T, n_pods, bands, eff[perm], cap, cap_all, load)
    else:
        got = costed.resolve(L[perm], T, n_pods, np.asarray(cost, dtype=np.uint32)[perm], bands, eff[perm], cap, cap_all, load, False)
    pick, score, rank = np.empty(R, dtype=np.int32), np.empty(R, dtype=np.float64), np.empty(R, dtype=np.uint8)
    pick[perm], score[perm], rank[perm] = got[0], got[1], got[2]
    service_out = None
    if service is not None:
        taken = np.zeros((nb, n_flows), dtype=np.int64)
        took = in_order & (pick != NO_PICK)
        np.add.at(taken, (bb[took].astype(np.int64), ff[took]), charge[took])
        service_out = np.minimum(s + taken, TOP).astype(np.uint32)
    return pick, score, rank, got[3], got[4], service_out
