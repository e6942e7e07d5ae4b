"""Weighted fair shares between flows with turns carried across batches (SEMANTICS.md §3h; include/eppk.h eppk_wfair_resolve_device)
restated in numpy: what the GPU tests hold the device against, exactly -- picks, ranks, loads, turns, scores as bit patterns, and the
launch status.

As tests/fair_ref.py the rule is a permutation in front of §3f: every row's turn q and cycle c = (turns[band][flow] + q) // weight[flow],
the rows that are in the order sorted by (band, c, flow, q), tests/costed_ref.py (without costs tests/banded_ref.py) over the permuted
batch, the answers scattered back; then the carry, turns += the rows of the key that hold an endpoint, saturating.  A row whose flow has
weight 0 is not in the order, as a row whose flow is >= n_flows.  Test infrastructure: the product does not import it."""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


fair = _load("fair_ref")
costed, banded = fair.costed, fair.banded
NO_PICK, SHED, SPILL = fair.NO_PICK, fair.SHED, fair.SPILL
RANK_OVERFLOW, RANK_NONE = fair.RANK_OVERFLOW, fair.RANK_NONE
LAUNCH_BAD_REQUEST_ROW, LAUNCH_BAD_PICK = fair.LAUNCH_BAD_REQUEST_ROW, fair.LAUNCH_BAD_PICK
MAX_COST, MAX_FLOWS, BAD_BAND = fair.MAX_COST, fair.MAX_FLOWS, fair.BAD_BAND
MAX_BANDS = 8
TOP = 0xFFFFFFFF


def tables(n_bands, n_flows, weight=None, turns=None):
    """(w i64 [n_flows], t i64 [n_bands][n_flows]) with the NULL arrays filled in: ones, zeros."""
    w = np.ones(n_flows, dtype=np.int64) if weight is None else np.asarray(weight, dtype=np.uint16).astype(np.int64)
    t = np.zeros((n_bands, n_flows), dtype=np.int64) if turns is None else np.asarray(turns, dtype=np.uint32).astype(np.int64).reshape(n_bands, n_flows)
    assert w.shape == (n_flows,)
    return w, t


def keys(R, n_bands, n_flows, band=None, flow=None, weight=None):
    """(band u8 [R], flow i64 [R], in_order bool [R]): fair_ref.keys and the weight test."""
    bb, ff, in_order = fair.keys(R, n_bands, n_flows, band, flow)
    w, _ = tables(n_bands, n_flows, weight)
    return bb, ff, in_order & (w[np.minimum(ff, n_flows - 1)] >= 1)


def cycles(bb, ff, in_order, n_flows, w, t):
    """(q i64 [R], c i64 [R]): turn and cycle of every row in the order; -1 elsewhere.  t + q < 2^33 and fits 64 bits with room."""
    q = fair.turns(bb, ff, in_order, n_flows)
    c = np.full(bb.size, -1, dtype=np.int64)
    rows = np.nonzero(in_order)[0]
    c[rows] = (t[bb[rows].astype(np.int64), ff[rows]] + q[rows]) // w[ff[rows]]
    return q, c


def order(bb, ff, in_order, n_flows, w, t):
    """The rows in the order, band by band, each band by (c, flow, q) ascending: place -> row."""
    q, c = cycles(bb, ff, in_order, n_flows, w, t)
    rows = np.nonzero(in_order)[0]
    return rows[np.lexsort((q[rows], ff[rows], c[rows], bb[rows]))]


def places(bb, ff, in_order, n_bands, n_flows, w, t):
    """The closed form of §3h, no sort: place(r) = seg[b] + q + sum over f' != f of clamp((c + [f' < f]) * w[f'] - t[b][f'], 0, n[b][f']);
    -1 for a row that is not in the order.  Python integers: no width to overflow."""
    q, c = cycles(bb, ff, in_order, n_flows, w, t)
    n = np.zeros((n_bands, n_flows), dtype=np.int64)
    np.add.at(n, (bb[in_order].astype(np.int64), ff[in_order]), 1)
    seg = np.concatenate([[0], np.cumsum(n.sum(axis=1))])
    place = np.full(bb.size, -1, dtype=np.int64)
    wo, lower = w.astype(object), np.arange(n_flows)
    for r in np.nonzero(in_order)[0]:
        b, f = int(bb[r]), int(ff[r])
        x = (int(c[r]) + (lower < f).astype(object)) * wo - t[b].astype(object)
        x = np.minimum(np.maximum(x, 0), n[b].astype(object))
        x[f] = 0
        place[r] = int(seg[b]) + int(q[r]) + int(x.sum())
    return place


def resolve(lists, scores, n_pods, flow, n_flows, weight, turns, cost, bands, band=None, cap=None, cap_all=0, load=None, per_entry=False):
    """weight: u16 [n_flows] or None (ones); turns: u32 [n_bands][n_flows] or None (zeros, nothing handed back); every other argument as
    fair_ref.resolve.  Returns (pick, score, rank, load_out, flags, turns_out | None)."""
    L = np.asarray(lists, dtype=np.int32)
    R, k = L.shape
    nb = len(bands)
    w, t = tables(nb, n_flows, weight, turns)
    bb, ff, in_order = keys(R, nb, n_flows, band, flow, weight)
    perm = np.concatenate([order(bb, ff, in_order, n_flows, w, t), np.nonzero(~in_order)[0]]).astype(np.int64)
    assert np.array_equal(np.sort(perm), np.arange(R))
    eff = np.where(in_order, bb, BAD_BAND).astype(np.uint8)                # weight 0 and a bad flow are answered as a bad band is
    T = None if scores is None else np.asarray(scores, dtype=np.float64)[perm]
    if cost is None:
        assert not per_entry
        got = banded.resolve(L[perm], T, n_pods, bands, eff[perm], cap, cap_all, load)
    else:
        got = costed.resolve(L[perm], T, n_pods, np.asarray(cost, dtype=np.uint32)[perm], bands, eff[perm], cap, cap_all, load, per_entry)
    pick, score, rank = np.empty(R, dtype=np.int32), np.empty(R, dtype=np.float64), np.empty(R, dtype=np.uint8)
    pick[perm], score[perm], rank[perm] = got[0], got[1], got[2]
    turns_out = None
    if turns is not None:
        taken = np.zeros((nb, n_flows), dtype=np.int64)
        took = in_order & (pick != NO_PICK)
        np.add.at(taken, (bb[took].astype(np.int64), ff[took]), 1)
        turns_out = np.minimum(t + taken, TOP).astype(np.uint32)
    return pick, score, rank, got[3], got[4], turns_out


def rebase(turns, weight, window):
    """eppk_fair_turns_rebase on a copy: u32 [n_bands][n_flows].  Python integers."""
    out = np.array(turns, dtype=np.uint32, copy=True)
    nb, nf = out.shape
    w = [1] * nf if weight is None else [int(x) for x in np.asarray(weight, dtype=np.uint16)]
    live = [f for f in range(nf) if w[f] >= 1]
    for b in range(nb):
        if not live:
            break
        t = {f: int(out[b, f]) for f in live}
        top = max(t[f] // w[f] for f in live)
        if top > window:
            for f in live:
                if t[f] // w[f] < top - window:
                    t[f] = (top - window) * w[f]
        low = min(t[f] // w[f] for f in live)
        for f in live:
            v = t[f] - low * w[f]
            assert 0 <= v <= TOP
            out[b, f] = v
    return out
