"""Fair shares between flows for the banded and costed pickers (SEMANTICS.md §3g; include/eppk.h eppk_fair_resolve_device) restated in
numpy: what the GPU tests hold the device against, exactly -- picks, ranks, loads, scores as bit patterns, and the launch status.

The rule is a permutation in front of §3f: compute every row's turn q, sort the rows that are in the order by (band, q, flow), run
tests/costed_ref.py (without costs tests/banded_ref.py) over the permuted batch, and scatter the answers back.  The rows that are not in
the order (band byte >= n_bands or flow >= n_flows) are appended behind the others with a band byte no table has, so that the
restatement underneath answers them as bad rows.  Test infrastructure: the product does not import it."""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


costed = _load("costed_ref")
banded = costed.banded
NO_PICK, SHED, SPILL = costed.NO_PICK, costed.SHED, costed.SPILL
RANK_OVERFLOW, RANK_NONE = costed.RANK_OVERFLOW, costed.RANK_NONE
LAUNCH_BAD_REQUEST_ROW, LAUNCH_BAD_PICK = costed.LAUNCH_BAD_REQUEST_ROW, costed.LAUNCH_BAD_PICK
MAX_COST, FULL = costed.MAX_COST, costed.FULL
MAX_FLOWS = 1024
BAD_BAND = 0xFF


def keys(R, n_bands, n_flows, band=None, flow=None):
    """(band u8 [R], flow i64 [R], in_order bool [R]) with the NULL arrays filled in."""
    bb = np.zeros(R, dtype=np.uint8) if band is None else np.asarray(band, dtype=np.uint8)
    ff = np.zeros(R, dtype=np.int64) if flow is None else np.asarray(flow, dtype=np.uint16).astype(np.int64)
    assert bb.shape == (R,) and ff.shape == (R,) and 1 <= n_flows <= MAX_FLOWS
    return bb, ff, (bb < n_bands) & (ff < n_flows)


def turns(bb, ff, in_order, n_flows):
    """i64 [R]: for a row in the order, the rows in front of it in the order with the same band and flow; -1 elsewhere."""
    q = np.full(bb.size, -1, dtype=np.int64)
    rows = np.nonzero(in_order)[0]
    g = bb[rows].astype(np.int64) * n_flows + ff[rows]
    by_key = np.argsort(g, kind="stable")                                  # batch order inside a key
    gs = g[by_key]
    q[rows[by_key]] = np.arange(gs.size) - np.searchsorted(gs, gs, side="left")
    return q


def fair_order(bb, ff, in_order, n_flows):
    """The rows in the order, band by band, each band by (q, flow) ascending: place -> row."""
    q = turns(bb, ff, in_order, n_flows)
    rows = np.nonzero(in_order)[0]
    return rows[np.lexsort((ff[rows], q[rows], bb[rows]))]


def places(bb, ff, in_order, n_bands, n_flows):
    """The closed form of §3g, no sort: place(r) = seg[b] + sum_f' min(cnt[b][f'], q) + #{f' < f: cnt[b][f'] > q}; -1 for a row that is
    not in the order."""
    q = turns(bb, ff, in_order, n_flows)
    cnt = np.zeros((n_bands, n_flows), dtype=np.int64)
    np.add.at(cnt, (bb[in_order].astype(np.int64), ff[in_order]), 1)
    seg = np.concatenate([[0], np.cumsum(cnt.sum(axis=1))])
    place = np.full(bb.size, -1, dtype=np.int64)
    for r in np.nonzero(in_order)[0]:
        c = cnt[bb[r]]
        place[r] = seg[bb[r]] + np.minimum(c, q[r]).sum() + np.count_nonzero(c[:ff[r]] > q[r])
    return place


def resolve(lists, scores, n_pods, flow, n_flows, cost, bands, band=None, cap=None, cap_all=0, load=None, per_entry=False):
    """flow: u16 [R] or None (all in flow 0); cost: as costed_ref.resolve, or None (every cost 1: banded_ref.resolve underneath); every
    other argument as costed_ref.resolve.  Returns (pick, score, rank, load_out, flags)."""
    L = np.asarray(lists, dtype=np.int32)
    R, k = L.shape
    bb, ff, in_order = keys(R, len(bands), n_flows, band, flow)
    perm = np.concatenate([fair_order(bb, ff, in_order, n_flows), np.nonzero(~in_order)[0]]).astype(np.int64)
    assert np.array_equal(np.sort(perm), np.arange(R))
    eff = np.where(in_order, bb, BAD_BAND).astype(np.uint8)                # a bad flow is answered as a bad band is
    T = None if scores is None else np.asarray(scores, dtype=np.float64)[perm]
    if cost is None:
        assert not per_entry
        got = banded.resolve(L[perm], T, n_pods, bands, eff[perm], cap, cap_all, load)
    else:
        got = costed.resolve(L[perm], T, n_pods, np.asarray(cost, dtype=np.uint32)[perm], bands, eff[perm], cap, cap_all, load, per_entry)
    pick, score, rank = np.empty(R, dtype=np.int32), np.empty(R, dtype=np.float64), np.empty(R, dtype=np.uint8)
    pick[perm], score[perm], rank[perm] = got[0], got[1], got[2]
    return pick, score, rank, got[3], got[4]
