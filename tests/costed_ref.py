"""Cost-weighted caps for the bounded and banded pickers (SEMANTICS.md §3f; include/eppk.h eppk_costed_resolve_device) restated in numpy:
what the GPU tests hold the device against, exactly -- picks, ranks, loads, scores as bit patterns, and the launch status.  One stable
sort and one segmented cumulative sum per round.  All sums are exact (int64: a batch of 2^32 rows of cost 2^24 stays below 2^63); the
loads are reduced modulo 2^32 only in what is returned.  Test infrastructure: the product does not import it."""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


banded = _load("banded_ref")
NO_PICK, SHED, SPILL = banded.NO_PICK, banded.SHED, banded.SPILL
RANK_OVERFLOW, RANK_NONE = banded.RANK_OVERFLOW, banded.RANK_NONE
LAUNCH_BAD_REQUEST_ROW, LAUNCH_BAD_PICK = banded.LAUNCH_BAD_REQUEST_ROW, banded.LAUNCH_BAD_PICK
MAX_COST = 0x00FFFFFF
FULL = 0xFFFFFFFF


def cost_matrix(cost, shape, per_entry):
    """The costs as i64 [R, k]: a per-request cost counts for every entry of the request."""
    c = np.asarray(cost, dtype=np.uint32).astype(np.int64)
    R, k = shape
    if per_entry:
        assert c.shape == (R, k)
        return c
    assert c.shape == (R,)
    return np.repeat(c[:, None], k, axis=1)


def bad_rows(lists, n_pods, cost, per_entry, n_bands, band=None):
    """bool [R]: a band byte >= n_bands, or a cost outside 1 .. MAX_COST -- per request: the row's cost; per entry: only at positions
    whose list entry is a valid pod."""
    L = np.asarray(lists, dtype=np.int32)
    R, k = L.shape
    Cm = cost_matrix(cost, (R, k), per_entry)
    out_of_range = (Cm < 1) | (Cm > MAX_COST)
    valid = (L >= 0) & (L < n_pods)
    bad = (out_of_range & valid).any(axis=1) if per_entry else out_of_range[:, 0] if k else np.zeros(R, dtype=bool)
    if band is not None:
        bad = bad | (np.asarray(band, dtype=np.uint8) >= n_bands)
    return bad


def resolve(lists, scores, n_pods, cost, bands, band=None, cap=None, cap_all=0, load=None, per_entry=False, finish_per_band=False):
    """cost: u32 [R], or [R, k] with per_entry; every other argument as banded_ref.resolve.  Returns (pick, score, rank, load_out,
    flags).  finish_per_band: NOT the rule -- every band finishes behind its own rounds, as §3e words it; the tests use it to show that
    under costs the two differ."""
    banded.check_table(bands)
    L = np.asarray(lists, dtype=np.int32)
    R, k = L.shape
    T = np.zeros((R, k), dtype=np.float64) if scores is None else np.asarray(scores, dtype=np.float64)
    bb = np.zeros(R, dtype=np.uint8) if band is None else np.asarray(band, dtype=np.uint8)
    assert bb.shape == (R,)
    Cm = cost_matrix(cost, (R, k), per_entry)
    valid = (L >= 0) & (L < n_pods)
    bad = bad_rows(L, n_pods, cost, per_entry, len(bands), bb)
    flags = (LAUNCH_BAD_PICK if np.any(~valid & (L != NO_PICK)) else 0) | (LAUNCH_BAD_REQUEST_ROW if bad.any() else 0)
    capv = np.full(n_pods, cap_all, dtype=np.int64) if cap is None else np.asarray(cap, dtype=np.uint32).astype(np.int64)
    ld = np.zeros(n_pods, dtype=np.int64) if load is None else np.asarray(load, dtype=np.uint32).astype(np.int64)
    pick = np.full(R, NO_PICK, dtype=np.int32)
    score = np.zeros(R, dtype=np.float64)
    rank = np.full(R, RANK_NONE, dtype=np.uint8)
    assigned = np.zeros(R, dtype=bool)

    def finish(rows):
        """rows: unassigned, not bad, in batch order."""
        for r in rows[valid[rows].any(axis=1)]:
            f = int(np.argmax(valid[r]))
            rank[r] = RANK_OVERFLOW
            if bands[bb[r]][0] == SPILL:
                pick[r], score[r], rank[r] = L[r, f], T[r, f], RANK_OVERFLOW | f
                ld[L[r, f]] += Cm[r, f]

    for b, (_, reserve) in enumerate(bands):
        in_band = (bb == b) & ~bad
        cap_b = capv - np.minimum(capv, int(reserve))
        for j in range(k):
            rows = np.nonzero(in_band & ~assigned & valid[:, j])[0]      # entry j is a valid pod, in batch order
            if rows.size == 0:
                continue
            room = np.maximum(cap_b - ld, 0)                             # on the loads as the round before left them
            p, c = L[rows, j].astype(np.int64), Cm[rows, j]
            fits = c <= room[p]                                           # the bidders: those that could fit alone
            rows, p, c = rows[fits], p[fits], c[fits]
            order = np.argsort(p, kind="stable")                          # by pod; batch order within a pod
            ps, cs = p[order], c[order]
            run = np.cumsum(cs) - cs                                      # exclusive, over all pods ...
            start = np.searchsorted(ps, ps, side="left")
            S = run - run[start] if ps.size else run                      # ... minus what the pods in front hold: S per bidder
            take = np.empty(rows.size, dtype=bool)
            take[order] = S + cs <= room[ps]
            got = rows[take]
            pick[got], score[got], rank[got] = L[got, j], T[got, j], j
            assigned[got] = True
            np.add.at(ld, p[take], c[take])
        if finish_per_band:
            finish(np.nonzero(in_band & ~assigned)[0])
    if not finish_per_band:
        finish(np.nonzero(~bad & ~assigned)[0])
    return pick, score, rank, (ld & FULL).astype(np.uint32), flags
