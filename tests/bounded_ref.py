"""The picker "best-score under per-pod caps" (SEMANTICS.md §3d; include/eppk.h eppk_bounded_resolve_device) restated in numpy: what the
GPU tests hold the device against, exactly -- picks, ranks, loads, and scores as bit patterns.  Test infrastructure: the product does not
import it.  One sort per round, so a 64k-row batch takes milliseconds."""
import numpy as np

NO_PICK = -1
SHED, SPILL = 0, 1
RANK_OVERFLOW, RANK_NONE = 0x40, 0x80
LAUNCH_BAD_PICK = 2
MAX_TOPK = 8


def resolve(lists, scores, n_pods, cap=None, cap_all=0, policy=SHED, load=None):
    """lists [R, k] i32; scores [R, k] f64 or None (the totals of the entries; absent: every score is 0.0); cap u32 [n_pods] or None
    (every pod: cap_all); load u32 [n_pods] or None (zeros).  Returns (pick [R] i32, score [R] f64, rank [R] u8, load_out [n_pods] u32,
    bad) -- bad: some entry is neither EPPK_NO_PICK nor in [0, n_pods), which raises EPPK_LAUNCH_BAD_PICK."""
    L = np.asarray(lists, dtype=np.int32)
    R, k = L.shape
    assert 1 <= k <= MAX_TOPK and policy in (SHED, SPILL)
    T = np.zeros((R, k), dtype=np.float64) if scores is None else np.asarray(scores, dtype=np.float64)
    valid = (L >= 0) & (L < n_pods)
    bad = bool(np.any(~valid & (L != NO_PICK)))
    capv = np.full(n_pods, cap_all, dtype=np.int64) if cap is None else np.asarray(cap, dtype=np.uint32).astype(np.int64)
    ld = np.zeros(n_pods, dtype=np.int64) if load is None else np.asarray(load, dtype=np.uint32).astype(np.int64)
    pick = np.full(R, NO_PICK, dtype=np.int32)
    score = np.zeros(R, dtype=np.float64)
    rank = np.full(R, RANK_NONE, dtype=np.uint8)
    assigned = np.zeros(R, dtype=bool)
    for j in range(k):
        rows = np.nonzero(~assigned & valid[:, j])[0]                 # this round's bidders, in batch order
        if rows.size == 0:
            continue
        p = L[rows, j].astype(np.int64)
        room = np.maximum(capv - ld, 0)                               # on the loads as the round before left them
        order = np.argsort(p, kind="stable")                          # by pod; batch order within a pod
        ps = p[order]
        place = np.empty(rows.size, dtype=np.int64)
        place[order] = np.arange(rows.size) - np.searchsorted(ps, ps, side="left")
        take = place < room[p]
        got = rows[take]
        pick[got] = L[got, j]
        score[got] = T[got, j]
        rank[got] = j
        assigned[got] = True
        ld += np.bincount(p[take], minlength=n_pods)
    rest = np.nonzero(~assigned & valid.any(axis=1))[0]                # unassigned, but with a valid entry: overflow
    if policy == SHED:
        rank[rest] = RANK_OVERFLOW
    else:
        f = np.argmax(valid[rest], axis=1)
        pick[rest] = L[rest, f]
        score[rest] = T[rest, f]
        rank[rest] = RANK_OVERFLOW | f.astype(np.uint8)
        ld += np.bincount(L[rest, f], minlength=n_pods)
    return pick, score, rank, (ld & 0xFFFFFFFF).astype(np.uint32), bad
