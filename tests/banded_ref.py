"""Priority bands over the bounded picker (SEMANTICS.md §3e; include/eppk.h eppk_banded_resolve_device) restated in numpy: band by band
through tests/bounded_ref.py's resolve with the band's own cap, every band finishing (SHED / SPILL) inside its band -- the rule as it is
written, not the deferred finish the device uses.  Test infrastructure: the product does not import it."""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ref = _load("bounded_ref")
NO_PICK, SHED, SPILL = ref.NO_PICK, ref.SHED, ref.SPILL
RANK_OVERFLOW, RANK_NONE = ref.RANK_OVERFLOW, ref.RANK_NONE
LAUNCH_BAD_REQUEST_ROW, LAUNCH_BAD_PICK = 1, ref.LAUNCH_BAD_PICK
MAX_BANDS = 8


def check_table(bands):
    """What the entry points refuse with EPPK_ERR_ARG."""
    assert 1 <= len(bands) <= MAX_BANDS
    assert all(p in (SHED, SPILL) for p, _ in bands)
    assert all(0 <= r <= 0xFFFFFFFF for _, r in bands)
    assert all(bands[b][1] >= bands[b - 1][1] for b in range(1, len(bands))), "reserves must not decrease"


def band_caps(n_pods, cap, cap_all, reserve):
    """cap_b[p] = cap[p] - min(cap[p], reserve_b), as i64."""
    capv = np.full(n_pods, cap_all, dtype=np.int64) if cap is None else np.asarray(cap, dtype=np.uint32).astype(np.int64)
    return capv - np.minimum(capv, int(reserve))


def resolve(lists, scores, n_pods, bands, band=None, cap=None, cap_all=0, load=None):
    """bands: [(policy, reserve)], band 0 first; band: u8 [R] or None (all in band 0); the other arguments as bounded_ref.resolve.
    Returns (pick, score, rank, load_out, flags) -- flags: the launch status bits the *_device forms raise (LAUNCH_BAD_PICK for a list
    entry out of range in ANY row, LAUNCH_BAD_REQUEST_ROW for a band byte >= n_bands)."""
    check_table(bands)
    L = np.asarray(lists, dtype=np.int32)
    R, k = L.shape
    T = np.zeros((R, k), dtype=np.float64) if scores is None else np.asarray(scores, dtype=np.float64)
    bb = np.zeros(R, dtype=np.uint8) if band is None else np.asarray(band, dtype=np.uint8)
    assert bb.shape == (R,)
    pick = np.full(R, NO_PICK, dtype=np.int32)
    score = np.zeros(R, dtype=np.float64)
    rank = np.full(R, RANK_NONE, dtype=np.uint8)                       # (what a row in no band keeps)
    ld = np.zeros(n_pods, dtype=np.uint32) if load is None else np.asarray(load, dtype=np.uint32).copy()
    wrapped = np.zeros(n_pods, dtype=bool)                             # pods whose load a spill has carried past 2^32 - 1: no room any more
    valid = (L >= 0) & (L < n_pods)
    flags = LAUNCH_BAD_PICK if np.any(~valid & (L != NO_PICK)) else 0
    if np.any(bb >= len(bands)):
        flags |= LAUNCH_BAD_REQUEST_ROW
    for b, (policy, reserve) in enumerate(bands):
        rows = np.nonzero(bb == b)[0]                                  # the band's requests, in batch order
        if rows.size == 0:
            continue
        cap_b = band_caps(n_pods, cap, cap_all, reserve)
        cap_b[wrapped] = 0
        p, s, rk, ld_out, _ = ref.resolve(L[rows], T[rows], n_pods, cap_b.astype(np.uint32), 0, policy, ld)
        pick[rows], score[rows], rank[rows] = p, s, rk
        placed = np.bincount(p[p >= 0], minlength=n_pods).astype(np.int64)
        wrapped |= ld.astype(np.int64) + placed > 0xFFFFFFFF
        ld = ld_out
    return pick, score, rank, ld, flags
