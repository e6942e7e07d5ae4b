"""Test-side cases for the buffers of a context that grow on demand: per buffer a sequence small -> large -> small -> larger through the
entry point that sizes it, at the smallest shapes that cross each capacity, with the reference model of tests/session_cases.py behind
every step.  tests/test_gpu_buffer_growth.py drives the library through them; tests/test_buffer_growth_cpu.py recomputes every
capacity from the sizing rules of csrc/eppk.hip and holds the sequences to crossing them.  Pure numpy plus oracle/; no GPU.  Loaded by
file name."""
import importlib.util
import os
from typing import Dict, List

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


sc = _load("session_cases")
sc.INDEX_PODS = 60                                             # (this copy of the module only: index entries name pods below the SMALLER publish)

SEED = 9100
CFG = dict(sc.config(SEED), max_pods=130, max_blocks=8, max_batch=64, index_slots=32768, groups=64, pods=(130, 60))
ENV = {"EPPK_QUAD_MIN": "4", "EPPK_BOUND_CHUNK": "64"}
PODS = (130, 130, 60, 60, 60, 60)                              # the snapshot under step i: J = 3, then J = 1 (published once each)
ROWS = (48, 700, 64, 1500)
TOPK = (2, 4, 2, 8)
# The resolves go on for two more steps.  With EPPK_BOUND_CHUNK=64 a batch of at most 64 rows takes the single-launch kernel and never
# asks for the chunk histogram, the band order or the band histogram: over the four steps above those three are made at 700 rows and
# replaced ONCE, at 1500.  A multi-chunk batch that reuses them (200 rows) and one that replaces them again (3100) follow.
EXTRA_ROWS, EXTRA_TOPK = (200, 3100), (2, 4)
ALL_ROWS, ALL_TOPK = ROWS + EXTRA_ROWS, TOPK + EXTRA_TOPK
SUBSET_ROWS_ENTRIES = ((60, 10), (55, 20), (60, 5), (60, 35))  # rows x entries each: 600 / 1100 / 300 / 2100 entries in all
INSERT_PAIRS = (3000, 5000, 1000, 9000)
RESIDENT_ROWS = 8
def steps_of(buffer: str) -> int:
    return 6 if buffer == "resolves" else 4


BUFFERS = ("work_list", "fallback_lists", "learn_words", "filter_mask", "subset_keys", "index_insert", "resolves")
BANDS3 = ((sc.SHED, 0), (sc.SPILL, 1), (sc.SHED, 1))
CHUNK = 64
EPPK_MAX_TOPK, EPPK_MAX_PODS, EPPK_MAX_BANDS, BAND_SEG_WORDS = 8, 4096, 8, 16


# ---- the sizing rules of csrc/eppk.hip, restated: units a step asks of its buffer, and what the buffer then holds --------------------------

def work_list_words(n: int, masked: bool) -> int:
    """launch_pick: 512-thread workgroups of pick_quad_kernel (8 wavefronts, 4 requests each); while the grid is not clipped by the
    device (47 workgroups at 1500 rows) every wavefront is a segment with room for its 4 requests; a masked batch parks 34 words a row."""
    nblk = (n + 3) // 4
    segs = 8 * ((nblk + 7) // 8)
    defer_cap = 4 * ((nblk + segs - 1) // segs)
    return 32 + segs + segs * defer_cap * (34 if masked else 1)


def need_of(buffer: str, i: int) -> Dict[str, int]:
    """Units asked of each buffer the entry point of `buffer` sizes at step i (the name says what a unit is)."""
    mb, n = CFG["max_batch"], ALL_ROWS[i]
    rows = max(n, mb)                                          # bounded_rows, d_learn, d_fmask: the floor of max_batch rows
    if buffer == "work_list":
        return {"words_unmasked_stream": work_list_words(n, False), "words_masked_stream": work_list_words(n, True)}
    if buffer == "fallback_lists":
        return {"rs_entries": n * TOPK[i]}
    if buffer == "learn_words":
        return {"learn_rows": rows}
    if buffer == "filter_mask":
        return {"fmask_rows": rows}
    if buffer == "subset_keys":
        total = SUBSET_ROWS_ENTRIES[i][0] * SUBSET_ROWS_ENTRIES[i][1]
        cap = 1024
        while cap < total:
            cap *= 2
        return {"sk_entries": cap, "so_offsets": mb + 1}
    if buffer == "index_insert":
        pairs = INSERT_PAIRS[i]
        return {"sortwl_words": 4 + max(4096, min(pairs, 1 << 24)), "tmp_bytes": pairs * 12}
    if buffer == "resolves":
        # bounded_resolve / banded_resolve / costed_resolve: the request states only for a call that takes no ranks (the step's last
        # resolve: tests/test_gpu_buffer_growth.py run_resolves), the lists for the pick_*_device forms (two of the three at every step);
        # a batch of at most one chunk returns through the single-launch kernel and asks for nothing else.  (d_cs_acc and d_bd_pods
        # hold EPPK_MAX_PODS words whatever the batch: made once, not part of the sequence.)
        need = {"bd_state_rows": rows, "bd_list_rows": rows}
        if n > CHUNK:
            chunks = (n + CHUNK - 1) // CHUNK
            need.update({"bd_hist_words": chunks * PODS[i], "bn_perm_rows": rows, "bn_bh_words": BAND_SEG_WORDS + chunks * EPPK_MAX_BANDS})
        return need
    raise ValueError(buffer)


def growth(buffer: str) -> Dict[str, List[str]]:
    """Per buffer of the case, what eppk::grow does at each step: 'first', 'replace', 'reuse', or 'none' where the step does not ask."""
    n = steps_of(buffer)
    names = sorted({name for i in range(n) for name in need_of(buffer, i)})
    out: Dict[str, List[str]] = {name: [] for name in names}
    cap = {name: 0 for name in names}
    for i in range(n):
        asked = need_of(buffer, i)
        for name in names:
            if name not in asked:
                out[name].append("none")
                continue
            need = max(asked[name], 1)
            out[name].append("reuse" if cap[name] >= need else "first" if cap[name] == 0 else "replace")
            cap[name] = max(cap[name], need)
    return out


# ---- the model and the steps -------------------------------------------------------------------------------------------------------------

def make_model(orc, workload, cfg=None, seed=SEED):
    cfg = dict(CFG if cfg is None else cfg)
    m = sc.Model(seed, orc, workload)
    m.cfg, m.pool, m.B = cfg, sc.Pool(cfg), cfg["max_blocks"]
    return m


def publish_step(P: int, seed: int = 11) -> Dict:
    return dict(fam="snapshot", op="publish", seed=seed + P, P=P, kind="workload", holes=False, qmode="a", kvmode="a")


def seed_step() -> Dict:
    return dict(fam="index", op="seed_index", seed=1, call=0, of=1)


def step(op: str, i: int, **kw) -> Dict:
    base = dict(fam="picks", op=op, seed=SEED + 17 * i + len(op), R=ALL_ROWS[i], k=ALL_TOPK[i], stream=i % 2, assumed=0, masked=False, local=True, case=0)
    base.update(kw)
    return base


def resolve_step(kind_form: str, i: int, j: int) -> Dict:
    """A load resolve of ALL_ROWS[i] requests; j = its place among the three of the step (bounded, banded with three bands, costed)."""
    return dict(fam="resolve", op=kind_form, seed=SEED + 100 * i + j, R=ALL_ROWS[i], k=ALL_TOPK[i], policy=(sc.SHED, sc.SPILL)[(i + j) & 1], cap_array=bool((i + j) % 3 == 1),
                load=("fresh", "none", "fresh")[j], bands=BANDS3 if "banded" in kind_form else BANDS3[:1 + (i % 3)], masked=bool(i == 1 and j == 0), per_entry=bool(j & 1),
                stream=(i + j) % 3, refused=False)


def resolve_forms(i: int) -> List[str]:
    """bounded, banded, costed in turn, each in its pick_*_device form and in its resolve-alone form (over the lists of the model)."""
    alone = i % 3                                              # which of the three takes the resolve-alone form at this step
    return [("resolve_%s_device" if j == alone else "pick_%s_device") % kind for j, kind in enumerate(("bounded", "banded", "costed"))]


def insert_pairs(m, i: int):
    """INSERT_PAIRS[i] (hash, pod) pairs over a recurring pool of 3000 hashes, three pods each: live hashes stay below index_slots / 4."""
    rng = np.random.default_rng(SEED + 5)
    pool = rng.integers(1, 1 << 63, 3000, dtype=np.uint64)
    n = INSERT_PAIRS[i]
    h = np.repeat(pool[: (n + 2) // 3], 3)[:n]
    p = ((np.arange(n) % 3) * 19 + (np.arange(n) // 3) % 17).astype(np.uint32) % np.uint32(m.pool.ipods)
    order = np.argsort(p, kind="stable")
    return np.ascontiguousarray(h[order]), np.ascontiguousarray(p[order])


def subset_filters(endpoints, i: int, seed: int = SEED) -> List[str]:
    rows, per = SUBSET_ROWS_ENTRIES[i]
    rng = np.random.default_rng(seed + i)
    out = []
    for _ in range(rows):
        idx = rng.choice(len(endpoints), per, replace=False)          # (distinct entries: the count is what sizes the staging)
        out.append(",".join(endpoints[j].address + (":" + endpoints[j].port if j & 1 else "") for j in idx))
    return out
