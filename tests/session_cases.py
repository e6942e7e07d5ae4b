"""Test-side generator of SESSIONS and their reference model: one long-lived context, every feature interleaved on it.

A session is a seeded list of steps (an operation and its arguments) for ONE eppk_ctx; the model applies the same step to reference state
-- the pods as they now stand (assumed-load bumps included), an OracleIndex, the filter programs, the assumed-load setting -- and returns
what the library must return, bit for bit.  tests/test_gpu_session.py drives the library through the steps; tests/test_session_cpu.py
holds this generator to the coverage that module relies on.  Pure numpy plus oracle/ and the numpy restatements beside this file
(filter_ref, bounded_ref, banded_ref, costed_ref, wrand_ref); no GPU.  Loaded by file name.

Order of steps.  A session is a PROLOGUE (publish, the index built in 20 inserts, an eligible batch, a batch that defers above the pause
threshold of the quad route, an eligible batch, a masked pick, filter programs set and the planes built, pick_filtered on 5 and on 256
rows, a resolve alone over the filtered lists, the three resolves, two small plain batches), a WALK and an EPILOGUE (programs set,
pick_filtered, a publish that changes J, pick_filtered again with no set_filters between; programs with thresholds at the medians
of the new gauges, so that the bump moves pods across them; filter, assumed load on, a pick that bumps
the rows, a filter, assumed load off, a filter, pick_filtered and a resolve alone over its lists; a masked pick; the three resolves,
the last two over 18 chunks of 64 rows and without `load`, one behind the other; a batch of one).  Programs stay set from the prologue
on but for the stretch behind a set_filters_none of the walk, so pick_filtered builds or reuses planes and fills d_fmask in every
session.  The batch that defers is one whose rows all carry a reserved hash (odd seeds: above n/4 of an unmasked batch) or one in
which every sixth row does (even seeds: between n/8 and n/4 -- unmasked it leaves the route on, masked, behind it, it pauses it).
The walk lays the eight operation families along an Eulerian circuit of the complete directed graph on them, loops
included: 65 steps in which every ordered pair of families, a family after itself among them, occurs exactly once; the seed rotates the
circuit and draws the arguments.  What an operation does while assumed load is on is decided by the plan (the library refuses the
load resolves then, and the oracle has a restatement of the plain pick only): the plain and the random pickers become `pick`, the
filter keeps its host forms, a load resolve becomes the refusal it is.

Sizes.  max_pods 1024, max_blocks 8, batches R in {1, 5, 64, 65, 256, 700, 1100} (R <= 64 where the reference is R x P score_row calls),
P in {65, 130, 1000} (J = 2, 3, 16).  One session at max_pods 4096 / max_blocks 32 (P up to 4096: the u64 lane word).

index_slots.  eppk.hip: sets_cap = max(1024, slots / 16) lines of interned sets, capacity slots / 2 live hashes, and sortwl_finish
rebuilds the set table once `used > sets_cap / 2` has been reported and 16 canon passes have gone by.  The small sessions take
index_slots = 16384: sets_cap = 1024, so the 640 groups of the pool -- each with a three-pod set of its own -- put 640 > 512 listed sets
into the table; the prologue inserts them in 20 calls (20 canon passes > 16), so the rebuild happens inside the prologue's inserts or
at the first update of the walk, with picks on both sides of it.  Live hashes stay below 640 * 4 shared + 512 * 4 tail (the request
pool: tails recur) + 9 * 64 fresh = 5184 < 8192.  The large session takes 65536 slots (160 groups * 16 + 512 * 16 + 576 = 11328 < 32768)."""
import importlib.util
import os
import sys
import zlib
from typing import Dict, List

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


vc = _load("value_cases")
fc = _load("filter_cases")
fr = fc.ref
br = _load("bounded_ref")
nr = _load("banded_ref")
cr = _load("costed_ref")
wr = _load("wrand_ref")
ng = _load("narrow_grid")

FAMILIES = ("snapshot", "index", "picks", "random", "assumed", "filter", "resolve", "refusal")
CHAIN = [(1, 2), (2, 2), (3, 1), (4, 3)]                       # queue, kv, lora, prefix: the chain the quad route serves
SIZES = (65, 1100, 5, 700, 64, 256, 1)                         # a larger batch after a smaller one, and a smaller one after a larger one
RESOLVE_SIZES = (700, 5, 1100, 65, 64, 256, 1)                 # the load resolves count their own: one chunk and many chunks inside every walk
QUAD_KINDS = ("eligible", "moderate", "heavy", "heavy_masked", "after")
DEFER_KIND = "reserved"                                        # narrow_grid.KINDS: a reserved hash among the blocks, the quad kernel defers the row
assert DEFER_KIND in ng.KINDS
SMALL_SIZES = (5, 64, 1, 33)                                   # where the reference is R x P score_row calls
INDEX_PODS = 65                                                # index entries name pods below the smallest snapshot
N_POOL = 512
SEEDS = (7101, 7102, 7103)
BIG_SEED = 7240
SHED, SPILL = br.SHED, br.SPILL
PER_ENTRY = 1

LIST_FORMS = ("resolve_banded_device", "resolve_bounded_device", "resolve_costed_device")        # the resolve alone, over lists of an earlier step
OWN_FORMS = ("pick_bounded", "pick_costed_device", "pick_banded", "pick_bounded_device", "pick_costed", "pick_banded_device")
RESOLVE_OPS = LIST_FORMS + OWN_FORMS
PICK_OPS = ("pick", "pick_topk", "pick_device", "pick_masked", "learn_then_pick", "pick_candidates", "pick_staged", "stage_pair", "pick_topk_masked")
RANDOM_OPS = ("random_topk", "weighted_random", "weighted_random_masked", "random_topk_masked")
# (programs are set from the prologue on: every pick_filtered of this cycle but one right behind set_filters_none finds some, whatever its start)
FILTER_OPS = ("set_filters", "pick_filtered", "filter_masks", "filter_masks_device", "pick_filtered", "set_filters_none", "filter_masks", "set_filters",
              "pick_filtered")
INDEX_OPS = ("insert", "insert_picks_device", "remove_pod", "tick_evict", "insert", "trim", "insert_picks_device", "clear", "insert")
REFUSALS = ("bad_policy", "bad_row", "bad_reserves", "too_many_programs", "end_without_begin", "bad_band", "bad_class")


def config(seed: int) -> Dict:
    big = seed == BIG_SEED
    return dict(seed=seed, max_pods=4096 if big else 1024, max_blocks=32 if big else 8, max_batch=1100, index_slots=65536 if big else 16384,
                groups=160 if big else 640, pods=(65, 4096, 130, 2500, 1000) if big else (65, 1000, 130), chain=CHAIN)


def euler_walk(n: int, rot: int) -> List[int]:
    """An Eulerian circuit of the complete directed graph with loops on n nodes (Hierholzer; the successors of a node are tried in an
    order the rotation fixes): n * n + 1 nodes, every ordered pair once."""
    left = {a: [(a + rot + d) % n for d in range(n)] for a in range(n)}
    stack, out = [rot % n], []
    while stack:
        a = stack[-1]
        if left[a]:
            stack.append(left[a].pop(0))
        else:
            out.append(stack.pop())
    return out[::-1]


# ---- the pool: groups with a pod set of their own, and the request rows drawn from them ----------------------------------------------------

class Pool:
    def __init__(self, cfg: Dict):
        rng = np.random.default_rng(cfg["seed"] * 31 + 5)
        B, G = cfg["max_blocks"], cfg["groups"]
        S = B // 2
        IP = self.ipods = min(INDEX_PODS, cfg["max_pods"])
        self.B, self.S, self.G = B, S, G
        self.shared = rng.integers(1, 1 << 63, (G, S), dtype=np.uint64)
        g = np.arange(G)
        a, t = g % IP, g // IP
        self.sets = np.stack([a, (a + 1 + t) % IP, (a + 20 + 2 * t) % IP], axis=1).astype(np.uint32)      # three distinct pods, a set per group
        self.adapter = np.where(rng.random(G) < 0.25, -1, rng.integers(0, 128, G)).astype(np.int32)
        grp = rng.integers(0, G, N_POOL)
        tails = rng.integers(1, 1 << 63, (N_POOL, B - S), dtype=np.uint64)
        nb = np.where(rng.random(N_POOL) < 0.2, rng.integers(0, B + 1, N_POOL), B)
        self.rows = vc.make_req_rows(self.adapter[grp], nb, np.concatenate([self.shared[grp], tails], axis=1), B)
        # the rows that defer are narrow_grid's kind DEFER_KIND, built as tests/test_gpu_narrow_grid.py builds it: the same rows, all their
        # blocks counted, with a reserved hash (0 and ~0 in turn) at a position that moves through the row
        self.defer = self.rows.copy()
        self.defer[:, 0] = (self.defer[:, 0] & np.uint64(0xFFFFFFFF)) | (np.uint64(B) << np.uint64(32))
        self.defer[np.arange(N_POOL), 1 + (np.arange(N_POOL) % B)] = np.where(np.arange(N_POOL) & 1, np.uint64(0), np.uint64(0xFFFFFFFFFFFFFFFF))

    def pairs(self, lo: int, hi: int):
        """The (hash, pod) pairs of groups [lo, hi), by pod in ascending order."""
        h = np.repeat(self.shared[lo:hi].reshape(-1), 3)
        p = np.tile(self.sets[lo:hi][:, None, :], (1, self.S, 1)).reshape(-1)
        order = np.argsort(p, kind="stable")
        return h[order], p[order]

    def seed_call(self, c: int):
        """Call c of the prologue: call 0 inserts every group; call c >= 1 puts the blocks of eight groups on one more pod, so that their
        set becomes a new one of four pods and leaves its line in the set table behind."""
        if c == 0:
            return self.pairs(0, self.G)
        g = np.arange(8 * (c - 1), 8 * c)
        return self.shared[g].reshape(-1).copy(), np.repeat((self.sets[g, 0] + 40) % self.ipods, self.S).astype(np.uint32)


def deferring(rows: np.ndarray) -> np.ndarray:
    """bool [R]: a reserved hash (0 or ~0) among the row's n_blocks hashes."""
    nb = (rows[:, 0] >> np.uint64(32)).astype(np.int64)
    h = rows[:, 1:]
    inside = np.arange(h.shape[1])[None, :] < nb[:, None]
    return np.any(inside & ((h == 0) | (h == np.uint64(0xFFFFFFFFFFFFFFFF))), axis=1)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------------

def make_session(seed: int) -> List[Dict]:
    """The steps of session `seed`: dicts of small scalars (op, family, sizes, a data seed); the model draws the arrays from them."""
    cfg = config(seed)
    rng = np.random.default_rng(seed)
    n = seed % 97
    steps: List[Dict] = []
    st = dict(P=0, assumed=0, nprog=0, lists=False, load=False, pub=0, size=n, small=n, stream=n, lform=n, oform=n, listed=False, part="prologue", cnt={f: n for f in FAMILIES})

    def add(fam, op, **kw):
        steps.append(dict(fam=fam, op=op, part=st["part"], seed=int(rng.integers(1, 1 << 31)), **kw))

    def size():
        st["size"] += 1
        return SIZES[st["size"] % len(SIZES)]

    def small():
        st["small"] += 1
        return SMALL_SIZES[st["small"] % len(SMALL_SIZES)]

    def stream():
        st["stream"] += 1
        return st["stream"] % 3

    def publish(avoid=0, qmode=None):
        i = st["pub"]
        st["pub"] += 1
        P = next(cfg["pods"][(i + n + d) % len(cfg["pods"])] for d in range(3) if cfg["pods"][(i + n + d) % len(cfg["pods"])] not in (st["P"], avoid))
        add("snapshot", "publish", P=P, kind=("workload", "values")[i & 1], holes=(i % 3 == 1), qmode=qmode or vc.QUEUE_MODES[(i + n) % 6], kvmode=vc.KV_MODES[(i // 2 + n) % 4])
        st.update(P=P, lists=False, load=False)

    def resolve(op, fam="resolve", refused=False, R=None, load=None):
        i = st["cnt"]["resolve"]
        kw = dict(k=(4, 2, 8, 3)[i % 4], policy=(SHED, SPILL)[i & 1], cap_array=bool(i % 3 == 1), load=("none", "fresh", "fresh")[i % 3],
                  bands=((SHED, 0), (SPILL, 1), (SHED, 1), (SPILL, 3))[: 1 + i % 4], masked=bool(i % 4 == 2), per_entry=bool(i & 1), stream=stream(), refused=refused)
        if st["load"] and i % 3 != 0:                          # the load an earlier resolve left behind, when there is one
            kw["load"] = "carried"
        if load == "carried" and not st["load"]:
            load = "fresh"
        if load is not None:
            kw["load"] = load
        if op is None:                                         # lists of an earlier step since the last publish: every other resolve takes them
            if (st["lists"] or refused) and not st["listed"]:
                op = LIST_FORMS[st["lform"] % 3]
                st["lform"] += 1
            else:
                op = OWN_FORMS[st["oform"] % 6]
                st["oform"] += 1
            st["listed"] = op in LIST_FORMS
        if not op.startswith("resolve_"):
            kw["R"] = RESOLVE_SIZES[i % len(RESOLVE_SIZES)] if R is None else R
        add(fam, op, **kw)
        if kw["load"] != "none" and not refused:
            st["load"] = True

    def family(fam, pair=None):
        i = st["cnt"][fam]
        st["cnt"][fam] += 1
        on = st["assumed"] != 0
        if fam == "snapshot":
            publish()
        elif fam == "index":
            op = INDEX_OPS[i % len(INDEX_OPS)]
            add(fam, op, R=small(), stream=stream(), pod=int(rng.integers(0, INDEX_PODS)), cap=int(rng.integers(8, 40)), keep=int(rng.integers(1, 3)))
        elif fam == "picks":
            op = PICK_OPS[i % len(PICK_OPS)]
            if on:
                op = ("pick", "pick_masked")[i & 1]
            R = small() if op in ("pick", "pick_staged", "pick_candidates", "learn_then_pick") and not on else size()      # (small plain batches: what rings a resident unit)
            add(fam, op, R=R, k=(4, 1, 8, 2)[i % 4], stream=stream(), assumed=st["assumed"])
            if op.startswith("pick_topk") and not on:
                st["lists"] = True
        elif fam == "random":
            op = RANDOM_OPS[i % len(RANDOM_OPS)]
            if on:
                op = ("pick_masked", "pick")[i & 1]
            R = small() if op.startswith("weighted") else size()
            add(fam, op, R=R, k=(4, 1)[(i // 2) & 1] if op.startswith("weighted") else (3, 1, 8)[i % 3], assumed=st["assumed"], stream=stream())
            if op.startswith("weighted") and steps[-1]["k"] > 1:
                st["lists"] = True
        elif fam == "assumed":
            E = (1, 3)[(i // 4) & 1] if (i % 4 == 0 and not on) else 0      # (E = 0 while it is off: a call that changes nothing)
            add(fam, "set_assumed_load", E=E)
            st["assumed"] = E
        elif fam == "filter":
            op = FILTER_OPS[i % len(FILTER_OPS)]
            if on and op in ("pick_filtered", "filter_masks_device"):
                op = "filter_masks"
            add(fam, op, R=size(), k=(2, 4, 1)[i % 3], stream=stream(), local=bool(i & 1), masked=bool(i % 3 != 0), case=fc.SEED0 + (n + i) % fc.N_SEEDS)
            if op.startswith("set_filters"):
                st["nprog"] = 0 if op.endswith("none") else 4
            if op == "pick_filtered":
                st["lists"] = True
        elif fam == "resolve":
            resolve(None, refused=on, load={"first": "fresh", "second": "carried"}.get(pair))      # (a resolve behind a resolve takes the load the first left)
        elif fam == "refusal":
            if on:
                resolve(None, fam, refused=True)
            else:
                op = REFUSALS[i % len(REFUSALS)]
                if op == "bad_class" and not st["nprog"]:
                    op = "bad_row"
                add(fam, op, R=small())

    # prologue
    publish()
    for c in range(20):
        add("index", "seed_index", call=c, of=20)
    # an eligible batch, one that defers above the pause threshold, an eligible one: odd seeds an unmasked batch above n/4; even seeds a
    # share between n/8 and n/4, which leaves the route on behind an unmasked batch ("moderate") and pauses it behind a masked one
    for quad in (("eligible", "moderate", "heavy_masked", "after") if seed % 2 == 0 else ("eligible", "heavy", "after")):
        add("picks", "pick", R=256, k=1, stream=0, assumed=0, quad=quad)
    add("picks", "pick_masked", R=256, k=1, stream=0, assumed=0)
    # the filter with programs from here on: planes built, then pick_filtered on a small batch and on a larger one (d_fmask grows), and a
    # resolve alone over the filtered lists
    add("filter", "set_filters", R=64, k=1, stream=0, local=True, masked=False, case=fc.SEED0)
    st["nprog"] = 4
    add("filter", "filter_masks", R=65, k=1, stream=0, local=True, masked=True, case=fc.SEED0)
    add("filter", "pick_filtered", R=5, k=4, stream=0, local=True, masked=True, case=fc.SEED0)
    add("filter", "pick_filtered", R=256, k=4, stream=0, local=True, masked=False, case=fc.SEED0)
    st["lists"] = True
    st["cnt"]["resolve"] += 1
    resolve("resolve_bounded_device")
    for op, R in (("pick_bounded", 1100), ("pick_banded", 5), ("pick_costed", 700)):
        st["cnt"]["resolve"] += 1
        resolve(op, R=R)
    add("picks", "pick", R=5, k=1, stream=0, assumed=0)            # small plain batches: what rings a resident unit under EPPK_RESIDENT=1
    add("picks", "pick_topk", R=5, k=4, stream=0, assumed=0)
    st["lists"] = True
    first_P = st["P"]
    # the walk
    st["part"] = "walk"
    walk = [FAMILIES[f] for f in euler_walk(len(FAMILIES), n)]
    for j, fam in enumerate(walk):
        twice = fam == "resolve" and ((j + 1 < len(walk) and walk[j + 1] == fam) or (j and walk[j - 1] == fam))
        family(fam, pair=("second" if j and walk[j - 1] == fam else "first") if twice else None)
    # epilogue
    st["part"] = "epilogue"
    if st["assumed"]:
        add("assumed", "set_assumed_load", E=0)
        st["assumed"] = 0
    # programs are set BEFORE the publish and not again: pick_filtered on each side of a publish that changes J finds planes that only the
    # publish can have made stale; a larger batch behind a smaller one again
    add("filter", "set_filters", R=64, k=1, stream=0, local=True, masked=False, case=fc.SEED0)
    add("filter", "pick_filtered", R=64, k=2, stream=0, local=True, masked=True, case=fc.SEED0)
    publish(avoid=first_P, qmode="f")                           # (queue gauges of 0 .. 63 where value_cases draws them: a bump of a few requests crosses a threshold)
    add("filter", "pick_filtered", R=700, k=2, stream=0, local=True, masked=True, case=fc.SEED0)
    # ... then thresholds from the gauges as they now stand (the bump must move pods across them), and nothing but the bump between the
    # filter calls on its two sides
    add("filter", "set_filters", R=64, k=1, stream=0, local=True, masked=False, case=fc.SEED0)
    add("filter", "filter_masks", R=64, k=1, stream=0, local=True, masked=True, case=fc.SEED0)
    add("assumed", "set_assumed_load", E=3)
    add("picks", "pick", R=700, k=1, stream=0, assumed=3)
    add("filter", "filter_masks", R=64, k=1, stream=0, local=True, masked=True, case=fc.SEED0)
    add("assumed", "set_assumed_load", E=0)
    add("filter", "filter_masks", R=64, k=1, stream=0, local=True, masked=False, case=fc.SEED0)
    add("filter", "pick_filtered", R=65, k=4, stream=0, local=True, masked=False, case=fc.SEED0)       # ... and behind the bump, its lists to a resolve alone
    st["lists"] = True
    st["cnt"]["resolve"] += 1
    resolve("resolve_costed_device")
    add("picks", "pick_masked", R=65, k=1, stream=0, assumed=0)
    # (two multi-chunk resolves without `load`, one behind the other: the second finds the first one's loads in the shared scratch row)
    for op, R, load in (("pick_bounded", 65, None), ("pick_banded_device", 1100, "none"), ("pick_costed", 1100, "none")):
        st["cnt"]["resolve"] += 1
        resolve(op, R=R, load=load)
    add("picks", "pick", R=1, k=1, stream=0, assumed=0)
    for i, s in enumerate(steps):
        s["i"] = i
    return steps


def describe(s: Dict) -> str:
    return s["op"] + "(" + ", ".join(f"{k}={v}" for k, v in s.items() if k not in ("op", "fam", "i", "part")) + ")"


def trail(steps: List[Dict], i: int, last: int = 12) -> str:
    return " > ".join(f"{s['i']}:{s['op']}" for s in steps[max(0, i - last):i])


def where(seed: int, steps: List[Dict], i: int) -> str:
    """What a failure message names: seed, step number, operation and arguments, and the operations before it."""
    return f"session seed {seed} step {i} of {len(steps)}: {describe(steps[i])}; before it: {trail(steps, i)}"


# ---- the model ------------------------------------------------------------------------------------------------------------------------------

class Refused(Exception):
    """The step is one the state forbids: the library must raise, report launch status 0 and change nothing."""


class Model:
    def __init__(self, seed: int, orc, workload):
        self.cfg = config(seed)
        self.orc, self.workload = orc, workload
        self.pool = Pool(self.cfg)
        self.B = self.cfg["max_blocks"]
        self.pods = np.zeros(0, dtype=vc.POD_DTYPE)
        self.oix = orc.OracleIndex()
        self.programs: List = []
        self.assumed = 0
        self.lists = None                                      # (picks [R, k] i32, scores [R, k] f64) of the latest list-making step
        self.load = None                                       # the load a resolve left behind, carried to the next call
        self.updates = 0                                       # index updates so far
        self.keys = set()
        self.unbumped = None                                   # the pods as they stood before the latest assumed-load bump of this snapshot
        self.stale = None                                      # what the latest filter step would give on them: for the twin

    # -- data drawn from a step -----------------------------------------------------------------------------------------------------------
    @property
    def P(self):
        return self.pods.shape[0]

    def rows(self, s, R=None, salt=0, defer=False):
        rng = np.random.default_rng(s["seed"] + salt)
        idx = rng.integers(0, N_POOL, s["R"] if R is None else R)
        return np.ascontiguousarray((self.pool.defer if defer else self.pool.rows)[idx])

    def mask(self, s, R, salt=0, sparse=False):
        rng = np.random.default_rng(s["seed"] + 77 + salt)
        dens = rng.choice([0.04, 0.04] if sparse else [0.05, 0.5, 0.9, 1.0], R)
        bits = rng.random((R, self.P)) < dens[:, None]
        if R > 2:
            bits[R // 2] = False                               # a row without candidates
        return vc.mask_words(bits)

    def _topk(self, reqs, k, mask=None):
        p, sc = self.orc.pick_topk_batch(CHAIN, self.pods, self.oix, reqs, self.B, k, mask=mask, threads=4)
        return np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(sc, dtype=np.float64)

    def _pick(self, reqs, mask=None):
        if self.assumed:
            self.unbumped = self.pods.copy()
            return self.orc.pick_batch_assumed(CHAIN, self.pods, self.oix, reqs, self.B, self.assumed, mask)
        return self.orc.pick_batch(CHAIN, self.pods, self.oix, reqs, self.B, mask)[:2]

    def _learn(self, reqs, picks):
        self.oix.insert_picks(reqs, self.B, picks)
        nb = (reqs[:, 0] >> np.uint64(32)).astype(np.int64)
        for r in np.nonzero(picks >= 0)[0]:
            self.keys.update(reqs[r, 1:1 + nb[r]].tolist())
        self.updates += 1

    def _insert(self, h, p):
        self.oix.insert(h, p, snapshot=self.pods)
        self.keys.update(np.asarray(h).tolist())
        self.updates += 1

    def listed_sets(self) -> int:
        """Distinct pod sets of 2 .. 24 pods among the live hashes: what the set table has to hold."""
        sets = set()
        for h in self.keys:
            pods = self.oix.lookup(h, 64)
            if 2 <= pods.size <= 24:
                sets.add(tuple(sorted(pods.tolist())))
        return len(sets)

    def local_programs(self):
        """Programs with thresholds from the gauges as they stand: every stage narrows, waives or sheds something."""
        live = (self.pods["flags"] & 1) == 0
        q, r = self.pods["queue"][live].astype(np.int64), self.pods["running"][live].astype(np.int64)
        qm, rm = int(np.median(q)), int(r.min())
        kv = self.pods["kv_util"][live]
        kvm = float(np.nanmedian(kv)) if np.isfinite(kv).any() else 0.5
        return [[(fr.QUEUE_LE, fr.PREFER, qm), (fr.KV_LE, fr.PREFER, kvm), (fr.LORA_SERVABLE, fr.PREFER, 0), (fr.QUEUE_WITHIN, fr.REQUIRE, 2)],
                [(fr.RUNNING_LE, fr.REQUIRE, rm)],
                [(fr.LORA_LOADED, fr.REQUIRE, 0), (fr.QUEUE_WITHIN, fr.PREFER, 1)],
                [(fr.QUEUE_LE, fr.REQUIRE, int(q.min())), (fr.RUNNING_LE, fr.PREFER, rm)]]

    def _cls(self, s, R):
        if not self.programs:
            return None
        return np.random.default_rng(s["seed"] + 9).integers(0, len(self.programs), R).astype(np.uint8)

    def _adapter(self, reqs):
        return (reqs[:, 0] & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)

    # -- one step -------------------------------------------------------------------------------------------------------------------------
    def apply(self, s: Dict):
        """(inputs, want): the arrays the library is to be called with and what it must return; raises Refused (with the inputs) for a
        step the state forbids."""
        op = s["op"]
        fn = getattr(self, "op_" + op, None)
        if fn is not None:
            return fn(s)
        if s["fam"] in ("resolve", "refusal") and (op in RESOLVE_OPS):
            return self.resolve(s)
        raise ValueError(op)

    def op_publish(self, s):
        P = s["P"]
        rng = np.random.default_rng(s["seed"])
        pods = self.workload.make_pods(s["seed"], P, 128) if s["kind"] == "workload" else vc.make_pods(rng, P, s["qmode"], s["kvmode"])
        pods = np.ascontiguousarray(pods, dtype=vc.POD_DTYPE)
        if s["holes"]:
            pods["flags"] = (rng.random(P) < 0.1).astype(np.uint32)
            pods["flags"][rng.choice(P, 2, replace=False)] = 0
        self.pods = pods.copy()
        self.oix.scrub_inactive(self.pods)
        self.lists, self.load, self.unbumped = None, None, None
        return dict(pods=pods), dict(size=self.oix.size())

    def op_seed_index(self, s):
        h, p = self.pool.seed_call(s["call"])
        self._insert(h, p)
        return dict(hashes=h, pods=p), dict(size=self.oix.size())

    def op_insert(self, s):
        rng = np.random.default_rng(s["seed"])
        if s["seed"] & 1:                                      # fresh hashes
            h = rng.integers(1, 1 << 63, 64, dtype=np.uint64)
        else:                                                  # a known prefix on one more pod: its set grows, the earlier set is left behind
            h = self.pool.shared[rng.integers(0, self.pool.G, 64), rng.integers(0, self.pool.S, 64)]
        p = rng.integers(0, self.pool.ipods, 64).astype(np.uint32)
        self._insert(h, p)
        return dict(hashes=h, pods=p), dict(size=self.oix.size())

    def op_insert_picks_device(self, s):
        reqs = self.rows(s)
        picks = np.ascontiguousarray(self.orc.pick_batch(CHAIN, self.pods, self.oix, reqs, self.B)[0], dtype=np.int32)
        self._learn(reqs, picks)
        return dict(reqs=reqs, picks=picks), dict(size=self.oix.size())

    def op_remove_pod(self, s):
        self.oix.remove_pod(s["pod"])
        self.updates += 1
        return dict(), dict(size=self.oix.size())

    def op_tick_evict(self, s):
        e = self.oix.advance_epoch()
        h, p = self.pool.pairs(0, self.pool.G * 7 // 8)        # seven groups in eight come back and are stamped again; the others age out
        self._insert(h, p)
        n = self.oix.evict_older(e - s["keep"] + 1)
        self.updates += 1
        return dict(hashes=h, pods=p, min_epoch=e - s["keep"] + 1), dict(epoch=e, evicted=n, size=self.oix.size())

    def op_trim(self, s):
        counts = np.zeros(self.cfg["max_pods"], dtype=np.int64)
        for h in self.keys:
            counts[self.oix.lookup(h, 64)] += 1
        cap = int(np.percentile(counts[counts > 0], 85)) if counts.any() else s["cap"]     # the pods listed most lose their oldest epochs
        n = self.oix.trim_pods(self.cfg["max_pods"], cap)
        self.updates += 1
        return dict(cap=cap), dict(removed=n, size=self.oix.size())

    def op_clear(self, s):
        self.oix.clear()
        self.keys.clear()
        h, p = self.pool.pairs(0, self.pool.G)                 # ... and every group again, in one call
        self._insert(h, p)
        return dict(hashes=h, pods=p), dict(size=self.oix.size())

    def op_set_assumed_load(self, s):
        self.assumed = s["E"]
        return dict(), dict()

    def op_pick(self, s, masked=False):
        quad = s.get("quad")
        reqs = self.rows(s, defer=quad == "heavy")
        if quad in ("moderate", "heavy_masked"):               # every sixth row defers: a share between 1/8 and 1/4
            sixth = np.arange(reqs.shape[0]) % 6 == 0
            reqs[sixth] = self.rows(s, defer=True)[sixth]
        mask = self.mask(s, reqs.shape[0]) if masked else None
        if quad == "heavy_masked":                             # masked, every pod a candidate: nothing but the reserved hashes defers a row
            mask = vc.mask_words(np.ones((reqs.shape[0], self.P), dtype=bool))
        p, sc = self._pick(reqs, mask)
        return dict(reqs=reqs, mask=mask), dict(picks=p, scores=sc)

    def op_pick_masked(self, s):
        return self.op_pick(s, True)

    op_pick_device = op_pick
    op_pick_staged = op_pick

    def op_pick_topk(self, s, masked=False):
        reqs = self.rows(s)
        mask = self.mask(s, reqs.shape[0]) if masked else None
        self.lists = self._topk(reqs, s["k"], mask)
        return dict(reqs=reqs, mask=mask), dict(picks=self.lists[0], scores=self.lists[1])

    def op_pick_topk_masked(self, s):
        return self.op_pick_topk(s, True)

    def op_pick_candidates(self, s):
        reqs = self.rows(s)
        mask = self.mask(s, reqs.shape[0], sparse=True)
        p, sc = self._topk(reqs, s["k"], mask)
        return dict(reqs=reqs, mask=mask), dict(picks=p, scores=sc)

    def op_learn_then_pick(self, s):
        reqs = self.rows(s)
        p0, s0 = self.orc.pick_batch(CHAIN, self.pods, self.oix, reqs, self.B)[:2]
        self._learn(reqs, p0)
        p1, s1 = self.orc.pick_batch(CHAIN, self.pods, self.oix, reqs, self.B)[:2]       # the same rows again: they find what was learnt
        return dict(reqs=reqs), dict(picks=p0, scores=s0, picks2=p1, scores2=s1, size=self.oix.size())

    def op_stage_pair(self, s):
        a, b = self.rows(s), self.rows(s, salt=1)
        mb = self.mask(s, b.shape[0])
        p0, s0 = self.orc.pick_batch(CHAIN, self.pods, self.oix, a, self.B)[:2]
        self._learn(a, p0)                                     # set 0 begins with LEARN: set 1's pick waits for the update
        p1, s1 = self.orc.pick_batch(CHAIN, self.pods, self.oix, b, self.B, mb)[:2]
        return dict(reqs=a, reqs2=b, mask2=mb), dict(picks=p0, scores=s0, picks2=p1, scores2=s1, size=self.oix.size())

    def op_random_topk(self, s, masked=False):
        reqs = self.rows(s)
        mask = self.mask(s, reqs.shape[0]) if masked else None
        p, sc = self.orc.pick_random_topk(CHAIN, self.pods, self.oix, reqs, self.B, s["k"], s["seed"], mask)
        return dict(reqs=reqs, mask=mask), dict(picks=p, scores=sc)

    def op_random_topk_masked(self, s):
        return self.op_random_topk(s, True)

    def op_weighted_random(self, s, masked=False):
        reqs = self.rows(s)
        R = reqs.shape[0]
        mask = self.mask(s, R) if masked else None
        T = np.stack([self.orc.score_row(CHAIN, self.pods, self.oix, reqs[r], None if mask is None else mask[r]) for r in range(R)])
        p, sc = wr.weighted_random(T, s["k"], s["seed"], np.arange(R))
        if s["k"] > 1:
            self.lists = (np.ascontiguousarray(p, dtype=np.int32), np.ascontiguousarray(sc, dtype=np.float64))
        return dict(reqs=reqs, mask=mask), dict(picks=p, scores=sc)

    def op_weighted_random_masked(self, s):
        return self.op_weighted_random(s, True)

    def op_set_filters(self, s):
        self.programs = self.local_programs() if s["local"] else fc.make_case(s["case"], P=65, R=8)["programs"]
        return dict(programs=self.programs), dict()

    def op_set_filters_none(self, s):
        self.programs = []
        return dict(programs=[]), dict()

    def _filter(self, s, device=False):
        reqs = self.rows(s)
        R = reqs.shape[0]
        mask = self.mask(s, R) if s["masked"] or device else None
        cls = self._cls(s, R)
        if device and cls is not None and R > 3:
            cls[3] = 200                                       # names no program: the device forms answer with a verdict
        words, verdict = fr.filter_mask_words(self.pods, self.programs, self._adapter(reqs), cls, mask)
        self.unfiltered = fr.filter_mask_words(self.pods, [], self._adapter(reqs), None, mask)[0]      # (what the same call gives without programs: for the twin)
        self.stale = None if self.unbumped is None else fr.filter_mask_words(self.unbumped, self.programs, self._adapter(reqs), cls, mask)[0]
        return reqs, mask, cls, words, verdict

    def op_filter_masks(self, s):
        reqs, mask, cls, words, verdict = self._filter(s)
        return dict(reqs=reqs, mask=mask, cls=cls), dict(masks=words, verdict=verdict)

    def op_filter_masks_device(self, s):
        reqs, mask, cls, words, verdict = self._filter(s, device=True)
        return dict(reqs=reqs, mask=mask, cls=cls), dict(masks=words, verdict=verdict)

    def op_pick_filtered(self, s):
        reqs, mask, cls, words, verdict = self._filter(s)
        self.lists = self._topk(reqs, s["k"], words)
        self.filtered = words
        return dict(reqs=reqs, mask=mask, cls=cls), dict(picks=self.lists[0], scores=self.lists[1], verdict=verdict)

    # -- the load resolves ------------------------------------------------------------------------------------------------------------------
    def resolve(self, s):
        op, P = s["op"], self.P
        kind = "bounded" if "bounded" in op else "banded" if "banded" in op else "costed"
        rng = np.random.default_rng(s["seed"] + 3)
        inp = dict(kind=kind)
        if op.startswith("resolve_"):
            if self.lists is None:                             # (a refused step: any lists will do, they are not looked at)
                lists = (np.zeros((5, 2), dtype=np.int32), np.zeros((5, 2), dtype=np.float64))
            else:
                lists = self.lists
            inp.update(lists=lists[0], list_scores=lists[1])
        else:
            reqs = self.rows(s)
            mask = self.mask(s, reqs.shape[0]) if s["masked"] else None
            inp.update(reqs=reqs, mask=mask)
            lists = None if s["refused"] else self._topk(reqs, s["k"], mask)
        R = inp["lists"].shape[0] if "lists" in inp else inp["reqs"].shape[0]
        k = inp["lists"].shape[1] if "lists" in inp else s["k"]
        unit = 4 if kind == "costed" else 1
        cap_all = unit * max(1, (3 * R) // (4 * max(P, 1)) + 1)
        cap = (rng.integers(0, 2 * cap_all + 1, P).astype(np.uint32)) if s["cap_array"] else None
        load = None
        if s["load"] == "fresh":
            load = rng.integers(0, 2, P).astype(np.uint32) * unit
        elif s["load"] == "carried":
            load = self.load.copy()
        bands = [(p, r * unit) for p, r in s["bands"]]
        band = rng.integers(0, len(bands), R).astype(np.uint8) if kind != "bounded" else None
        per_entry = bool(s["per_entry"]) and op == "resolve_costed_device"
        cost = (rng.integers(1, 9, (R, k) if per_entry else R).astype(np.uint32)) if kind == "costed" else None
        inp.update(k=k, R=R, cap=cap, cap_all=cap_all, policy=s["policy"], load=load, bands=bands, band=band, cost=cost, per_entry=per_entry)
        if s["refused"] or self.assumed:
            raise Refused(inp)
        if kind == "bounded":
            want = br.resolve(lists[0], lists[1], P, cap, cap_all, s["policy"], load)
            flags = br.LAUNCH_BAD_PICK if want[4] else 0
        elif kind == "banded":
            want = nr.resolve(lists[0], lists[1], P, bands, band, cap, cap_all, load)
            flags = want[4]
        else:
            want = cr.resolve(lists[0], lists[1], P, cost, bands, band, cap, cap_all, load, per_entry=per_entry)
            flags = want[4]
        assert flags == 0, "the generator makes no bad rows"
        if load is not None:
            self.load = want[3].copy()
        return inp, dict(picks=want[0], scores=want[1], ranks=want[2], load=None if load is None else want[3])

    # -- refusals -----------------------------------------------------------------------------------------------------------------------------
    def _refuse(self, s, **inp):
        raise Refused(dict(reqs=self.rows(s), **inp))

    def op_bad_policy(self, s):
        self._refuse(s)

    def op_bad_reserves(self, s):
        self._refuse(s, bands=[(SHED, 2), (SHED, 1)])

    def op_bad_band(self, s):
        self._refuse(s, bands=[(SHED, 0), (SPILL, 1)], band=np.full(s["R"], 2, dtype=np.uint8), cost=np.ones(s["R"], dtype=np.uint32))

    def op_bad_row(self, s):
        reqs = self.rows(s)
        reqs[reqs.shape[0] // 2, 0] = np.uint64(self.B + 1) << np.uint64(32)              # n_blocks > max_blocks
        raise Refused(dict(reqs=reqs))

    def op_too_many_programs(self, s):
        raise Refused(dict(programs=[[(fr.QUEUE_LE, fr.PREFER, 1)]] * 5))

    def op_end_without_begin(self, s):
        raise Refused(dict())

    def op_bad_class(self, s):
        self._refuse(s, cls=np.full(s["R"], len(self.programs), dtype=np.uint8))


def run_model(seed: int, orc, workload, observe=None):
    """Every step of session `seed` through the model: [(step, inputs, want | None)] -- None for a refused step.  `observe(model, step)`
    is called after each step."""
    steps = make_session(seed)
    m = Model(seed, orc, workload)
    out = []
    for s in steps:
        try:
            inp, want = m.apply(s)
        except Refused as e:
            inp, want = e.args[0], None
        out.append((s, inp, want))
        if observe is not None:
            observe(m, s)
    return out


def digest(run) -> int:
    """A checksum over every byte the model wants from the library."""
    crc = 0
    for s, _, want in run:
        crc = zlib.crc32(repr(sorted((k, v) for k, v in s.items())).encode(), crc)
        for key in sorted(want or {}):
            v = want[key]
            crc = zlib.crc32(key.encode() + (b"" if v is None else np.ascontiguousarray(v).tobytes()), crc)
    return crc
