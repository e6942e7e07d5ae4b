"""Displaced index keys at every probe position, on every pick route, bit for bit against the oracle.

A key whose home bucket is full lives in a later bucket.  Every pick kernel follows such a key with code of its own -- probe() (generic
kernel), pair_probe_finish (fast kernel), the two-pass fetch / walk loop of pick_quad_body (every quad instantiation, launched and resident)
-- and the rest of the suite reaches that code only by crowding a table.  Here tests/index_placement.py PLACES the keys: each of the 32 probe
positions displaced alone, adjacent pairs and runs around the 16 / 17-key limits of the quad kernel's gather, by one bucket, by two, and
wrapped from the last bucket to the front of the table; walks that end in a miss; the two pod sets of a returning request; home buckets
that are all tombstones.  The rows are laid out in the wavefront both alone among rows that stop short and in mixed quadruples, because the
quad kernel decides what to fetch by a vote of the four rows a wavefront scores.

One table holds every chain; each test is one route over the same batch.  tests/test_index_placement_cpu.py checks, without a GPU, that the
plans built here put every key where they say.
"""
import contextlib
import functools
import importlib.util
import os
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ip = _load("index_placement")

Q, KV, L, PF = 1, 2, 3, 4
FUSED = [(Q, 2), (KV, 2), (L, 1), (PF, 3)]               # the headline chain: fast / quad kernels
GENERIC = [(L, 1), (Q, 2), (KV, 2), (Q, 1), (PF, 3)]     # three trailing pod-only scorers: the generic (unfused) kernel, probe()
P, B = 4096, 32
SLOTS, SEED = 1 << 17, 1617
LONG_B, LONG_SLOTS, LONG_SEED = 40, 1 << 13, 4017
FILL_POD, TOMB_POD = 4000, 4001                            # fillers appear in no request; TOMB_POD is removed once the chains are in
N_GROUPS = 8
NBS = (16, 17, 18, 19, 20, 21, 31, 32)
RUNS = [(15, 16), (16, 17), (16, 17, 18), (15, 16, 17), (16, 17, 18, 19), (17, 18), (19, 20), (16, 17, 20), tuple(range(16, 32)),
        tuple(range(32))]
HOWS = (ip.D1, ip.D2, ip.WRAP)


def group_pods(g: int) -> Tuple[int, ...]:
    return tuple(97 * g + o for o in (5, 23, 42, 71))


@dataclass
class Chain:
    name: str
    spec: List[str]
    tail_from: int = 1 << 30                               # keys from here on are cached on ONE pod of the group (a request that came back)
    odd: Dict[int, str] = field(default_factory=dict)    # position -> "list" | "pod": that key's pod set differs from the rest
    limit: bool = False                                    # around the 16 / 17-key limits: also laid out alone in its wavefront, next to a 17-hit row


def _spec(disp=(), how=ip.D1, n=B, absent=None, absent_how=ip.ABSENT):
    s = [ip.HOME] * n
    for i in disp:
        s[i] = how
    if absent is not None:
        s[absent] = absent_how
    return s


def _name(pos):
    pos = list(pos)
    if len(pos) > 4 and pos == list(range(pos[0], pos[-1] + 1)):
        return f"{{{pos[0]}..{pos[-1]}}}"
    return "{" + ",".join(map(str, pos)) + "}"


PLAIN, NONE, M17 = 0, 1, 2                                 # helper chains: all at home; nothing cached; exactly 17 leading hits


def main_chains() -> List[Chain]:
    cs = [Chain("plain", _spec()), Chain("none", [ip.ABSENT] * 4), Chain("m17", _spec(absent=17))]
    for i in range(B):                                     # single positions
        cs.append(Chain(f"single{{{i}}}/d1", _spec([i]), limit=i in (15, 16, 17, 18)))
    for i in (0, 15, 16, 17, 18, 19, 20, 31):
        cs.append(Chain(f"single{{{i}}}/d2", _spec([i], ip.D2)))
        cs.append(Chain(f"single{{{i}}}/w", _spec([i], ip.WRAP)))
    for how in HOWS:                                       # adjacent pairs, runs
        for i in range(B - 1):
            cs.append(Chain(f"pair{{{i},{i + 1}}}/{how}", _spec([i, i + 1], how), limit=how == ip.D1 and 14 <= i <= 19))
        for run in RUNS:
            cs.append(Chain(f"run{_name(run)}/{how}", _spec(run, how), limit=True))
    for a in (0, 15, 16, 17, 18, 20, 31):                  # walks that end in a miss, behind a run of displaced hits
        for ah in (ip.ABSENT_OVF, ip.ABSENT):
            cs.append(Chain(f"miss@{a}/{ah}", _spec(range(max(0, a - 3), a), ip.D1, absent=a, absent_how=ah), limit=True))
    for run in [(15,), (16,), (15, 16), (16, 17), (14, 15, 16, 17), (17, 18), (16, 17, 18, 19)]:   # blocks 0..15 on the group's pods, the tail on one pod
        for how in (ip.D1, ip.D2):
            cs.append(Chain(f"twosets{_name(run)}/{how}", _spec(run, how), tail_from=16, limit=True))
    for pos, kind in [(5, "list"), (16, "list"), (17, "list"), (5, "pod"), (16, "pod"), (17, "pod"), (30, "pod")]:
        cs.append(Chain(f"oddset@{pos}/{kind}", _spec([pos]), odd={pos: kind}, limit=True))
    cs.append(Chain("oddset{16,17}/pod", _spec([16, 17]), odd={16: "pod", 17: "pod"}, limit=True))
    for run in [(0,), (16,), (16, 17), (15, 16, 17), (31,), (16, 17, 18, 19)]:                      # home bucket all tombstones, flag still set
        cs.append(Chain(f"tomb{_name(run)}", _spec(run, ip.TOMB_D1), limit=True))
    return cs


def long_chains() -> List[Chain]:
    """Chains of 40 keys: beyond the 32 keys of the pipelined gather the fast kernel's chunk loop takes over."""
    n = LONG_B
    cs = [Chain("plain", _spec(n=n)), Chain("none", [ip.ABSENT] * 4), Chain("m17", _spec(n=n, absent=17)),
            Chain("run{16,17}/d1", _spec([16, 17], n=n)), Chain("run{31,32}/d1", _spec([31, 32], n=n)), Chain("single{33}/d1", _spec([33], n=n)),
            Chain("run{35,36}/d2", _spec([35, 36], ip.D2, n=n)), Chain("run{16..19}/d1", _spec(range(16, 20), n=n)),
            Chain("run{32,33}/w", _spec([32, 33], ip.WRAP, n=n)), Chain("run{16,17,39}/w", _spec([16, 17, 39], ip.WRAP, n=n)),
            Chain("miss@36/ao", _spec([34, 35], n=n, absent=36, absent_how=ip.ABSENT_OVF)), Chain("miss@33/a", _spec([31, 32], n=n, absent=33)),
            Chain("twosets{31,32}/d1", _spec([31, 32], n=n), tail_from=16), Chain("tomb{32,33}", _spec([32, 33], ip.TOMB_D1, n=n))]
    for ch in cs[3:]:
        ch.limit = True
    return cs


@functools.lru_cache(maxsize=None)
def main_plan():
    cs = main_chains()
    return cs, ip.plan([c.spec for c in cs], SLOTS, SEED)


@functools.lru_cache(maxsize=None)
def long_plan():
    cs = long_chains()
    return cs, ip.plan([c.spec for c in cs], LONG_SLOTS, LONG_SEED)


def all_plans():
    """Every plan this module runs on (tests/test_index_placement_cpu.py verifies each without a GPU)."""
    return {"main": main_plan(), "long": long_plan()}


def layout(cs: List[Chain], nbs, max_b: int) -> List[Tuple[int, int, str]]:
    """(chain, n_blocks, label) per request row; row r is scored by wavefront r // 4 as its row r % 4."""
    rows = []
    short = [(PLAIN, 10, "short"), (NONE, 4, "short"), (PLAIN, 15, "short")]          # rows that stop below 16 hits

    def pad4():
        while len(rows) % 4:
            rows.append(short[len(rows) % 3])

    for c, ch in enumerate(cs):                             # mixed quadruples: every chain at every length, one after the other
        for nb in nbs:
            rows.append((c, min(nb, len(ch.spec)), f"{ch.name} nb={nb} mixed"))
    pad4()
    lim = [c for c, ch in enumerate(cs) if ch.limit]
    top = [nb for nb in nbs if nb >= 19] or [max_b]
    for c in lim:                                           # alone among three rows that stop short, at each g
        for nb in (top[0], top[-1]):
            for g in range(4):
                quad = list(short)
                quad.insert(g, (c, nb, f"{cs[c].name} nb={nb} alone@g{g}"))
                rows.extend(quad)
    for n, c in enumerate(lim):                             # next to a row with exactly 17 hits (which makes the wavefront fetch keys 17..31)
        quad = [(c, top[-1], f"{cs[c].name} nb={top[-1]} beside-m17"), (M17, top[-1], "m17"), short[0], short[1]]
        rows.extend(quad[n % 4:] + quad[:n % 4])
    return rows


@dataclass
class Case:
    B: int
    chains: List[Chain]
    plan: object
    pods: np.ndarray
    reqs: np.ndarray
    labels: List[str]
    inserts: List[Tuple[np.ndarray, np.ndarray]]
    has_tomb: bool
    first_limit_row: int                                    # rows from here on: the quadruples built around the limit chains
    listed: List[Tuple[int, ...]]                           # per row: the pods of its chain's group


def build_case(pkg, cs, pl, max_b, nbs, seed) -> Case:
    ip.verify(pl)                                           # never run on a plan that places nothing
    key_pods: Dict[int, Tuple[int, ...]] = {}
    for c, (ch, keys) in enumerate(zip(cs, pl.chains)):
        A = group_pods(c % N_GROUPS)
        for i, h in enumerate(keys.tolist()):
            if h not in pl.want:
                continue
            pods = A if i < ch.tail_from else (A[1],)
            if ch.odd.get(i) == "list":
                pods = group_pods((c + 1) % N_GROUPS)
            elif ch.odd.get(i) == "pod":
                pods = (3000 + c,)
            key_pods[h] = pods
    inserts = []
    for kind, keys in pl.calls:
        if kind in ("filler", "spill"):
            inserts.append((keys, np.full(keys.size, FILL_POD, dtype=np.uint32)))
        elif kind == "tomb":
            inserts.append((keys, np.full(keys.size, TOMB_POD, dtype=np.uint32)))
        else:                                               # a chain key's FIRST pair places it; the other pods of its set follow below
            inserts.append((keys, np.array([key_pods[h][0] for h in keys.tolist()], dtype=np.uint32)))
    rest = [(h, p_) for kind, keys in pl.calls if kind in ("chain", "wrap") for h in keys.tolist() for p_ in key_pods[h][1:]]
    inserts.append((np.array([h for h, _ in rest], dtype=np.uint64), np.array([p_ for _, p_ in rest], dtype=np.uint32)))
    rows = layout(cs, nbs, max_b)
    rng = np.random.default_rng(seed)
    R = len(rows)
    hashes = np.zeros((R, max_b), dtype=np.uint64)
    for r, (c, nb, _) in enumerate(rows):
        k = pl.chains[c]
        hashes[r, :k.size] = k                              # (the whole chain: what lies behind n_blocks must not be looked at)
    reqs = pkg.picker.make_req_rows(rng.integers(-1, 128, R), np.array([nb for _, nb, _ in rows]), hashes, max_b)
    first_limit = next(r for r, (_, _, lab) in enumerate(rows) if "alone@" in lab)
    assert first_limit % 4 == 0 and R % 4 == 0
    return Case(max_b, cs, pl, pkg.workload.make_pods(1617, P, 128), reqs, [f"[{r}] {lab}" for r, (_, _, lab) in enumerate(rows)], inserts,
                any(kind == "tomb" for kind, _ in pl.calls), first_limit, [group_pods(c % N_GROUPS) for c, _, _ in rows])


_CASES: Dict[str, Case] = {}


def case_of(pkg, which="main") -> Case:
    if which not in _CASES:
        if which == "main":
            cs, pl = main_plan()
            _CASES[which] = build_case(pkg, cs, pl, B, NBS, 1)
        else:
            cs, pl = long_plan()
            _CASES[which] = build_case(pkg, cs, pl, LONG_B, (33, 36, 40), 2)
    return _CASES[which]


def oracle_index(orc, case: Case):
    oix = orc.OracleIndex()
    for h, p_ in case.inserts:
        oix.insert(h, p_)
    if case.has_tomb:
        oix.remove_pod(TOMB_POD)
    return oix


_ORACLE: Dict[str, object] = {}


def shared_oracle(orc, case: Case, which="main"):
    """The oracle's index of a case, for the tests that do not change it."""
    if which not in _ORACLE:
        _ORACLE[which] = oracle_index(orc, case)
    return _ORACLE[which]


@contextlib.contextmanager
def picker(pkg, case: Case, chain=FUSED, max_batch=None):
    with pkg.BatchedPicker(chain, max_pods=P, max_blocks=case.B, max_batch=max_batch or case.reqs.shape[0], index_slots=case.plan.index_slots) as pk:
        pk.publish(case.pods)
        for h, p_ in case.inserts:
            pk.index_insert(h, p_)
        if case.has_tomb:
            pk.index_remove_pod(TOMB_POD)
        yield pk


def check_index(pk, oix):
    assert pk.index_selfcheck() == 0
    assert pk.launch_status() == 0
    assert pk.index_size() == oix.size()


def assert_rows(labels, got, want, what):
    """Picks equal, scores equal as uint64 -- the failing rows by name."""
    gp, gs = np.asarray(got[0]), np.asarray(got[1])
    wp, ws = np.asarray(want[0]), np.asarray(want[1])
    assert gp.shape == wp.shape and gs.shape == ws.shape, what
    bad = (gp != wp) | (gs.view(np.uint64) != ws.view(np.uint64))
    if bad.ndim > 1:
        bad = bad.any(axis=1)
    rows = np.nonzero(bad)[0]
    if rows.size:
        lines = [f"  {labels[r]}: gpu {gp[r]} {gs[r]!r} oracle {wp[r]} {ws[r]!r}" for r in rows[:60]]
        names = sorted({labels[r].split("] ", 1)[1].split(" nb=")[0] for r in rows})
        raise AssertionError(f"{what}: {rows.size} of {bad.size} rows differ from the oracle; chains: {names}\n" + "\n".join(lines))


@functools.lru_cache(maxsize=None)
def _masks(which, seed):
    return _build_masks(_CASES[which], seed)


def masks_of(case: Case, seed=5):
    return _masks("main" if case.B == B else "long", seed)


def _build_masks(case: Case, seed):
    """A 50 % mask on every row; and the same with every third row cut down to 3 candidates that miss the snapshot-wide QUEUE extremes (the
    request's own normalisers: the quad kernel parks such a row), half of them with a pod the chain is cached on among the three."""
    rng = np.random.default_rng(seed)
    R, W = case.reqs.shape[0], P // 64
    half = rng.integers(0, 1 << 63, (R, W), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, (R, W), dtype=np.uint64)
    q = case.pods["queue"]
    inner = np.nonzero((q != q.min()) & (q != q.max()))[0]
    few = half.copy()
    for r in range(0, R, 3):
        keep = [int(x) for x in rng.choice(inner, size=3, replace=False)]
        listed = [p_ for p_ in case.listed[r] if q[p_] != q.min() and q[p_] != q.max()]
        if (r // 3) % 2 == 0 and listed:
            keep[0] = listed[(r // 6) % len(listed)]
        few[r] = 0
        for p_ in keep:
            few[r, p_ // 64] |= np.uint64(1) << np.uint64(p_ % 64)
    return half, few


MODES = {
    "quadmin4": ({"EPPK_QUAD_MIN": "4"}, FUSED),           # the quad kernel for every batch
    "quad0": ({"EPPK_QUAD": "0"}, FUSED),                  # the fast kernel alone
    "lists0": ({"EPPK_LISTS": "0"}, FUSED),                # the dense route
    "generic": ({}, GENERIC),                              # the unfused kernel
    "default": ({}, FUSED),                                # as the library comes: the quad kernel from 4096 rows on
}
ROUTES = ["quadmin4", "quad0", "lists0", "generic"]


def set_mode(monkeypatch, mode):
    for k in ("EPPK_QUAD_MIN", "EPPK_QUAD", "EPPK_LISTS", "EPPK_RESIDENT"):
        monkeypatch.delenv(k, raising=False)
    env, chain = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return chain


@pytest.mark.parametrize("mode", ROUTES)
def test_single_picks(pkg, orc, monkeypatch, mode):
    """eppk_pick_batch without a mask, with a 50 % mask, and with subsets of 3 candidates that miss the queue extremes."""
    chain = set_mode(monkeypatch, mode)
    case = case_of(pkg)
    oix = shared_oracle(orc, case)
    half, few = masks_of(case)
    with picker(pkg, case, chain) as pk:
        assert pk.chain_is_fused() == (0 if mode == "generic" else 1)
        for what, mask in (("unmasked", None), ("mask 50 %", half), ("subsets of 3", few)):
            want = orc.pick_batch(chain, case.pods, oix, case.reqs, case.B, mask)[:2]
            assert_rows(case.labels, pk.pick(case.reqs, mask), want, f"{mode}, {what}")
        if mode == "quadmin4":
            assert pk.quad_stats()[0] >= 3, "the quad route was not taken"
        if mode == "quad0":
            assert pk.quad_stats() == (0, 0)
        check_index(pk, oix)


def test_headline_shape_batch_of_4096_rows_and_more(pkg, orc, monkeypatch):
    """The default mode, where only batches from 4096 rows on take the quad kernel: the rows twice, with other adapters."""
    set_mode(monkeypatch, "default")
    case = case_of(pkg)
    oix = shared_oracle(orc, case)
    again = case.reqs.copy()
    ad = np.random.default_rng(9).integers(-1, 128, again.shape[0]).astype(np.int32).view(np.uint32).astype(np.uint64)
    again[:, 0] = (again[:, 0] & np.uint64(0xFFFFFFFF00000000)) | ad
    reqs = np.concatenate([case.reqs, again])
    assert reqs.shape[0] >= 4096
    labels = case.labels + case.labels
    with picker(pkg, case, FUSED, max_batch=reqs.shape[0]) as pk:
        want = orc.pick_batch(FUSED, case.pods, oix, reqs, case.B)[:2]
        assert_rows(labels, pk.pick(reqs), want, "default mode, 2 x the rows")
        assert pk.quad_stats()[0] == 1, "a batch of 4096 rows and more takes the quad kernel"
        check_index(pk, oix)


@pytest.mark.parametrize("mode", ["quadmin4", "quad0"])
def test_fallback_lists_and_the_other_pickers(pkg, orc, monkeypatch, mode):
    """eppk_pick_topk (k = 4, plain and masked), random-top-k, eppk_pick_candidates."""
    chain = set_mode(monkeypatch, mode)
    case = case_of(pkg)
    oix = shared_oracle(orc, case)
    half, few = masks_of(case)
    with picker(pkg, case, chain) as pk:
        for what, mask in (("plain", None), ("mask 50 %", half), ("subsets of 3", few)):
            want = orc.pick_topk_batch(chain, case.pods, oix, case.reqs, case.B, 4, mask, threads=8)
            assert_rows(case.labels, pk.pick_topk(case.reqs, 4, mask), want, f"{mode}, top-4 {what}")
        for what, mask in (("plain", None), ("subsets of 3", few)):
            want = orc.pick_random_topk(chain, case.pods, oix, case.reqs, case.B, 3, 0xC0FFEE, mask)
            assert_rows(case.labels, pk.pick_random_topk(case.reqs, 3, 0xC0FFEE, mask), want, f"{mode}, random-top-3 {what}")
        for k in (1, 2):
            want = orc.pick_topk_batch(chain, case.pods, oix, case.reqs, case.B, k, few, threads=8)
            assert_rows(case.labels, pk.pick_candidates(case.reqs, few, k), want, f"{mode}, candidates k={k}")
        check_index(pk, oix)


@pytest.mark.parametrize("mode", ["quadmin4", "lists0", "generic"])
def test_weighted_random(pkg, orc, monkeypatch, mode):
    """pick_wrand_kernel has look-ups of its own: against tests/wrand_ref.py on the oracle's totals, over the quadruples built around the
    limit chains."""
    ref = _load("wrand_ref")
    chain = set_mode(monkeypatch, mode)
    case = case_of(pkg)
    oix = shared_oracle(orc, case)
    half, _ = masks_of(case)
    lo = case.first_limit_row
    reqs, labels = case.reqs[lo:], case.labels[lo:]
    n = reqs.shape[0]
    with picker(pkg, case, chain) as pk:
        for what, mask in (("plain", None), ("mask 50 %", half[lo:])):
            T = np.stack([orc.score_row(chain, case.pods, oix, reqs[r], None if mask is None else mask[r]) for r in range(n)])
            for k, seed in ((1, 0), (4, 0xDEADBEEFCAFEF00D)):
                want = ref.weighted_random(T, k, seed, np.arange(n))
                assert_rows(labels, pk.pick_weighted_random(reqs, seed, k, mask), want, f"{mode}, weighted-random {what} k={k}")
        check_index(pk, oix)


@pytest.mark.parametrize("mode", ["quadmin4", "quad0"])
def test_learn_then_pick_again(pkg, orc, monkeypatch, mode):
    """eppk_pick_learn_device: the picks are learnt into the table the plan filled (absent keys of the rows take free words -- tombstones
    among them -- or are displaced themselves), then the same batch again, twice."""
    import torch
    chain = set_mode(monkeypatch, mode)
    case = case_of(pkg)
    oix = oracle_index(orc, case)                           # (a private one: LEARN changes it)
    R = case.reqs.shape[0]
    with picker(pkg, case, chain) as pk:
        d_reqs = torch.from_numpy(case.reqs.view(np.int64)).cuda()
        d_pick = torch.empty(R, dtype=torch.int32, device="cuda")
        d_score = torch.empty(R, dtype=torch.float64, device="cuda")
        for gen in range(3):
            pk.pick_learn_device(d_reqs.data_ptr(), R, None, d_pick.data_ptr(), d_score.data_ptr())
            torch.cuda.synchronize()
            want = orc.pick_batch(chain, case.pods, oix, case.reqs, case.B)[:2]
            assert_rows(case.labels, (d_pick.cpu().numpy(), d_score.cpu().numpy()), want, f"{mode}, LEARN generation {gen}")
            oix.insert_picks(case.reqs, case.B, want[0])
            check_index(pk, oix)
        want = orc.pick_batch(chain, case.pods, oix, case.reqs, case.B)[:2]
        assert_rows(case.labels, pk.pick(case.reqs), want, f"{mode}, pick after LEARN")
        check_index(pk, oix)


@pytest.mark.timeout(120)
def test_resident_units(pkg, orc, monkeypatch):
    """EPPK_RESIDENT=1: batches of 8..64 rows are scored by the resident workgroups (pick_quad_body inside them): plain, masked, top-4."""
    set_mode(monkeypatch, "default")
    monkeypatch.setenv("EPPK_RESIDENT", "1")
    case = case_of(pkg)
    oix = shared_oracle(orc, case)
    half, few = masks_of(case)
    want = orc.pick_batch(FUSED, case.pods, oix, case.reqs, case.B)[:2]
    want_m = orc.pick_batch(FUSED, case.pods, oix, case.reqs, case.B, few)[:2]
    want_k = orc.pick_topk_batch(FUSED, case.pods, oix, case.reqs, case.B, 4, None, threads=8)
    R = case.reqs.shape[0]
    with picker(pkg, case, FUSED, max_batch=256) as pk:
        on, b0, _ = pk.resident_stats()
        assert on
        lo, n_calls, sizes, i = case.first_limit_row, 0, (8, 16, 32, 64, 12, 60, 24), 0
        while lo < R:
            hi = min(lo + sizes[i % len(sizes)], R)
            if hi - lo < 8:
                lo = hi - 8
            s = slice(lo, hi)
            lab = case.labels[s]
            assert_rows(lab, pk.pick(case.reqs[s]), (want[0][s], want[1][s]), f"resident, rows {lo}..{hi}")
            n_calls += 1
            if i % 3 == 0:
                assert_rows(lab, pk.pick(case.reqs[s], few[s]), (want_m[0][s], want_m[1][s]), f"resident masked, rows {lo}..{hi}")
                assert_rows(lab, pk.pick_topk(case.reqs[s], 4), (want_k[0][s], want_k[1][s]), f"resident top-4, rows {lo}..{hi}")
                n_calls += 2
            lo, i = hi, i + 1
        on, b1, starts = pk.resident_stats()
        assert b1 - b0 == n_calls and starts >= 1, (b1 - b0, n_calls, starts)
        check_index(pk, oix)


@pytest.mark.parametrize("mode", ROUTES)
def test_chains_of_40_blocks(pkg, orc, monkeypatch, mode):
    """More than 32 blocks per request (the shape of test_long_chains_beyond_the_pipelined_gather): displaced keys on both sides of the
    pipelined gather's 32 keys and behind it, where the synchronous chunk loop looks them up."""
    chain = set_mode(monkeypatch, mode)
    case = case_of(pkg, "long")
    oix = shared_oracle(orc, case, "long")
    with picker(pkg, case, chain) as pk:
        want = orc.pick_batch(chain, case.pods, oix, case.reqs, case.B)[:2]
        assert_rows(case.labels, pk.pick(case.reqs), want, f"{mode}, B = 40")
        half, few = masks_of(case)
        want = orc.pick_batch(chain, case.pods, oix, case.reqs, case.B, few)[:2]
        assert_rows(case.labels, pk.pick(case.reqs, few), want, f"{mode}, B = 40, subsets of 3")
        check_index(pk, oix)
