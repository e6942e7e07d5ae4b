"""The pick kernels' edge cases through MANY loop trips per wavefront, bit for bit against the oracle.

Every pick kernel is a persistent loop with state carried from one trip to the next: pick_quad_body's request rows two blocks ahead in
registers that swap roles, its ONE set of probe registers (gathered a block ahead, and written again by the refetch of keys 17..31), the
"listed" bits in LDS that are zeroed once in front of the loop, the deferred and parked counts that grow over the whole loop into lists of
defer_cap = 4 x trips entries; pick_fast_kernel's two rows in flight and its pod histogram that must stay zero between rows, the same
pipeline inside a work-list segment; the resident kernels' guards for a wavefront's second block.  A grid sized from the device's CUs gives
a wavefront ONE trip on every corpus of the suite but the benign full-size workload.  Here EPPK_MAX_CU / EPPK_MAX_WG_PER_CU (and, for
one-wavefront workgroups, EPPK_QUAD_THREADS / EPPK_FAST_THREADS) make the grid narrow -- tests/narrow_grid.py GEOMETRIES -- so that the
displaced-key corpus of tests/test_gpu_displaced.py, the value cases of tests/value_cases.py and blocks arranged as ordered neighbours run
with up to 147 (one wavefront: 1170) trips.  Every call asserts the geometry it relied on through launch_geometry(): a knob that is ignored
fails the test instead of letting it pass on one trip.

The corpora are those of tests/test_gpu_displaced.py and tests/value_cases.py, loaded by file name; tests/test_narrow_grid_cpu.py checks
the neighbour generator without a GPU.  EPPK_QUAD_PAUSE=0 throughout: a batch of four rows with two deferred would pause the quad route,
and the point is which kernel ran.
"""
import importlib.util
import os
import zlib
from typing import Dict, Sequence

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ng = _load("narrow_grid")
dp = _load("test_gpu_displaced")
vc = _load("value_cases")
FUSED, GENERIC, P = dp.FUSED, dp.GENERIC, dp.P

SWITCHES = ng.GEOMETRY_KNOBS + ("EPPK_QUAD_MIN", "EPPK_QUAD", "EPPK_LISTS", "EPPK_QUAD_TAIL", "EPPK_QUAD_PAUSE", "EPPK_RESIDENT", "EPPK_RESIDENT_MAX",
                                "EPPK_RESIDENT_QUAD_FROM")
# form -> (library mode of test_gpu_displaced.MODES, one-launch form of the quad route)
FORMS = {"quadmin4": ("quadmin4", True), "quadmin4-two-launches": ("quadmin4", False), "quad0": ("quad0", True), "lists0": ("lists0", True),
         "generic": ("generic", True), "default": ("default", True)}
ROUTES = ["quadmin4", "quadmin4-two-launches", "quad0", "lists0", "generic"]
QUAD_FORMS = ["quadmin4", "quadmin4-two-launches"]
# (the generic kernel has no thread knob: g1w1 would repeat g1w8 for it)
GEOMETRY_ROUTES = [(g, f) for g in ("g1w8", "g1w1") for f in ROUTES if not (g == "g1w1" and f == "generic")]
RES_WAVES = 16                                               # a resident workgroup: 1024 threads


def set_env(monkeypatch, geometry, form, **extra):
    """The module's own environment (read when a context is created); returns the chain of the form."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    env = dict(ng.GEOMETRIES[geometry][0]) if geometry else {}
    mode, tail = FORMS[form]
    env.update(dp.MODES[mode][0])
    if not tail:
        env["EPPK_QUAD_TAIL"] = "0"
    env["EPPK_QUAD_PAUSE"] = "0"
    env.update(extra)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return dp.MODES[mode][1]


class Watch:
    """Asserts the launch geometry behind every call of a picker created under (geometry, form), and keeps the largest trip count seen."""

    def __init__(self, pk, geometry, form, quad_exists=True, kernel=None):
        self.pk, self.geometry, self.form = pk, geometry, form
        self.cfg = ng.GEOMETRIES[geometry][1]
        self.quad = FORMS[form][0] == "quadmin4" and quad_exists
        self.tail = FORMS[form][1]
        self.kernel = kernel or ("generic" if form == "generic" else "fast")
        self.max_trips = 0

    def picks(self, n, what=""):
        """After a call that goes through launch_pick (pick, pick_topk, pick_random_topk, pick_learn_device)."""
        g = self.pk.launch_geometry()
        if self.quad and n >= 4:
            assert g[:2] == ng.expected_grid("quad", n, self.geometry), f"{what}: quad geometry {g} under {self.geometry}"
            if self.tail:
                assert g[2:] == (0, 0), f"{what}: the one-launch form launched a second kernel: {g}"
            else:
                assert g[3] == self.cfg["fast"] and 1 <= g[2] <= self.cfg["max_cu"], f"{what}: work-list pass {g} under {self.geometry}"
            t = ng.trips("quad", n, g[0], g[1])
        else:
            assert g == (0, 0) + ng.expected_grid(self.kernel, n, self.geometry), f"{what}: geometry {g} under {self.geometry}"
            t = ng.trips(self.kernel, n, g[2], g[3])
        self.max_trips = max(self.max_trips, t)
        return t

    def wrand(self, n, what=""):
        g = self.pk.launch_geometry()
        assert g == (0, 0, min(ng.ceil_div(n, 16), self.cfg["max_cu"]), 1024), f"{what}: weighted-random geometry {g} under {self.geometry}"
        return ng.ceil_div(n, g[2] * 16)

    def cands(self, n, what="", k=1):
        """After pick_candidates: the candidate-major kernel, four rows to a workgroup of 256 threads, eight workgroups per CU -- but where
        the quad route exists the library hands single picks from 8192 rows on, and fallback lists from 4096, to the general route."""
        if self.quad and n >= (8192 if k == 1 else 4096):
            return self.picks(n, what)
        g = self.pk.launch_geometry()
        assert g == (0, 0, min(ng.ceil_div(n, 4), 8 * self.cfg["max_cu"]), 256), f"{what}: candidates geometry {g} under {self.geometry}"
        return ng.ceil_div(n, g[2] * 4)


_WANT: Dict[tuple, object] = {}


def want(key, fn):
    """An oracle answer, computed once per module run and left unchanged."""
    if key not in _WANT:
        _WANT[key] = fn()
    return _WANT[key]


def chain_key(chain):
    return "generic" if chain is GENERIC else "fused"


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------

def _small_picker(pkg, chain, max_batch):
    wl = pkg.workload.make_workload(3, R=256, P=1000)
    pk = pkg.BatchedPicker(chain, max_pods=1024, max_blocks=wl.B, max_batch=max_batch, index_slots=wl.index_slots)
    pk.publish(wl.pods)
    pk.index_insert(wl.index_hashes, wl.index_pods)
    return pk, wl


def _rows(wl, n):
    return wl.reqs[np.arange(n) % wl.reqs.shape[0]]


@pytest.mark.parametrize("geometry", list(ng.GEOMETRIES))
def test_each_geometry_reports_what_the_table_says(pkg, monkeypatch, geometry):
    """quad / fast / generic kernel, the weighted-random and the candidates kernel: workgroups and threads per workgroup under each
    geometry; a kernel that was not launched reports 0."""
    cfg = ng.GEOMETRIES[geometry][1]
    n = 640
    for form in ("quadmin4", "quadmin4-two-launches", "quad0", "generic"):
        chain = set_env(monkeypatch, geometry, form)
        pk, wl = _small_picker(pkg, chain, n)
        with pk:
            assert pk.launch_geometry() == (0, 0, 0, 0), "nothing launched yet"
            pk.pick(_rows(wl, n))
            g = pk.launch_geometry()
            if form == "quadmin4":
                assert g == (cfg["max_cu"], cfg["quad"], 0, 0), (geometry, form, g)
            elif form == "quadmin4-two-launches":
                assert g[:2] == (cfg["max_cu"], cfg["quad"]) and g[3] == cfg["fast"] and 1 <= g[2] <= cfg["max_cu"], (geometry, form, g)
            else:
                assert g == (0, 0, cfg["max_cu"], cfg["fast" if form == "quad0" else "generic"]), (geometry, form, g)
            pk.pick_weighted_random(_rows(wl, n), 7, 2)
            assert pk.launch_geometry() == (0, 0, cfg["max_cu"], 1024), (geometry, form)
            mask = np.zeros((n, 16), dtype=np.uint64)
            mask[:, :15] = np.uint64(0x0101010101010101)
            pk.pick_candidates(_rows(wl, n), mask, 2)
            assert pk.launch_geometry() == (0, 0, 8 * cfg["max_cu"], 256), (geometry, form)
            pk.pick(_rows(wl, 2))
            assert pk.launch_geometry()[:2] == (0, 0), "a batch below EPPK_QUAD_MIN does not take the quad kernel"
            assert pk.launch_status() == 0


def test_a_640_row_batch_under_g1w8_reports_20_trips(pkg, monkeypatch):
    set_env(monkeypatch, "g1w8", "quadmin4")
    pk, wl = _small_picker(pkg, FUSED, 640)
    with pk:
        pk.pick(_rows(wl, 640))
        g = pk.launch_geometry()
        assert g == (1, 512, 0, 0)
        assert ng.trips("quad", 640, g[0], g[1]) == 20
        assert pk.quad_stats()[0] == 1


def test_without_a_knob_the_grid_is_what_it_was(pkg, monkeypatch):
    """No EPPK_MAX_CU: below the device's capacity the grid is one workgroup per wavefront-load of blocks; at capacity it is a whole
    number of workgroups per CU -- exactly one with EPPK_MAX_WG_PER_CU=1 --, and an EPPK_MAX_CU beyond the device changes nothing."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus >= 147
    n_big = 65536
    seen = {}
    for tag, extra in (("none", {}), ("huge", {"EPPK_MAX_CU": "100000"}), ("one-per-cu", {"EPPK_MAX_WG_PER_CU": "1"})):
        for form in ("quadmin4", "quad0"):
            set_env(monkeypatch, None, form, **extra)
            pk, wl = _small_picker(pkg, FUSED, n_big)
            with pk:
                if form == "quadmin4":                     # 4680 rows: 1170 blocks, eight to a workgroup
                    pk.pick(_rows(wl, 4680))
                    assert pk.launch_geometry() == (147, 512, 0, 0), (tag, pk.launch_geometry())
                else:                                      # 2048 rows: sixteen to a workgroup
                    pk.pick(_rows(wl, 2048))
                    assert pk.launch_geometry() == (0, 0, 128, 1024), (tag, pk.launch_geometry())
                pk.pick(_rows(wl, n_big))
                g = pk.launch_geometry()
                grid = g[0] if form == "quadmin4" else g[2]
                assert grid >= cus and grid % cus == 0, (tag, form, g, cus)
                if tag == "one-per-cu":
                    assert grid == cus, (tag, form, g, cus)
                seen[(tag, form)] = g
    for form in ("quadmin4", "quad0"):
        assert seen[("none", form)] == seen[("huge", form)], seen


# ---- blocks of chosen kinds over the displaced corpus's table -------------------------------------------------------------------------------

SHORT = [("plain", 10), ("none", 4), ("plain", 15), ("plain", 12)]
PRINCIPAL = {"short": ("plain", 13), "none": ("none", 4), "m17": ("m17", 32), "home32": ("plain", 32), "d16_17": ("run{16,17}/d1", 32),
             "d16_31": ("run{16..31}/d1", 32), "miss_ovf": ("miss@17/ao", 32), "twosets": ("twosets{16,17}/d1", 32), "tomb": ("tomb{16,17}", 32),
             "reserved": ("plain", 20), "parked": ("plain", 20), "nocand": ("run{16,17}/d1", 32)}


class Batch:
    """Request rows built block by block from kinds (narrow_grid.KINDS) over the MAIN case of tests/test_gpu_displaced.py: the kind's
    principal row at position block % 4 among three short rows (rows_per_block = 4), or alone (rows_per_block = 1)."""

    def __init__(self, pkg, case, kinds: Sequence[str], rows_per_block: int, nwaves: int, seed: int):
        at = {ch.name: i for i, ch in enumerate(case.chains)}
        rng = np.random.default_rng(seed)
        rows, self.kind_of_row, self.labels = [], [], []
        for blk, kind in enumerate(kinds):
            quad = [PRINCIPAL[kind] + (kind,)]
            if rows_per_block == 4:
                quad = [s_ + ("short",) for s_ in SHORT[:3]]
                quad.insert(blk % 4, PRINCIPAL[kind] + (kind,))
            for name, nb, row_kind in quad:
                self.kind_of_row.append(row_kind)
                self.labels.append(f"[{len(rows)}] {row_kind} nb={nb} block {blk} wavefront {blk % nwaves} trip {blk // nwaves}")
                rows.append((at[name], nb))
        R = len(rows)
        hashes = np.zeros((R, case.B), dtype=np.uint64)
        for r, (c, _) in enumerate(rows):
            k = case.plan.chains[c]
            hashes[r, :k.size] = k
        for n, r in enumerate(r for r in range(R) if self.kind_of_row[r] == "reserved"):     # 0 and ~0, at positions on both sides of key 16
            hashes[r, (3, 16, 19, 0)[n % 4]] = np.uint64(0) if n % 2 else np.uint64(0xFFFFFFFFFFFFFFFF)
        self.reqs = pkg.picker.make_req_rows(rng.integers(-1, 128, R), np.array([nb for _, nb in rows]), hashes, case.B)
        self.listed = [dp.group_pods(c % dp.N_GROUPS) for c, _ in rows]
        self.R = R
        # masks: 50 % on every row; three candidates that miss the snapshot-wide QUEUE extremes (the quad kernel parks such a row)
        W = P // 64
        self.half = rng.integers(0, 1 << 63, (R, W), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, (R, W), dtype=np.uint64)
        q = case.pods["queue"]
        inner = np.nonzero((q != q.min()) & (q != q.max()))[0]
        self.few = np.zeros((R, W), dtype=np.uint64)
        for r in range(R):
            keep = [int(x) for x in rng.choice(inner, size=3, replace=False)]
            listed = [p_ for p_ in self.listed[r] if q[p_] != q.min() and q[p_] != q.max()]
            if r % 2 == 0 and listed:
                keep[0] = listed[(r // 2) % len(listed)]
            for p_ in keep:
                self.few[r, p_ // 64] |= np.uint64(1) << np.uint64(p_ % 64)
        # by kind: 50 %, but a "parked" row its three candidates and a "nocand" row none
        self.by_kind = self.half.copy()
        for r, kind in enumerate(self.kind_of_row):
            if kind == "parked":
                self.by_kind[r] = self.few[r]
            elif kind == "nocand":
                self.by_kind[r] = 0


_BATCHES: Dict[tuple, Batch] = {}


def batch_of(pkg, key, kinds_fn, rows_per_block, nwaves) -> Batch:
    k = (key, rows_per_block, nwaves)
    if k not in _BATCHES:
        _BATCHES[k] = Batch(pkg, dp.case_of(pkg), kinds_fn(), rows_per_block, nwaves, zlib.crc32(repr(k).encode()))
    return _BATCHES[k]


def form_geometry(geometry, form):
    """(kernel whose loop the form's batches run through, its rows per block, its wavefronts under the geometry at full width)."""
    kernel = "quad" if form in QUAD_FORMS else "generic" if form == "generic" else "fast"
    cfg = ng.GEOMETRIES[geometry][1]
    return kernel, ng.ROWS_PER_BLOCK[kernel], cfg["max_cu"] * cfg[kernel] // 64


# ---- every batch length -------------------------------------------------------------------------------------------------------------------

LENGTHS = {"g1w8": list(range(1, 133)), "g3w8": [1, 3, 4, 5, 31, 32, 33, 64, 65, 93, 95, 96, 97, 99, 100, 101, 127, 128, 129, 130, 131, 132]}


def _mixed_33_blocks():
    return [ng.KINDS[(5 * i) % len(ng.KINDS)] for i in range(33)]


@pytest.mark.parametrize("form", ROUTES)
@pytest.mark.parametrize("geometry", ["g1w8", "g3w8"])
def test_every_batch_length(pkg, orc, monkeypatch, geometry, form):
    """One batch of 132 rows (33 blocks of every kind), cut to R = 1..132 (g3w8: a coarser set): unmasked, 50 % mask, subsets of 3 that miss
    the QUEUE extremes, top-3 (plain and subsets), the candidates form, weighted-random.  Every `break` of the loops that are unrolled
    twice: odd and even trip counts, a partial last block, a last trip in which only some wavefronts have a block, idle wavefronts.
    Under g1w8 the quad kernel makes 1..5 trips (32 rows each), the fast kernel 1..9 (16 rows), the generic kernel 1..17 (8 rows)."""
    ref = _load("wrand_ref")
    chain = set_env(monkeypatch, geometry, form)
    case = dp.case_of(pkg)
    oix = dp.shared_oracle(orc, case)
    b = batch_of(pkg, "lengths", _mixed_33_blocks, 4, 8)
    ck = chain_key(chain)
    w_plain = want(("len", ck, "plain"), lambda: orc.pick_batch(chain, case.pods, oix, b.reqs, case.B)[:2])
    w_half = want(("len", ck, "half"), lambda: orc.pick_batch(chain, case.pods, oix, b.reqs, case.B, b.half)[:2])
    w_few = want(("len", ck, "few"), lambda: orc.pick_batch(chain, case.pods, oix, b.reqs, case.B, b.few)[:2])
    w_top = want(("len", ck, "top3"), lambda: orc.pick_topk_batch(chain, case.pods, oix, b.reqs, case.B, 3, None, threads=8))
    w_topf = want(("len", ck, "top3 few"), lambda: orc.pick_topk_batch(chain, case.pods, oix, b.reqs, case.B, 3, b.few, threads=8))
    w_c2 = want(("len", ck, "cands 2"), lambda: orc.pick_topk_batch(chain, case.pods, oix, b.reqs, case.B, 2, b.few, threads=8))
    T = want(("len", ck, "T"), lambda: np.stack([orc.score_row(chain, case.pods, oix, b.reqs[r], b.half[r]) for r in range(b.R)]))
    w_wr = want(("len", ck, "wrand"), lambda: ref.weighted_random(T, 3, 0xDEADBEEFCAFEF00D, np.arange(b.R)))
    kernel = form_geometry(geometry, form)[0]
    seen_trips = set()
    with dp.picker(pkg, case, chain, max_batch=b.R) as pk:
        watch = Watch(pk, geometry, form)
        for R in LENGTHS[geometry]:
            reqs, lab, what = b.reqs[:R], b.labels[:R], f"{form} {geometry} R={R}"
            cut = lambda w: (w[0][:R], w[1][:R])
            dp.assert_rows(lab, pk.pick(reqs), cut(w_plain), what + " unmasked")
            seen_trips.add(watch.picks(R, what))
            dp.assert_rows(lab, pk.pick(reqs, b.half[:R]), cut(w_half), what + " mask 50 %")
            watch.picks(R, what)
            dp.assert_rows(lab, pk.pick(reqs, b.few[:R]), cut(w_few), what + " subsets of 3")
            watch.picks(R, what)
            dp.assert_rows(lab, pk.pick_topk(reqs, 3), cut(w_top), what + " top-3")
            watch.picks(R, what)
            dp.assert_rows(lab, pk.pick_topk(reqs, 3, b.few[:R]), cut(w_topf), what + " top-3, subsets of 3")
            watch.picks(R, what)
            dp.assert_rows(lab, pk.pick_candidates(reqs, b.few[:R], 2), cut(w_c2), what + " candidates k=2")
            watch.cands(R, what, 2)
            dp.assert_rows(lab, pk.pick_weighted_random(reqs, 0xDEADBEEFCAFEF00D, 3, b.half[:R]), cut(w_wr), what + " weighted-random k=3")
            watch.wrand(R, what)
        dp.check_index(pk, oix)
        if form in QUAD_FORMS:
            assert pk.quad_stats()[0] == 5 * sum(1 for R in LENGTHS[geometry] if R >= 4), "the quad route was not taken"
    per_trip = {"quad": 32, "fast": 16, "generic": 8}[kernel] * ng.GEOMETRIES[geometry][1]["max_cu"]
    assert seen_trips == set(range(1, ng.ceil_div(132, per_trip) + 1)), (seen_trips, per_trip)


# ---- the displaced corpus, main and long ------------------------------------------------------------------------------------------------------

def _corpus(pkg, orc, which):
    case = dp.case_of(pkg, which)
    return case, dp.shared_oracle(orc, case, which), dp.masks_of(case)


def _corpus_trips(case, geometry, form):
    kernel, rpb, nwaves = form_geometry(geometry, form)
    return ng.ceil_div(ng.ceil_div(case.reqs.shape[0], rpb), nwaves)


@pytest.mark.parametrize("geometry,form", GEOMETRY_ROUTES)
@pytest.mark.parametrize("which", ["main", "long"])
def test_displaced_corpus_single_picks(pkg, orc, monkeypatch, which, geometry, form):
    """The rows of tests/test_gpu_displaced.py (main: 4680 rows of 32 blocks; long: chains of 40) through eppk_pick_batch without a mask,
    with a 50 % mask and with subsets of 3: under g1w8 a quad wavefront makes 147 trips over the main corpus, under g1w1 ONE wavefront walks
    the whole batch (1170 blocks; the fast kernel 4680 rows)."""
    chain = set_env(monkeypatch, geometry, form)
    case, oix, (half, few) = _corpus(pkg, orc, which)
    R, ck = case.reqs.shape[0], chain_key(chain)
    with dp.picker(pkg, case, chain) as pk:
        watch = Watch(pk, geometry, form)
        for what, mask in (("unmasked", None), ("mask 50 %", half), ("subsets of 3", few)):
            w = want((which, ck, "pick", what), lambda: orc.pick_batch(chain, case.pods, oix, case.reqs, case.B, mask)[:2])
            dp.assert_rows(case.labels, pk.pick(case.reqs, mask), w, f"{form} {geometry} {which}, {what}")
            assert watch.picks(R, what) == _corpus_trips(case, geometry, form)
        if form in QUAD_FORMS:
            assert pk.quad_stats()[0] == 3, "the quad route was not taken"
        dp.check_index(pk, oix)
    if which == "main" and geometry == "g1w8" and form in QUAD_FORMS:
        assert watch.max_trips == 147


@pytest.mark.parametrize("form", QUAD_FORMS + ["quad0"])
@pytest.mark.parametrize("geometry", ["g1w8", "g1w1"])
def test_displaced_corpus_fallback_lists_and_the_other_pickers(pkg, orc, monkeypatch, geometry, form):
    """eppk_pick_topk (k = 4; plain, 50 % mask, subsets of 3), random-top-3, the candidates form."""
    chain = set_env(monkeypatch, geometry, form)
    case, oix, (half, few) = _corpus(pkg, orc, "main")
    R = case.reqs.shape[0]
    with dp.picker(pkg, case, chain) as pk:
        watch = Watch(pk, geometry, form)
        for what, mask in (("plain", None), ("mask 50 %", half), ("subsets of 3", few)):
            w = want(("main", "fused", "top4", what), lambda: orc.pick_topk_batch(chain, case.pods, oix, case.reqs, case.B, 4, mask, threads=8))
            dp.assert_rows(case.labels, pk.pick_topk(case.reqs, 4, mask), w, f"{form} {geometry}, top-4 {what}")
            assert watch.picks(R, what) == _corpus_trips(case, geometry, form)
        for what, mask in (("plain", None), ("subsets of 3", few)):
            w = want(("main", "fused", "random3", what), lambda: orc.pick_random_topk(chain, case.pods, oix, case.reqs, case.B, 3, 0xC0FFEE, mask))
            dp.assert_rows(case.labels, pk.pick_random_topk(case.reqs, 3, 0xC0FFEE, mask), w, f"{form} {geometry}, random-top-3 {what}")
            assert watch.picks(R, what) == _corpus_trips(case, geometry, form)
        for k in (1, 2):
            w = want(("main", "fused", "cands", k), lambda: orc.pick_topk_batch(chain, case.pods, oix, case.reqs, case.B, k, few, threads=8))
            dp.assert_rows(case.labels, pk.pick_candidates(case.reqs, few, k), w, f"{form} {geometry}, candidates k={k}")
            assert watch.cands(R, f"candidates k={k}", k) == (_corpus_trips(case, geometry, form) if form in QUAD_FORMS and k > 1 else ng.ceil_div(R, 32))
        dp.check_index(pk, oix)


@pytest.mark.parametrize("form", ["quadmin4", "lists0", "generic"])
@pytest.mark.parametrize("geometry", ["g1w8", "g1w1"])
def test_displaced_corpus_weighted_random(pkg, orc, monkeypatch, geometry, form):
    """pick_wrand_kernel (one workgroup of 16 wavefronts under either geometry: it has no thread knob) over the quadruples built around
    the limit chains, against tests/wrand_ref.py on the oracle's totals."""
    ref = _load("wrand_ref")
    chain = set_env(monkeypatch, geometry, form)
    case, oix, (half, _) = _corpus(pkg, orc, "main")
    lo, ck = case.first_limit_row, chain_key(chain)
    reqs, labels = case.reqs[lo:], case.labels[lo:]
    n = reqs.shape[0]
    with dp.picker(pkg, case, chain) as pk:
        watch = Watch(pk, geometry, form)
        for what, mask in (("plain", None), ("mask 50 %", half[lo:])):
            T = want(("main", ck, "T", what), lambda: np.stack([orc.score_row(chain, case.pods, oix, reqs[r], None if mask is None else mask[r]) for r in range(n)]))
            for k, seed in ((1, 0), (4, 0xDEADBEEFCAFEF00D)):
                w = want(("main", ck, "wrand", what, k), lambda: ref.weighted_random(T, k, seed, np.arange(n)))
                dp.assert_rows(labels, pk.pick_weighted_random(reqs, seed, k, mask), w, f"{form} {geometry}, weighted-random {what} k={k}")
                assert watch.wrand(n) == ng.ceil_div(n, 16)
        dp.check_index(pk, oix)


@pytest.mark.parametrize("form", QUAD_FORMS + ["quad0"])
@pytest.mark.parametrize("geometry", ["g1w8", "g1w1"])
def test_displaced_corpus_learn_then_pick_again(pkg, orc, monkeypatch, geometry, form):
    """eppk_pick_learn_device twice (the learn words come out of the quad loop), then the same batch through eppk_pick_batch."""
    import torch
    chain = set_env(monkeypatch, geometry, form)
    case = dp.case_of(pkg)
    oix = dp.oracle_index(orc, case)                         # (a private one: LEARN changes it)
    R = case.reqs.shape[0]
    with dp.picker(pkg, case, chain) as pk:
        watch = Watch(pk, geometry, form)
        d_reqs = torch.from_numpy(case.reqs.view(np.int64)).cuda()
        d_pick = torch.empty(R, dtype=torch.int32, device="cuda")
        d_score = torch.empty(R, dtype=torch.float64, device="cuda")
        for gen in range(2):
            pk.pick_learn_device(d_reqs.data_ptr(), R, None, d_pick.data_ptr(), d_score.data_ptr())
            assert watch.picks(R, "LEARN") == _corpus_trips(case, geometry, form)
            torch.cuda.synchronize()
            w = orc.pick_batch(chain, case.pods, oix, case.reqs, case.B)[:2]
            dp.assert_rows(case.labels, (d_pick.cpu().numpy(), d_score.cpu().numpy()), w, f"{form} {geometry}, LEARN generation {gen}")
            oix.insert_picks(case.reqs, case.B, w[0])
            dp.check_index(pk, oix)
        w = orc.pick_batch(chain, case.pods, oix, case.reqs, case.B)[:2]
        dp.assert_rows(case.labels, pk.pick(case.reqs), w, f"{form} {geometry}, pick after LEARN")
        assert watch.picks(R, "pick after LEARN") == _corpus_trips(case, geometry, form)
        dp.check_index(pk, oix)


# ---- ordered neighbours -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geometry,form", GEOMETRY_ROUTES)
def test_ordered_neighbours(pkg, orc, monkeypatch, geometry, form):
    """Every ordered pair of the twelve block kinds (narrow_grid.KINDS) in one wavefront on consecutive trips, at an even and at an odd
    trip, and a few triples -- laid out for the wavefront count of the kernel that runs (tests/test_narrow_grid_cpu.py checks the layout).
    A block that refetches into the probe registers, parks or defers must leave nothing behind for the next block, nor inherit anything
    from the one before.  Unmasked, masked by kind (50 %; a parked row three candidates; an empty row none), top-4 both ways."""
    chain = set_env(monkeypatch, geometry, form)
    kernel, rpb, nwaves = form_geometry(geometry, form)
    case = dp.case_of(pkg)
    oix = dp.shared_oracle(orc, case)
    b = batch_of(pkg, "neighbours", lambda: ng.neighbour_schedule(nwaves).kinds, rpb, nwaves)
    sched = ng.neighbour_schedule(nwaves)
    assert b.R == len(sched.kinds) * rpb <= 4680
    ck = (chain_key(chain), rpb, nwaves)
    with dp.picker(pkg, case, chain, max_batch=b.R) as pk:
        watch = Watch(pk, geometry, form)
        for what, mask in (("unmasked", None), ("masked by kind", b.by_kind)):
            w = want(("nb", ck, "pick", what), lambda: orc.pick_batch(chain, case.pods, oix, b.reqs, case.B, mask)[:2])
            dp.assert_rows(b.labels, pk.pick(b.reqs, mask), w, f"{form} {geometry} neighbours, {what}")
            assert watch.picks(b.R, what) == sched.n_trips
            g = pk.launch_geometry()
            assert (g[0] * g[1] if kernel == "quad" else g[2] * g[3]) // 64 == nwaves, "the batch was laid out for another wavefront count"
            w = want(("nb", ck, "top4", what), lambda: orc.pick_topk_batch(chain, case.pods, oix, b.reqs, case.B, 4, mask, threads=8))
            dp.assert_rows(b.labels, pk.pick_topk(b.reqs, 4, mask), w, f"{form} {geometry} neighbours, top-4 {what}")
            assert watch.picks(b.R, what) == sched.n_trips
        if form in QUAD_FORMS:
            launches, deferred = pk.quad_stats()
            assert launches == 4, "the quad route was not taken"
            assert deferred >= 4 * b.kind_of_row.count("reserved"), "a row with a reserved hash is deferred"
        dp.check_index(pk, oix)


# ---- full work-list segments, full park lists -----------------------------------------------------------------------------------------------

BENIGN = ("short", "m17", "home32", "d16_17", "d16_31", "miss_ovf", "twosets", "tomb")     # rows the quad kernel scores itself
RSV_H = np.array([0, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
RSV_P = np.array([dp.group_pods(0)[0], 3000], dtype=np.uint32)


def _density_rows(R, density):
    if density == "all":
        return np.arange(R)
    if density == "alternating":
        return np.arange(0, R, 2)
    return np.array([4 * (w + 8 * ((3 * w + 1) % 20)) + w % 4 for w in range(8)])          # one row of each wavefront, on trips of its own


@pytest.mark.parametrize("density", ["one", "alternating", "all"])
@pytest.mark.parametrize("form", QUAD_FORMS)
def test_full_work_list_segments_and_park_lists(pkg, orc, monkeypatch, form, density):
    """640 rows under g1w8: 8 wavefronts x 20 trips, so a wavefront's work-list segment and its park list hold exactly defer_cap = 80
    entries.  A reserved hash (0 / ~0, both in the index) defers a row: one row per wavefront, every other row, every row -- then the
    segment is full to its last entry and the work-list pass (one-launch form: the workgroup's own; two-launch form: pick_fast_kernel's
    work-list instantiation, 80 rows through its two-row pipeline per segment) scores all of them.  Single picks, top-4, masked.  The same
    with rows PARKED (subsets of 3 that miss the QUEUE extremes) at the same densities, and with parked, deferred and plain rows mixed in
    every wavefront."""
    chain = set_env(monkeypatch, "g1w8", form)
    case = dp.case_of(pkg)
    b = batch_of(pkg, "benign", lambda: [BENIGN[(3 * i) % len(BENIGN)] for i in range(160)], 4, 8)
    R = b.R
    assert R == 640
    oix = want(("rsv", "oix"), lambda: _rsv_oracle(orc, case))
    sel = _density_rows(R, density)
    rsv_all = b.reqs.copy()                                  # a reserved hash in every row, on both sides of key 16
    nb = (rsv_all[:, 0] >> np.uint64(32)).astype(np.int64)
    rsv_all[np.arange(R), 1 + np.arange(R) % np.minimum(nb, 20)] = RSV_H[(np.arange(R) // 3) % 2]
    reqs = b.reqs.copy()
    reqs[sel] = rsv_all[sel]
    chosen = set(sel.tolist())
    lab = [l + (" +reserved hash" if r in chosen else "") for r, l in enumerate(b.labels)]
    parked = b.half.copy()
    parked[sel] = b.few[sel]
    mixed = b.half.copy()                                    # row 3i parked, row 3i + 1 deferred, row 3i + 2 plain: all three in every wavefront
    mixed[0::3] = b.few[0::3]
    mixed_reqs = b.reqs.copy()
    mixed_reqs[1::3] = rsv_all[1::3]
    with dp.picker(pkg, case, chain, max_batch=R) as pk:
        pk.index_insert(RSV_H, RSV_P)
        watch = Watch(pk, "g1w8", form)
        d0 = pk.quad_stats()[1]
        for what, rq, mask, k in (("deferred", reqs, None, 1), ("deferred top-4", reqs, None, 4), ("deferred, mask 50 %", reqs, b.half, 1),
                                  ("deferred top-4, mask 50 %", reqs, b.half, 4), ("parked", b.reqs, parked, 1), ("parked top-4", b.reqs, parked, 4),
                                  ("parked and deferred", reqs, parked, 1), ("parked, deferred and plain mixed", mixed_reqs, mixed, 1),
                                  ("parked, deferred and plain mixed, top-4", mixed_reqs, mixed, 4)):
            if k == 1:
                w = orc.pick_batch(chain, case.pods, oix, rq, case.B, mask)[:2]
                got = pk.pick(rq, mask)
            else:
                w = orc.pick_topk_batch(chain, case.pods, oix, rq, case.B, k, mask, threads=8)
                got = pk.pick_topk(rq, k, mask)
            dp.assert_rows(lab, got, w, f"{form} {density}: {what}")
            assert watch.picks(R, what) == 20
            d1 = pk.quad_stats()[1]
            if what.startswith("deferred"):
                assert d1 - d0 >= sel.size, f"{what}: {d1 - d0} rows deferred, {sel.size} carry a reserved hash"
                if density == "all":
                    assert d1 - d0 == R, f"{what}: {d1 - d0} of {R} rows deferred"
            d0 = d1
        assert pk.quad_stats()[0] == 9, "the quad route was not taken"
        dp.check_index(pk, oix)


def _rsv_oracle(orc, case):
    oix = dp.oracle_index(orc, case)
    oix.insert(RSV_H, RSV_P)
    return oix


# ---- the value cases ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [vc.SEED0 + i for i in range(vc.N_SEEDS)])
def test_value_cases_over_several_trips(pkg, orc, monkeypatch, seed):
    """The 104 cases of tests/value_cases.py (queue over all of u32, kv_util NaN / inf / subnormal, extreme weights) through pick and
    pick_topk under g1w8, with the quad route for every batch and without it: R <= 200 rows are up to 7 trips through the quad kernel,
    13 through the fast kernel, 25 through the generic one."""
    c = vc.make_case(seed)
    oix = orc.OracleIndex()
    if c["B"] and c["ih"].size:
        oix.insert(c["ih"], c["ip"], snapshot=c["pods"])
    w = orc.pick_batch(c["chain"], c["pods"], oix, c["reqs"], c["B"], c["mask"])[:2]
    w_k = orc.pick_topk(c["chain"], c["pods"], oix, c["reqs"], c["k"], c["mask"])
    for form in ("quadmin4", "quad0"):
        set_env(monkeypatch, "g1w8", form)
        what = f"{form} g1w8 {vc.info(c)}"
        with pkg.BatchedPicker(c["chain"], max_pods=c["P"], max_blocks=c["B"], max_batch=c["R"], index_slots=c["slots"] if c["B"] else 0) as pk:
            pk.publish(c["pods"])
            if c["B"] and c["ih"].size:
                pk.index_insert(c["ih"], c["ip"])
            assert pk.chain_is_fused() == c["kind"], what
            watch = Watch(pk, "g1w8", form, quad_exists=vc.quad_route_exists(c), kernel="fast" if c["kind"] else "generic")
            got = pk.pick(c["reqs"], c["mask"])
            t = watch.picks(c["R"], what)
            got_k = pk.pick_topk(c["reqs"], c["k"], c["mask"])
            assert watch.picks(c["R"], what) == t
            assert t == ng.ceil_div(c["R"], 32 if watch.quad and c["R"] >= 4 else 16 if c["kind"] else 8), what
            if watch.quad:
                assert pk.quad_stats()[0] == 2, what + ": the quad route was not taken"
            assert pk.launch_status() == 0, what
        for g_, w_, tag in ((got, w, ""), (got_k, w_k, f" topk {c['k']}")):
            gp, gs, wp, ws = np.asarray(g_[0]), np.asarray(g_[1]), np.asarray(w_[0]), np.asarray(w_[1])
            assert gp.shape == wp.shape, what + tag
            bad = np.nonzero(((gp != wp) | (gs.view(np.uint64) != ws.view(np.uint64))).reshape(gp.shape[0], -1).any(axis=1))[0]
            assert bad.size == 0, f"{what}{tag}: {bad.size} rows differ from the oracle, first {bad[:5]}: gpu {gp[bad[:3]]} {gs[bad[:3]]!r} oracle {wp[bad[:3]]} {ws[bad[:3]]!r}"


# ---- resident units beyond one block per wavefront --------------------------------------------------------------------------------------------

RES_N = [65, 96, 128, 129, 192, 255]


def _res_rows(case, n):
    lo = case.first_limit_row + 4 * ((7 * n) % 500)
    return slice(lo, lo + n)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("n", RES_N)
def test_resident_units_with_more_than_one_block_per_wavefront(pkg, orc, monkeypatch, n):
    """EPPK_RESIDENT=1 with EPPK_RESIDENT_MAX=255: batches of 65..255 rows of the displaced corpus are 17..64 blocks for the 16 wavefronts
    of a resident workgroup -- up to four trips of pick_quad_body<RESIDENT>, whose look-ahead is guarded by `blk + nwaves < nblk`.  The
    plain, masked and top-4 units, one doorbell each; nothing is launched."""
    set_env(monkeypatch, None, "default", EPPK_RESIDENT="1", EPPK_RESIDENT_MAX="255")
    case, oix, (half, few) = _corpus(pkg, orc, "main")
    s = _res_rows(case, n)
    reqs, lab = case.reqs[s], case.labels[s]
    trips = ng.ceil_div(ng.ceil_div(n, 4), RES_WAVES)
    assert trips == {65: 2, 96: 2, 128: 2, 129: 3, 192: 3, 255: 4}[n]
    with dp.picker(pkg, case, FUSED, max_batch=1024) as pk:     # (room for the n x 4 lists in the pinned result buffers: else top-4 is launched)
        on, b0, _ = pk.resident_stats()
        assert on
        dp.assert_rows(lab, pk.pick(reqs), orc.pick_batch(FUSED, case.pods, oix, reqs, case.B)[:2], f"resident n={n}")
        dp.assert_rows(lab, pk.pick(reqs, few[s]), orc.pick_batch(FUSED, case.pods, oix, reqs, case.B, few[s])[:2], f"resident masked n={n}")
        dp.assert_rows(lab, pk.pick_topk(reqs, 4), orc.pick_topk_batch(FUSED, case.pods, oix, reqs, case.B, 4, None, threads=8), f"resident top-4 n={n}")
        on, b1, starts = pk.resident_stats()
        assert b1 - b0 == 3 and starts >= 3, (b1 - b0, starts)
        assert pk.launch_geometry() == (0, 0, 0, 0), "a batch took a launched kernel"
        dp.check_index(pk, oix)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("n", RES_N)
def test_resident_learn_unit_with_more_than_one_block_per_wavefront(pkg, orc, monkeypatch, n):
    """The LEARN unit: eppk_pick_stage_begin(EPPK_PICK_LEARN) of 65..255 rows is answered, and learnt, by the resident workgroup; the plain
    unit then scores the same rows against what was learnt."""
    set_env(monkeypatch, None, "default", EPPK_RESIDENT="1", EPPK_RESIDENT_MAX="255")
    case = dp.case_of(pkg)
    oix = dp.oracle_index(orc, case)                         # (a private one: LEARN changes it)
    s = _res_rows(case, n)
    reqs, lab = case.reqs[s], case.labels[s]
    assert ng.ceil_div(ng.ceil_div(n, 4), RES_WAVES) >= 2
    with dp.picker(pkg, case, FUSED, max_batch=256) as pk:
        on, b0, _ = pk.resident_stats()
        assert on
        sb, _ = pk.stage_buffers(0)
        sb[:n] = reqs
        pk.stage_begin(0, n, learn=True)
        w = orc.pick_batch(FUSED, case.pods, oix, reqs, case.B)[:2]
        oix.insert_picks(reqs, case.B, w[0])
        dp.assert_rows(lab, pk.stage_end(0), w, f"resident LEARN n={n}")
        dp.assert_rows(lab, pk.pick(reqs), orc.pick_batch(FUSED, case.pods, oix, reqs, case.B)[:2], f"resident, after LEARN n={n}")
        assert pk.resident_stats()[1] - b0 == 2
        assert pk.launch_geometry() == (0, 0, 0, 0), "a batch took a launched kernel"
        dp.check_index(pk, oix)


@pytest.mark.timeout(120)
def test_resident_fast_form_unit_serves_255_rows(pkg, orc, monkeypatch):
    """EPPK_RESIDENT_QUAD_FROM=256: plain batches stay with the unit that runs pick_fast_kernel's body -- 16 wavefronts, one row per trip:
    5..16 trips."""
    set_env(monkeypatch, None, "default", EPPK_RESIDENT="1", EPPK_RESIDENT_MAX="255", EPPK_RESIDENT_QUAD_FROM="256")
    case, oix, _ = _corpus(pkg, orc, "main")
    with dp.picker(pkg, case, FUSED, max_batch=256) as pk:
        on, b0, _ = pk.resident_stats()
        assert on
        for n in RES_N:
            s = _res_rows(case, n)
            assert ng.ceil_div(n, RES_WAVES) >= 5
            dp.assert_rows(case.labels[s], pk.pick(case.reqs[s]), orc.pick_batch(FUSED, case.pods, oix, case.reqs[s], case.B)[:2], f"resident fast form n={n}")
        assert pk.resident_stats()[1] - b0 == len(RES_N)
        assert pk.launch_geometry() == (0, 0, 0, 0), "a batch took a launched kernel"
        dp.check_index(pk, oix)
