"""CPU: the restatement of the weighted fair resolve (tests/wfair_ref.py, SEMANTICS.md §3h): the closed-form place against the sort;
weights of one and turns of zero against tests/fair_ref.py; the rebase equality; the worked examples of §3h; the header and the
binding's names; the generator (tests/wfair_cases.py) against its coverage; and eppk_fair_turns_rebase, a host function that needs no
device, through ctypes against wfair_ref.rebase."""
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path=None):
    spec = importlib.util.spec_from_file_location(name, path or os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


wc = _load("wfair_cases")
ref = wc.ref
CHUNKS = (64, 512)
TOP = ref.TOP


@pytest.fixture(scope="module")
def corpus():
    """chunk -> (cases, the restatement's answers): computed once, shared, left unchanged."""
    out = {}
    for chunk in CHUNKS:
        cases = wc.make_cases(chunk)
        out[chunk] = (cases, [wc.want(c) for c in cases])
    return out


@pytest.mark.parametrize("chunk", CHUNKS)
def test_the_generator_covers_every_required_situation(corpus, chunk):
    cases, wants = corpus[chunk]
    seen = wc.coverage(cases, chunk, wants)
    assert not set(wc.REQUIRED) - seen, sorted(set(wc.REQUIRED) - seen)
    assert sum(c["lists"].shape[0] <= 1100 and c["n_pods"] <= 64 for c in cases) == len(cases)
    # the caps bind in most cases: the order decides who is placed
    assert sum(bool((w[2] & ref.RANK_OVERFLOW).any() and (w[2] < 8).any()) for w in wants) > len(cases) // 2


def test_the_closed_form_place_equals_the_sort(corpus):
    """On every case of the generator, and on random keys under weights up to 65535 and turns up to 2^32 - 1."""
    rng = np.random.default_rng(wc.SEED0)
    inputs = [(len(c["bands"]), c["n_flows"], c["band"], c["flow"], c["weight"], c["turns"], c["lists"].shape[0]) for c in corpus[64][0] + corpus[512][0]]
    for i in range(150):
        nb, nf, R = int(rng.integers(1, 9)), int((1, 2, 3, 9, 64, 1024)[int(rng.integers(0, 6))]), int(rng.integers(0, 300))
        wtop, ttop = ((1, 0), (5, 12), (65535, TOP), (3, TOP), (65535, 70000))[i % 5]
        weight = rng.integers(0 if i % 7 == 0 else 1, wtop + 1, size=nf)
        inputs.append((nb, nf, rng.integers(0, nb + 1, size=R).astype(np.uint8), wc.fc.heavy_flows(rng, R, nf) + (rng.random(R) < 0.02), weight,
                       rng.integers(0, ttop + 1, size=(nb, nf)), R))
    for nb, nf, band, flow, weight, turns, R in inputs:
        w, t = ref.tables(nb, nf, weight, turns)
        bb, ff, in_order = ref.keys(R, nb, nf, band, flow, weight)
        order = ref.order(bb, ff, in_order, nf, w, t)
        place = ref.places(bb, ff, in_order, nb, nf, w, t)
        assert np.array_equal(place[order], np.arange(order.size)) and np.all(place[~in_order] == -1)
        if weight is None and turns is None:
            assert np.array_equal(place, ref.fair.places(bb, ff, in_order, nb, nf)), "weights 1, turns 0: §3g's closed form"


def _same(a, b, what):
    for x, y, name in zip(a[:4], b[:4], ("picks", "scores", "ranks", "loads")):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), f"{what}: {name}"
    assert a[4] == b[4], f"{what}: flags"


def test_weights_of_one_and_turns_of_zero_are_the_fair_restatement(corpus):
    for c in corpus[64][0]:
        nb, nf = len(c["bands"]), c["n_flows"]
        args = (c["cost"], c["bands"], c["band"], c["cap"], c["cap_all"], c["load"])
        want = ref.fair.resolve(c["lists"], c["scores"], c["n_pods"], c["flow"], nf, *args)
        _same(ref.resolve(c["lists"], c["scores"], c["n_pods"], c["flow"], nf, None, None, *args), want, wc.info(c) + " (NULL / NULL)")
        got = ref.resolve(c["lists"], c["scores"], c["n_pods"], c["flow"], nf, np.ones(nf, dtype=np.uint16), np.zeros((nb, nf), dtype=np.uint32), *args)
        _same(got, want, wc.info(c) + " (ones / zeros)")


def test_a_rebase_changes_no_answer(corpus):
    """turns + m * weight per band, without saturation: the same picks, ranks, scores and loads, and the turns handed back moved alike."""
    rng = np.random.default_rng(wc.SEED0 + 1)
    done = 0
    for c, want in zip(*corpus[64]):
        if c["turns"] is None:
            continue
        nb, nf = len(c["bands"]), c["n_flows"]
        w, t = ref.tables(nb, nf, c["weight"], c["turns"])
        room = (TOP - want[5].astype(np.int64).max(axis=1)) // w.max()
        m = np.minimum(rng.integers(1, 1000, size=nb), room)[:, None]
        if not m.any():
            continue
        got = wc.want(dict(c, turns=(t + m * w).astype(np.uint32)))
        _same(got, want, wc.info(c))
        live = w >= 1
        assert np.array_equal(got[5].astype(np.int64)[:, live], (want[5].astype(np.int64) + m * w)[:, live]), wc.info(c)
        done += 1
    assert done >= 10


def test_the_worked_examples():
    """§3h: (1) weights (3, 1, 1) over five slots place 3 / 1 / 1; (2) one slot per batch and turns carried: the flows take it in turn,
    and without turns flow 0 takes it every time."""
    lists, flow, weight, cap, rows = wc.shares_case()
    got = ref.resolve(lists, None, 1, flow, 3, weight, None, None, [(ref.SHED, 0)], cap_all=cap)
    assert list(np.nonzero(got[0] >= 0)[0]) == rows
    assert [int(np.count_nonzero(got[0][flow == f] >= 0)) for f in range(3)] == [3, 1, 1]
    assert got[5] is None
    lists, flow = np.zeros((3, 1), dtype=np.int32), np.arange(3, dtype=np.uint16)
    turns, placed, stateless = np.zeros((1, 3), dtype=np.uint32), [], []
    for _ in range(3):
        pick, _, _, load, _, turns = ref.resolve(lists, None, 1, flow, 3, None, turns, None, [(ref.SHED, 0)], cap_all=1, load=np.zeros(1, dtype=np.uint32))
        assert load[0] == 1
        placed.append(int(np.nonzero(pick >= 0)[0][0]))
        stateless.append(int(np.nonzero(ref.resolve(lists, None, 1, flow, 3, None, None, None, [(ref.SHED, 0)], cap_all=1)[0] >= 0)[0][0]))
    assert placed == [0, 1, 2] and stateless == [0, 0, 0] and turns.tolist() == [[1, 1, 1]]


def test_the_header_declares_the_exports_and_the_binding_names_them():
    with open(os.path.join(ROOT, "include", "eppk.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+EPPK_ABI_VERSION\s+4u", header)
    lib = _load("eppk_lib_names", os.path.join(ROOT, "gateway-api-inference-extension_amd", "_lib.py"))
    for name in ("eppk_wfair_resolve_device", "eppk_pick_wfair_device", "eppk_pick_wfair", "eppk_group_pick_wfair", "eppk_fair_turns_rebase"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SYMBOLS, name

    def names(fn):
        decl = re.search(r"int\s+" + fn + r"\s*\(([^;]*)\)\s*;", header).group(1)
        return [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]

    assert names("eppk_wfair_resolve_device") == ["ctx", "d_lists", "d_list_scores", "n_reqs", "k", "d_flow", "n_flows", "d_weight", "d_turns", "d_cost",
                                                  "cost_flags", "d_band", "bands", "d_cap", "cap_all", "d_load", "d_out_pick", "d_out_score", "d_out_rank",
                                                  "stream"]
    assert names("eppk_pick_wfair_device") == ["ctx", "d_reqs", "n_reqs", "d_cand_mask", "k", "d_flow", "n_flows", "d_weight", "d_turns", "d_cost", "d_band",
                                               "bands", "d_cap", "cap_all", "d_load", "d_out_pick", "d_out_score", "d_out_rank", "stream"]
    host = ["reqs", "n_reqs", "cand_mask", "k", "flow", "n_flows", "weight", "turns", "cost", "band", "bands", "cap", "cap_all", "load", "out_pick", "out_score",
            "out_rank"]
    assert names("eppk_pick_wfair") == ["ctx"] + host and names("eppk_group_pick_wfair") == ["g"] + host
    assert names("eppk_fair_turns_rebase") == ["turns", "weight", "n_bands", "n_flows", "window"]
    assert header.index("eppk_group_pick_fair(") < header.index("eppk_wfair_resolve_device(") < header.index("adjacent host-side steps") < \
        header.index("eppk_fair_turns_rebase(")


# ---- eppk_fair_turns_rebase: host memory in, host memory out ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


def _rebase(lib, turns, weight, window):
    t = np.ascontiguousarray(turns, dtype=np.uint32).copy()
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.uint16)
    rc = lib.eppk_fair_turns_rebase(t.ctypes.data, None if w is None else w.ctypes.data, t.shape[0], t.shape[1], window)
    return rc, t


def test_turns_rebase_equals_the_restatement(lib):
    rng = np.random.default_rng(wc.SEED0 + 2)
    cases = [
        ([[10, 0, 7], [3, 3, 3]], [2, 1, 0], 2),                             # an idle flow beyond the window; weight 0 left alone
        ([[1000000, 0, 999990]], None, 5),
        ([[TOP, TOP - 1, 0, TOP - 65535 * 3]], [65535, 65535, 65535, 65534], 1),   # weights 65535 with turns near 2^32
        ([[TOP, 0]], [1, 65535], 0),                                         # the lift passes 32 bits on its way
        ([[TOP, 0]], [1, 65535], TOP),
        ([[5, 9, 5]], [0, 0, 0], 1),                                         # nobody has a weight: nothing moves
    ]
    for i in range(60):
        nb, nf = int(rng.integers(1, 9)), int((1, 2, 5, 64, 1024)[i % 5])
        wtop, ttop = ((1, 50), (7, 500), (65535, TOP), (65535, 200000))[i % 4]
        weight = None if i % 6 == 0 else rng.integers(0 if i % 3 == 0 else 1, wtop + 1, size=nf)
        cases.append((rng.integers(0, ttop + 1, size=(nb, nf)), weight, int((0, 1, TOP, 3, 1000)[i % 5])))
    for turns, weight, window in cases:
        want = ref.rebase(np.asarray(turns, dtype=np.uint32), weight, window)
        rc, got = _rebase(lib, turns, weight, window)
        assert rc == 0 and np.array_equal(got, want), (turns, weight, window)
    assert {0, 1, TOP} <= {c[2] for c in cases}
    # what it is for: the order of the next batch does not change, and nobody is more than `window` cycles behind
    rc, got = _rebase(lib, [[10, 0, 7]], [2, 1, 0], 2)
    assert got.tolist() == [[4, 0, 7]]


def test_turns_rebase_refuses_bad_arguments(lib):
    t = np.full((8, 4), 7, dtype=np.uint32)
    ARG = -1
    assert lib.eppk_fair_turns_rebase(None, None, 1, 4, 0) == ARG
    for nb, nf in ((0, 4), (9, 4), (1, 0), (1, 1025)):
        assert lib.eppk_fair_turns_rebase(t.ctypes.data, None, nb, nf, 0) == ARG
    assert np.all(t == 7), "a refused call writes nothing"
    big = np.zeros((8, 1024), dtype=np.uint32)
    assert lib.eppk_fair_turns_rebase(big.ctypes.data, None, 8, 1024, 0) == 0
