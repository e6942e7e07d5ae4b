"""CPU: the restatement of the fair resolve (tests/fair_ref.py, SEMANTICS.md §3g) against a row-by-row loop -- a queue per flow, served
round-robin in flow-id order, through a per-request restatement of the rounds; the closed-form place against the sort; the header and
the binding's names; and the generator (tests/fair_cases.py) against its coverage counters."""
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


fc = _load("fair_cases")
ref = fc.ref
CHUNKS = (64, 512)


@pytest.fixture(scope="module")
def corpus():
    """chunk -> (cases, the restatement's answers): computed once, shared, left unchanged."""
    out = {}
    for chunk in CHUNKS:
        cases = fc.make_cases(chunk)
        out[chunk] = (cases, [fc.want(c) for c in cases])
    return out


def loop_resolve(c):
    """The rule, one request at a time: per band a queue per flow, served round-robin in flow-id order; per round every request of that
    order that is still unassigned bids for entry j if its cost fits the pod's room alone, and takes it if the costs of the bidders in
    front of it leave room; one finish behind the last band."""
    L, k = c["lists"], c["lists"].shape[1]
    R, P, bands, nf = L.shape[0], c["n_pods"], c["bands"], c["n_flows"]
    T = np.zeros(L.shape) if c["scores"] is None else c["scores"]
    band = [0] * R if c["band"] is None else [int(b) for b in c["band"]]
    flow = [0] * R if c["flow"] is None else [int(f) for f in c["flow"]]
    cost = [1] * R if c["cost"] is None else [int(x) for x in c["cost"]]
    cap = [c["cap_all"]] * P if c["cap"] is None else [int(x) for x in c["cap"]]
    ld = [0] * P if c["load"] is None else [int(x) for x in c["load"]]
    in_order = [band[r] < len(bands) and flow[r] < nf for r in range(R)]
    bad = [not in_order[r] or not 1 <= cost[r] <= ref.MAX_COST for r in range(R)]
    valid = lambda e: 0 <= e < P                                             # noqa: E731
    pick, score, rank = [ref.NO_PICK] * R, [0.0] * R, [ref.RANK_NONE] * R
    assigned = [False] * R
    flags = 0
    if any(bad):
        flags |= ref.LAUNCH_BAD_REQUEST_ROW
    if any(not valid(int(e)) and int(e) != ref.NO_PICK for e in L.ravel()):
        flags |= ref.LAUNCH_BAD_PICK
    for b, (_, reserve) in enumerate(bands):
        queues = {}
        for r in range(R):
            if in_order[r] and band[r] == b:
                queues.setdefault(flow[r], []).append(r)
        order, turn = [], 0
        while any(len(q) > turn for q in queues.values()):
            order += [queues[f][turn] for f in sorted(queues) if len(queues[f]) > turn]
            turn += 1
        for j in range(k):
            room = [max(cap[p] - min(cap[p], reserve) - ld[p], 0) for p in range(P)]
            S = [0] * P
            for r in order:
                e = int(L[r, j])
                if assigned[r] or bad[r] or not valid(e) or cost[r] > room[e]:
                    continue
                if S[e] + cost[r] <= room[e]:
                    assigned[r], pick[r], score[r], rank[r] = True, e, T[r, j], j
                    ld[e] += cost[r]
                S[e] += cost[r]
    for r in range(R):
        if assigned[r] or bad[r]:
            continue
        first = [i for i in range(k) if valid(int(L[r, i]))]
        if first:
            rank[r] = ref.RANK_OVERFLOW
            if bands[band[r]][0] == ref.SPILL:
                e = int(L[r, first[0]])
                pick[r], score[r], rank[r] = e, T[r, first[0]], ref.RANK_OVERFLOW | first[0]
                ld[e] += cost[r]
    return (np.array(pick, dtype=np.int32), np.array(score, dtype=np.float64), np.array(rank, dtype=np.uint8),
            np.array([x & ref.FULL for x in ld], dtype=np.uint32), flags)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_the_restatement_equals_the_row_by_row_loop(corpus, chunk):
    cases, wants = corpus[chunk]
    for c, w in zip(cases, wants):
        g = loop_resolve(c)
        assert np.array_equal(g[0], w[0]), fc.info(c) + ": picks"
        assert np.array_equal(g[1].view(np.uint64), w[1].view(np.uint64)), fc.info(c) + ": scores"
        assert np.array_equal(g[2], w[2]), fc.info(c) + ": ranks"
        assert np.array_equal(g[3], w[3]), fc.info(c) + ": loads"
        assert g[4] == w[4], fc.info(c) + ": flags"


def test_the_closed_form_place_equals_the_sort(corpus):
    rng = np.random.default_rng(fc.SEED0)
    inputs = [(len(c["bands"]), c["n_flows"], c["band"], c["flow"], c["lists"].shape[0]) for c in corpus[64][0]]
    for _ in range(200):
        nb, nf, R = int(rng.integers(1, 9)), int((1, 2, 3, 9, 64, 1024)[int(rng.integers(0, 6))]), int(rng.integers(0, 300))
        inputs.append((nb, nf, rng.integers(0, nb + 1, size=R).astype(np.uint8), fc.heavy_flows(rng, R, nf) + (rng.random(R) < 0.02), R))
    for nb, nf, band, flow, R in inputs:
        bb, ff, in_order = ref.keys(R, nb, nf, band, flow)
        order = ref.fair_order(bb, ff, in_order, nf)
        place = ref.places(bb, ff, in_order, nb, nf)
        assert np.array_equal(place[order], np.arange(order.size)) and np.all(place[~in_order] == -1)


def test_what_it_buys():
    """§3g's example: batch order gives the flows 6 / 0 / 0 slots, the fair order 2 / 2 / 2."""
    lists, flow, n_flows, cap, rows = fc.tenant_case()
    in_batch_order = ref.resolve(lists, None, 1, None, 1, None, [(ref.SHED, 0)], cap_all=cap)
    assert list(np.nonzero(in_batch_order[0] >= 0)[0]) == [0, 1, 2, 3, 4, 5]
    fair = ref.resolve(lists, None, 1, flow, n_flows, None, [(ref.SHED, 0)], cap_all=cap)
    assert list(np.nonzero(fair[0] >= 0)[0]) == rows
    assert [int(np.count_nonzero(fair[0][flow == f] >= 0)) for f in range(3)] == [2, 2, 2]
    costed = ref.resolve(lists, None, 1, flow, n_flows, np.ones(15, dtype=np.uint32), [(ref.SHED, 0)], cap_all=cap)
    assert all(np.array_equal(a, b) for a, b in zip(fair[:4], costed[:4])), "a null cost is a cost array of ones"


def test_one_flow_is_the_costed_and_the_banded_restatement(corpus):
    """Identity 1 of §3g on the restatements: n_flows = 1 / no flow array is tests/costed_ref.py, without costs tests/banded_ref.py."""
    for c in corpus[64][0]:
        if c["band"] is not None and np.any(c["band"] >= len(c["bands"])) and c["cost"] is None:
            continue                                                         # (a bad band under banded_ref: the same answer, kept simple)
        got = ref.resolve(c["lists"], c["scores"], c["n_pods"], None, 1, c["cost"], c["bands"], c["band"], c["cap"], c["cap_all"], c["load"])
        if c["cost"] is None:
            want = ref.banded.resolve(c["lists"], c["scores"], c["n_pods"], c["bands"], c["band"], c["cap"], c["cap_all"], c["load"])
        else:
            want = ref.costed.resolve(c["lists"], c["scores"], c["n_pods"], c["cost"], c["bands"], c["band"], c["cap"], c["cap_all"], c["load"])
        assert all(np.array_equal(a, b) for a, b in zip(got[:4], want[:4])) and got[4] == want[4], fc.info(c)


def test_the_header_declares_the_four_exports_and_the_binding_names_them():
    with open(os.path.join(ROOT, "include", "eppk.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+EPPK_ABI_VERSION\s+4u", header)
    assert re.search(r"#define\s+EPPK_MAX_FLOWS\s+1024u", header)
    lib = _load("eppk_lib_names", os.path.join(ROOT, "gateway-api-inference-extension_amd", "_lib.py"))
    for name in ("eppk_fair_resolve_device", "eppk_pick_fair_device", "eppk_pick_fair", "eppk_group_pick_fair"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in lib.SYMBOLS, name
    assert lib.EPPK_MAX_FLOWS == 1024
    decl = re.search(r"int\s+eppk_fair_resolve_device\s*\(([^;]*)\)\s*;", header).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    assert names == ["ctx", "d_lists", "d_list_scores", "n_reqs", "k", "d_flow", "n_flows", "d_cost", "cost_flags", "d_band", "bands", "d_cap", "cap_all",
                     "d_load", "d_out_pick", "d_out_score", "d_out_rank", "stream"]


@pytest.mark.parametrize("chunk", CHUNKS)
def test_the_generator_covers_every_required_situation(corpus, chunk):
    cases, wants = corpus[chunk]
    seen = fc.coverage(cases, chunk, wants)
    required = set(fc.REQUIRED)
    if chunk == 64:
        required.discard("pair-in-adjacent-trips")                           # (a chunk of 64 rows is one trip: the default chunk has them)
    assert not required - seen, sorted(required - seen)
    assert sum(c["lists"].shape[0] <= 1100 and c["n_pods"] <= 64 for c in cases) == len(cases)
    # the caps bind in most cases: the order decides who is placed
    assert sum(bool((w[2] & ref.RANK_OVERFLOW).any() and (w[2] < 8).any()) for w in wants) > len(cases) // 2
