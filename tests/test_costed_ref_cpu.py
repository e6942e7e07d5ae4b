"""CPU: the numpy restatement of the costed resolve (tests/costed_ref.py, SEMANTICS.md §3f) against a row-by-row loop of the rule and
hand-computed answers; every cost 1 against tests/banded_ref.py; the case generator the GPU tests run (tests/costed_cases.py) against
the list of situations that have to occur in it -- observed by the loop, not declared by the generator; and the new symbols."""
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


cases = _load("costed_cases")
ref = cases.ref
banded = ref.banded                                                   # tests/banded_ref.py
SHED, SPILL, NO = ref.SHED, ref.SPILL, ref.NO_PICK
MAX_COST, FULL = ref.MAX_COST, ref.FULL
CHUNKS = (64, 512)


def brute(c, chunk=None, seen=None):
    """§3f word for word: band after band, round after round, request after request; every sum a Python int.  With `chunk` and `seen`
    it also records which of cases.SITUATIONS occur, by the place a request has in the order the device walks: the batch order in the
    one-launch form (n <= chunk), the place inside the band's segment else."""
    L, T, P, bands = c["lists"], c["scores"], c["n_pods"], c["bands"]
    R, k = L.shape
    band = np.zeros(R, dtype=np.uint8) if c["band"] is None else c["band"]
    cost = c["cost"] if c["per_entry"] else np.repeat(c["cost"][:, None], k, axis=1)
    capv = [c["cap_all"]] * P if c["cap"] is None else [int(x) for x in c["cap"]]
    ld = [0] * P if c["load"] is None else [int(x) for x in c["load"]]
    pick, score, rank = [NO] * R, [0.0] * R, [ref.RANK_NONE] * R
    valid = lambda e: 0 <= e < P                                       # noqa: E731
    note = (lambda s: seen.add(s)) if seen is not None else (lambda s: None)
    bad = [False] * R
    for r in range(R):
        for i in range(k):
            ci, ok = int(cost[r, i]), 1 <= int(cost[r, i]) <= MAX_COST
            if c["per_entry"] and not valid(int(L[r, i])):
                if not ok:
                    note("bad-cost-behind-invalid-entry-candidate")
                continue
            if not ok:
                bad[r] = True
                note("cost-0" if ci == 0 else "cost-MAX+1" if ci == MAX_COST + 1 else "cost-other")
        if band[r] >= len(bands):
            bad[r] = True
            note("band>=n_bands")
    if c["per_entry"] and seen is not None and "bad-cost-behind-invalid-entry-candidate" in seen:
        # a row whose ONLY bad costs sit behind invalid entries, and which is not bad
        for r in range(R):
            behind = any(not valid(int(L[r, i])) and not 1 <= int(cost[r, i]) <= MAX_COST for i in range(k))
            if behind and not bad[r]:
                note("bad-cost-behind-invalid-entry")
    one_launch = chunk is None or R <= chunk
    left_all = []
    for b, (policy, reserve) in enumerate(bands):
        in_band = [r for r in range(R) if band[r] == b]
        place = {r: (r if one_launch else i) for i, r in enumerate(in_band)}
        s0 = sum(1 for r in range(R) if band[r] < b)
        ck = chunk if (chunk is not None and not one_launch) else 1 << 62
        cap_b = [cv - min(cv, reserve) for cv in capv]
        left = [r for r in in_band if not bad[r]]
        for j in range(k):
            S, still, trail, taken = {}, [], {}, {}                    # (the takers' totals reach the loads behind the round)
            for r in left:
                e = int(L[r, j])
                if not valid(e):
                    still.append(r)
                    continue
                rm = max(cap_b[e] - ld[e], 0)                          # on the loads as the round before left them
                ci = int(cost[r, j])
                tr = trail.setdefault(e, [])
                if ci > rm:                                            # could not fit even alone: no bidder, counts for nothing
                    still.append(r)
                    tr.append((place[r], "x", 0))
                    continue
                if ci == MAX_COST:
                    note("c==MAX")
                s = S.get(e, 0)
                if s + ci <= rm:
                    pick[r], score[r], rank[r] = e, 0.0 if T is None else float(T[r, j]), j
                    taken[e] = taken.get(e, 0) + ci
                    tr.append((place[r], "t", s + ci))
                    if s + ci == rm:
                        note("S+c==room")
                else:
                    still.append(r)
                    tr.append((place[r], "n", s + ci))
                    if s + ci == rm + 1:
                        note("S+c==room+1")
                S[e] = s + ci
            for e, add in taken.items():
                ld[e] += add
                if ld[e] == FULL and cap_b[e] == FULL:
                    note("load+takers==cap==FULL")
            left = still
            if seen is not None:
                for e, tr in trail.items():
                    _observe(tr, ck, chunk or 64, s0, cap_b[e] == FULL, note)
        left_all += left
    for r in left_all:
        first = [i for i in range(k) if valid(int(L[r, i]))]
        if not first:
            continue
        rank[r] = ref.RANK_OVERFLOW
        if bands[band[r]][0] == SPILL:
            e = int(L[r, first[0]])
            pick[r], score[r], rank[r] = e, 0.0 if T is None else float(T[r, first[0]]), ref.RANK_OVERFLOW | first[0]
            if ld[e] <= FULL < ld[e] + int(cost[r, first[0]]):
                note("spill-wraps")
            ld[e] += int(cost[r, first[0]])
    flags = ref.LAUNCH_BAD_PICK if any(int(e) != NO and not valid(int(e)) for e in L.ravel()) else 0
    flags |= ref.LAUNCH_BAD_REQUEST_ROW if any(bad) else 0
    return (np.array(pick, dtype=np.int32), np.array(score, dtype=np.float64), np.array(rank, dtype=np.uint8),
            np.array([x & FULL for x in ld], dtype=np.uint32), flags)


def _observe(tr, ck, chunk, s0, cap_full, note):
    """tr: one pod's requests of one round in walking order, (place, 't'aker | eligible 'n'on-taker | ine'x'ligible, S + c)."""
    takers = [q for q, kind, _ in tr if kind == "t"]
    misses = [q for q, kind, _ in tr if kind == "n"]
    if takers and misses:
        a, bnd = takers[-1], misses[0]
        assert a < bnd, "the takers are a prefix of the bidders"
        if a // 64 == bnd // 64:
            note("boundary-in-trip")
        if a % 64 == 63 and bnd == a + 1:
            note("boundary-between-trips")
        if bnd == a + 1 and bnd % ck == 0:
            note("boundary-at-chunk")
            if s0 % ck:
                note("boundary-at-chunk-of-ragged-segment")
    if len(takers) >= 2 and any(kind == "x" and takers[0] < q < takers[-1] for q, kind, _ in tr):
        note("ineligible-between-takers")
    if cap_full:
        bids = [(q, s) for q, kind, s in tr if kind != "x"]
        for (x, sx), (y, sy) in zip(bids, bids[1:]):
            if sx <= FULL < sy:
                if x // 64 == y // 64:
                    note("2^32-in-trip")
                if x // ck == y // ck and (x // 64 != y // 64 or chunk == 64):
                    note("2^32-in-chunk")
                if x // ck != y // ck:
                    note("2^32-across-chunks")


def _same(got, want, what):
    for g, w, name in zip(got[:4], want[:4], ("picks", "scores", "ranks", "loads")):
        assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)), f"{what}: {name}: {g[:12]} against {w[:12]}"
    assert got[4] == want[4], f"{what}: flags {got[4]} against {want[4]}"


@pytest.fixture(scope="module", params=CHUNKS)
def generated(request):
    chunk = request.param
    cs = cases.make_cases(chunk)
    seen, answers = set(), []
    for c in cs:
        answers.append(brute(c, chunk, seen) if c["n_pods"] <= 100 else None)
    return chunk, cs, answers, seen


def test_the_restatement_equals_the_row_by_row_loop_on_every_case(generated):
    chunk, cs, answers, _ = generated
    for c, a in zip(cs, answers):
        _same(cases.want(c), a if a is not None else brute(c), cases.info(c))


def test_hand_computed_answers():
    lists, cost, band, table, cap = cases.two_request_case()
    pick, _, rank, load, flags = ref.resolve(lists, None, 1, cost, table, band, None, cap, np.zeros(1, dtype=np.uint32))
    assert pick.tolist() == [0, 0] and rank.tolist() == [0x40, 0] and load.tolist() == [30] and flags == 0
    pick, _, rank, load, _ = ref.resolve(lists, None, 1, cost, table, band, None, cap, np.zeros(1, dtype=np.uint32), finish_per_band=True)
    assert pick.tolist() == [0, -1] and rank.tolist() == [0x40, 0x40] and load.tolist() == [20]
    # room 10: 3 takes, 50 could not fit alone and counts for nothing, 3 and 4 take (S + c == 10), the next 1 misses by one -- and so
    # does every later one: the takers are a prefix of the bidders.  The 50 goes on to its second entry.
    pick, _, rank, load, _ = ref.resolve([[0, 1], [0, 1], [0, 1], [0, 1], [0, NO], [0, NO]], None, 2, [3, 50, 3, 4, 1, 1], [(SHED, 0)], None, [10, 60],
                                         0, np.zeros(2, dtype=np.uint32))
    assert pick.tolist() == [0, 1, 0, 0, -1, -1] and rank.tolist() == [0, 1, 0, 0, 0x40, 0x40] and load.tolist() == [10, 50]
    # 257 requests of EPPK_MAX_COST on a pod with cap 2^32 - 1: the sum passes 2^32 at the last; 256 fit
    pick, _, _, load, _ = ref.resolve(np.zeros((257, 1), dtype=np.int32), None, 1, np.full(257, MAX_COST), [(SHED, 0)], None, None, FULL, np.zeros(1, dtype=np.uint32))
    assert pick.tolist() == [0] * 256 + [-1] and load.tolist() == [256 * MAX_COST]
    # a spill adds the request's cost, modulo 2^32 in what is handed back
    pick, _, rank, load, _ = ref.resolve([[0]], None, 1, [0x20], [(SPILL, 0)], None, None, FULL, np.array([FULL - 1], dtype=np.uint32))
    assert pick.tolist() == [0] and rank.tolist() == [0x40] and load.tolist() == [0x1E]
    # bad rows: cost 0, cost too large, band byte >= n_bands -- no room taken; per entry a bad cost behind an invalid entry is not read
    pick, _, rank, load, flags = ref.resolve([[0], [0], [0], [0]], None, 1, [0, MAX_COST + 1, 2, 2], [(SHED, 0)], [0, 0, 1, 0], None, 2, np.zeros(1, dtype=np.uint32))
    assert pick.tolist() == [-1, -1, -1, 0] and rank.tolist() == [0x80, 0x80, 0x80, 0] and load.tolist() == [2] and flags == ref.LAUNCH_BAD_REQUEST_ROW
    pick, _, rank, _, flags = ref.resolve([[NO, 0], [5, 0]], None, 1, [[0, 1], [0, 1]], [(SHED, 0)], None, None, 2, None, per_entry=True)
    assert pick.tolist() == [0, 0] and rank.tolist() == [1, 1] and flags == ref.LAUNCH_BAD_PICK


def test_every_cost_one_is_the_banded_resolve(generated):
    chunk, cs, _, _ = generated
    for c in cs:
        u = cases.unit_cost(c)
        _same(cases.want(u), banded.resolve(c["lists"], c["scores"], c["n_pods"], c["bands"], c["band"], c["cap"], c["cap_all"], c["load"]), cases.info(c))


def test_mixed_costs_answer_otherwise_than_counts(generated):
    """A device that ignored the costs would give the banded resolve's picks: the GPU tests cannot pass on it."""
    chunk, cs, _, _ = generated
    differ = sum(not np.array_equal(cases.want(c)[0], cases.want(cases.unit_cost(c))[0]) for c in cs)
    assert differ >= len(cs) // 2, (differ, len(cs))


def test_no_pod_ends_above_its_cap_in_cost_units_under_shed(generated):
    chunk, cs, _, _ = generated
    checked = 0
    for c in cs:
        if not cases.host_ok(c):
            continue
        bands = [(SHED, r) for _, r in c["bands"]]
        P = c["n_pods"]
        load_in = np.zeros(P, dtype=np.int64) if c["load"] is None else c["load"].astype(np.int64)
        pick, _, _, load, _ = ref.resolve(c["lists"], c["scores"], P, c["cost"], bands, c["band"], c["cap"], c["cap_all"], load_in.astype(np.uint32))
        band = np.zeros(pick.size, dtype=np.uint8) if c["band"] is None else c["band"]
        placed = np.zeros(P, dtype=np.int64)
        np.add.at(placed, pick[pick >= 0], c["cost"][pick >= 0].astype(np.int64))
        assert np.array_equal(load.astype(np.int64), load_in + placed)
        for p in np.unique(pick[pick >= 0]):
            last = int(band[pick == p].max())
            cap_b = int(banded.band_caps(P, c["cap"], c["cap_all"], bands[last][1])[p])
            assert int(load[p]) <= max(cap_b, int(load_in[p])), (cases.info(c), int(p))
            checked += 1
    assert checked > 100


def test_the_generator_covers_what_it_has_to(generated):
    chunk, cs, _, seen = generated
    tags = set().union(*(c["tags"] for c in cs))
    assert not set(cases.REQUIRED) - tags, sorted(set(cases.REQUIRED) - tags)
    assert len({c["name"] for c in cs}) == len(cs)
    for c in cs:                                                       # the deferred finish and a finish per band differ somewhere under SPILL
        if any(p == SPILL for p, _ in c["bands"]) and not np.array_equal(cases.want(c)[0], cases.want(c, finish_per_band=True)[0]):
            seen.add("deferred-differs")
    assert not set(cases.SITUATIONS) - seen, sorted(set(cases.SITUATIONS) - seen)
    sizes = {c["lists"].shape[0] for c in cs}
    assert {0, 1, 63, 64, 65, 127, 129, chunk - 1, chunk, chunk + 1, 2 * chunk + 3, 9 * chunk + 5} <= sizes and max(sizes) == 9 * chunk + 5
    assert max(c["n_pods"] for c in cs) == 4096
    for c in cs:
        banded.check_table(c["bands"])
        n = c["lists"].shape[0]
        assert c["band"] is None or c["band"].shape == (n,)
        assert ("one-launch" not in c["tags"] or n <= chunk) and ("chunked" not in c["tags"] or n > chunk)
    assert any(not cases.host_ok(c) for c in cs) and any(c["per_entry"] for c in cs)


def test_symbols_header_and_binding_agree_on_the_new_names():
    with open(os.path.join(ROOT, "include", "eppk.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    with open(os.path.join(ROOT, "gateway-api-inference-extension_amd", "_lib.py")) as f:
        src = f.read()
    syms = set(re.findall(r'"(eppk_[a-z0-9_]+)"', re.search(r"SYMBOLS = \[(.*?)\]", src, re.S).group(1)))
    new = {"eppk_costed_resolve_device", "eppk_pick_costed_device", "eppk_pick_costed", "eppk_group_pick_costed"}
    declared = set(re.findall(r"\b(eppk_[a-z0-9_]+)\s*\(", hdr))
    assert {s for s in declared if "costed" in s} == {s for s in syms if "costed" in s} == new
    for name in new:
        assert re.search(r"lib\.%s\.argtypes = \[" % name, src), f"{name} has no argtypes"
    assert re.search(r"#define EPPK_MAX_COST 0x00FFFFFFu", hdr) and re.search(r"^EPPK_MAX_COST = 0x00FFFFFF$", src, re.M)
    assert re.search(r"#define EPPK_COST_PER_ENTRY 1u", hdr) and re.search(r"^EPPK_COST_PER_ENTRY = 1$", src, re.M)
    assert re.search(r"#define EPPK_ABI_VERSION 4u\b", hdr), "additive: the ABI version stays"
    lib = os.path.join(ROOT, "gateway-api-inference-extension_amd", "libeppk.so")
    if os.path.exists(lib):                                            # (built: the library exports them)
        import subprocess
        exported = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        assert new <= set(re.findall(r"\b(eppk_[a-z0-9_]+)\b", exported))
