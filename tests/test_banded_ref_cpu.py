"""CPU: the numpy restatement of the banded resolve (tests/banded_ref.py, SEMANTICS.md §3e) against a naive per-request, per-round loop and
hand-computed answers; the identities §3e states; and the case generator the GPU tests run (tests/banded_cases.py) against its own list
of what it has to cover."""
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


cases = _load("banded_cases")
ref = cases.ref
plain = ref.ref                                                       # tests/bounded_ref.py
SHED, SPILL, NO = ref.SHED, ref.SPILL, ref.NO_PICK
CHUNKS = (64, 512)


def naive(c):
    """§3e word for word: band after band, round after round, request after request; the loads are Python ints (carried exactly)."""
    L, T, P, bands = c["lists"], c["scores"], c["n_pods"], c["bands"]
    R, k = L.shape
    band = np.zeros(R, dtype=np.uint8) if c["band"] is None else c["band"]
    capv = [c["cap_all"]] * P if c["cap"] is None else [int(x) for x in c["cap"]]
    ld = [0] * P if c["load"] is None else [int(x) for x in c["load"]]
    pick, score, rank = [NO] * R, [0.0] * R, [ref.RANK_NONE] * R
    valid = lambda e: 0 <= e < P                                       # noqa: E731
    for b, (policy, reserve) in enumerate(bands):
        rows = [r for r in range(R) if band[r] == b]
        cap_b = [cv - min(cv, reserve) for cv in capv]
        left = list(rows)
        for j in range(k):
            room = [max(cap_b[p] - ld[p], 0) for p in range(P)]        # on the loads as the round before left them
            bidders = [0] * P
            still = []
            for r in left:
                e = int(L[r, j])
                if not valid(e):
                    still.append(r)
                    continue
                if bidders[e] < room[e]:
                    pick[r], score[r], rank[r] = e, 0.0 if T is None else float(T[r, j]), j
                    ld[e] += 1
                else:
                    still.append(r)
                bidders[e] += 1
            left = still
        for r in left:
            first = [i for i in range(k) if valid(int(L[r, i]))]
            if not first:
                continue
            rank[r] = ref.RANK_OVERFLOW
            if policy == SPILL:
                e = int(L[r, first[0]])
                pick[r], score[r], rank[r] = e, 0.0 if T is None else float(T[r, first[0]]), ref.RANK_OVERFLOW | first[0]
                ld[e] += 1
    flags = ref.LAUNCH_BAD_PICK if any(int(e) != NO and not valid(int(e)) for e in L.ravel()) else 0
    flags |= ref.LAUNCH_BAD_REQUEST_ROW if any(int(x) >= len(bands) for x in band) else 0
    return (np.array(pick, dtype=np.int32), np.array(score, dtype=np.float64), np.array(rank, dtype=np.uint8),
            np.array([x & 0xFFFFFFFF for x in ld], dtype=np.uint32), flags)


def _same(got, want, what):
    for g, w, name in zip(got[:4], want[:4], ("picks", "scores", "ranks", "loads")):
        assert np.array_equal(np.asarray(g).view(np.uint8), np.asarray(w).view(np.uint8)), f"{what}: {name}: {g[:12]} against {w[:12]}"
    assert got[4] == want[4], f"{what}: flags"


def _small(c):
    return c["lists"].shape[0] <= 700 and c["n_pods"] <= 100


@pytest.fixture(scope="module", params=CHUNKS)
def generated(request):
    return request.param, cases.make_cases(request.param)


def test_the_restatement_equals_the_naive_loop(generated):
    chunk, cs = generated
    checked = 0
    for c in cs:
        if _small(c):
            _same(cases.want(c), naive(c), cases.info(c))
            checked += 1
    assert checked >= 40


def test_hand_computed_answers():
    lists, band = cases.operator_case()
    # what the plain resolve does today: batch order decides, the critical rows 2 and 3 lose pod 0 to the sheddable row 0
    assert plain.resolve(lists, None, 2, None, 1, SHED, None)[0].tolist() == [0, -1, -1, 1]
    pick, score, rank, load, flags = ref.resolve(lists, None, 2, [(SHED, 0), (SHED, 0)], band, None, 1, np.zeros(2, dtype=np.uint32))
    assert pick.tolist() == [-1, -1, 0, 1] and rank.tolist() == [0x40, 0x40, 0, 0] and load.tolist() == [1, 1] and flags == 0
    # two slots per pod, one reserved against band 1: band 0 takes row 2 -> pod 0, row 3 -> pod 1; band 1 sees cap 1 and both pods at 1
    pick, _, rank, load, _ = ref.resolve(lists, None, 2, [(SHED, 0), (SPILL, 1)], band, None, 2, np.zeros(2, dtype=np.uint32))
    assert pick.tolist() == [0, 0, 0, 1] and rank.tolist() == [0x40, 0x40, 0, 0] and load.tolist() == [3, 1]
    # ... without the reserve band 1 fills what band 0 left: row 0 -> pod 0, row 1 refused there, -> pod 1 in round 1
    pick, _, rank, load, _ = ref.resolve(lists, None, 2, [(SHED, 0), (SPILL, 0)], band, None, 2, np.zeros(2, dtype=np.uint32))
    assert pick.tolist() == [0, 1, 0, 1] and rank.tolist() == [0, 1, 0, 0] and load.tolist() == [2, 2]
    # a band byte >= n_bands: no room taken, NO_PICK / RANK_NONE, and the flag; the row behind it gets the slot
    pick, _, rank, load, flags = ref.resolve([[0], [0]], None, 1, [(SHED, 0)], [1, 0], None, 1, np.zeros(1, dtype=np.uint32))
    assert pick.tolist() == [-1, 0] and rank.tolist() == [0x80, 0] and load.tolist() == [1] and flags == ref.LAUNCH_BAD_REQUEST_ROW
    # band 0 spills two requests onto a pod at 2^32 - 2: the load handed back wraps to 0, and band 1 finds no room there
    full = 0xFFFFFFFF
    pick, _, rank, load, _ = ref.resolve([[0], [0], [0]], None, 1, [(SPILL, 0), (SHED, 0)], [0, 0, 1], None, full, np.array([full - 1], dtype=np.uint32))
    assert pick.tolist() == [0, 0, -1] and rank.tolist() == [0, 0x40, 0x40] and load.tolist() == [0]


def test_one_band_without_reserve_is_the_plain_resolve(generated):
    chunk, cs = generated
    for c in cs:
        if not cases.host_ok(c):
            continue
        for policy in (SHED, SPILL):
            got = ref.resolve(c["lists"], c["scores"], c["n_pods"], [(policy, 0)], None, c["cap"], c["cap_all"], c["load"])
            want = plain.resolve(c["lists"], c["scores"], c["n_pods"], c["cap"], c["cap_all"], policy, c["load"])
            _same(got, want[:4] + (ref.LAUNCH_BAD_PICK if want[4] else 0,), cases.info(c))


def _deferred(c):
    """What the device does: every band's rounds first (a band's unplaced requests wait), ONE finish behind the last band."""
    L, P, bands = c["lists"], c["n_pods"], c["bands"]
    R, k = L.shape
    T = np.zeros((R, k)) if c["scores"] is None else c["scores"]
    band = np.zeros(R, dtype=np.uint8) if c["band"] is None else c["band"]
    pick, score, rank = np.full(R, NO, dtype=np.int32), np.zeros(R), np.full(R, ref.RANK_NONE, dtype=np.uint8)
    ld = np.zeros(P, dtype=np.uint32) if c["load"] is None else c["load"].copy()
    for b, (_, reserve) in enumerate(bands):
        rows = np.nonzero(band == b)[0]
        if rows.size:
            cap_b = ref.band_caps(P, c["cap"], c["cap_all"], reserve).astype(np.uint32)
            pick[rows], score[rows], rank[rows], ld, _ = plain.resolve(L[rows], T[rows], P, cap_b, 0, SHED, ld)   # (SHED: the finish takes no room)
    ld = ld.astype(np.int64)
    valid = (L >= 0) & (L < P)
    for r in np.nonzero((rank == ref.RANK_OVERFLOW) & (band < len(bands)))[0]:
        if bands[band[r]][0] == SPILL:
            f = int(np.argmax(valid[r]))
            pick[r], score[r], rank[r] = L[r, f], T[r, f], ref.RANK_OVERFLOW | f
            ld[L[r, f]] += 1
    return pick, score, rank, (ld & 0xFFFFFFFF).astype(np.uint32), cases.want(c)[4]


def test_one_finish_behind_the_last_band_equals_a_finish_per_band(generated):
    chunk, cs = generated
    for c in cs:
        _same(_deferred(c), cases.want(c), cases.info(c))
    rng = np.random.default_rng(0x1DE7 + chunk)
    for i in range(200):                                               # mixed policies, monotone reserves, tight caps
        P, n, k, nb = int(rng.integers(1, 9)), int(rng.integers(1, 120)), int(rng.integers(1, 5)), int(rng.integers(1, 9))
        caps = rng.integers(0, 2 * max(1, n // P) + 2, size=P)
        c = cases._case(f"seeded-{i}", [], cases.bc._random_lists(rng, n, k, P, p_no=0.15), P, cases._table(rng, nb, int(caps.max())),
                        rng.integers(0, nb, size=n), cap=caps, load=rng.integers(0, 4, size=P), seed=i)
        _same(_deferred(c), cases.want(c), cases.info(c))
        _same(naive(c), cases.want(c), cases.info(c))


def test_the_generator_covers_what_it_has_to(generated):
    chunk, cs = generated
    tags = set().union(*(c["tags"] for c in cs))
    assert not set(cases.REQUIRED) - tags, sorted(set(cases.REQUIRED) - tags)
    assert len({c["name"] for c in cs}) == len(cs)
    assert max(c["lists"].shape[0] for c in cs) <= 4 * chunk + 100
    for c in cs:
        ref.check_table(c["bands"])
        n = c["lists"].shape[0]
        assert c["band"] is None or c["band"].shape == (n,)
        for t in c["tags"]:
            if t.startswith("one-launch-"):
                assert n <= chunk
            if t.startswith("chunked-"):
                assert n > chunk
    assert any(not cases.host_ok(c) for c in cs)


def test_where_the_order_matters_the_plain_resolve_answers_otherwise(generated):
    """A device that ignored the band bytes would give the plain resolve's picks: the GPU tests cannot pass on it."""
    chunk, cs = generated
    marked = [c for c in cs if "order-matters" in c["tags"]]
    assert len(marked) >= 2
    for c in marked:
        want = cases.want(c)[0]
        for policy in (SHED, SPILL):
            batch_order = plain.resolve(c["lists"], c["scores"], c["n_pods"], c["cap"], c["cap_all"], policy, c["load"])[0]
            assert not np.array_equal(want, batch_order), cases.info(c)


def test_under_shed_no_pod_ends_above_the_cap_of_the_last_band_that_placed_on_it(generated):
    chunk, cs = generated
    checked = 0
    for c in cs:
        if not cases.host_ok(c):
            continue
        bands = [(SHED, r) for _, r in c["bands"]]
        P = c["n_pods"]
        load_in = np.zeros(P, dtype=np.int64) if c["load"] is None else c["load"].astype(np.int64)
        pick, _, _, load, _ = ref.resolve(c["lists"], c["scores"], P, bands, c["band"], c["cap"], c["cap_all"], load_in.astype(np.uint32))
        band = np.zeros(pick.size, dtype=np.uint8) if c["band"] is None else c["band"]
        for p in np.unique(pick[pick >= 0]):
            last = int(band[pick == p].max())
            cap_b = int(ref.band_caps(P, c["cap"], c["cap_all"], bands[last][1])[p])
            assert int(load[p]) <= max(cap_b, int(load_in[p])), (cases.info(c), int(p))
            checked += 1
        assert np.array_equal(load.astype(np.int64), load_in + np.bincount(pick[pick >= 0], minlength=P))
    assert checked > 100


def test_tables_the_entry_points_refuse():
    for bad in ([], [(SHED, 0)] * 9, [(2, 0)], [(SHED, 3), (SHED, 2)]):
        with pytest.raises(AssertionError):
            ref.check_table(bad)
    ref.check_table([(SPILL, 0), (SHED, 0), (SHED, 7)])


def test_symbols_header_and_binding_agree_on_the_new_names():
    with open(os.path.join(ROOT, "include", "eppk.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    with open(os.path.join(ROOT, "gateway-api-inference-extension_amd", "_lib.py")) as f:
        src = f.read()
    syms = set(re.findall(r'"(eppk_[a-z0-9_]+)"', re.search(r"SYMBOLS = \[(.*?)\]", src, re.S).group(1)))
    new = {"eppk_banded_resolve_device", "eppk_pick_banded_device", "eppk_pick_banded", "eppk_group_pick_banded"}
    declared = set(re.findall(r"\b(eppk_[a-z0-9_]+)\s*\(", hdr))
    assert {s for s in declared if "banded" in s} == {s for s in syms if "banded" in s} == new
    for name in new:
        assert re.search(r"lib\.%s\.argtypes = \[" % name, src), f"{name} has no argtypes"
    assert re.search(r"#define EPPK_MAX_BANDS 8u", hdr) and re.search(r"^EPPK_MAX_BANDS = 8$", src, re.M)
    assert re.search(r"#define EPPK_ABI_VERSION 4u\b", hdr), "additive: the ABI version stays"
