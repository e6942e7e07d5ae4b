"""eppk_index_export / eppk_index_import against a plain dict {hash: (pods, stamp)} kept beside the calls (SEMANTICS.md §6d).

Exports are compared as SORTED triples (the order follows placement, which follows history); only the determinism and `cap` checks
look at the raw order.  Everything is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHAIN = [(1, 1), (2, 2), (3, 1), (4, 4)]
B = 4
ONES = 0xFFFFFFFFFFFFFFFF
ERR_ARG, ERR_LIMIT, EXPORT_TRUNCATED = -1, -2, 16


class Mirror:
    """A picker and the dict; every index call the tests make goes through here."""

    def __init__(self, pkg, P, index_slots, seed=7):
        self.pk = pkg.BatchedPicker(CHAIN, max_pods=P, max_blocks=B, max_batch=4096, index_slots=index_slots)
        self.pods = pkg.workload.make_pods(seed, P, 128)
        self.pk.publish(self.pods)
        self.d, self.epoch = {}, 1

    def insert(self, sets):
        h = np.array([k for k, ps in sets.items() for _ in ps], dtype=np.uint64)
        p = np.array([q for ps in sets.values() for q in ps], dtype=np.uint32)
        self.pk.index_insert(h, p)
        for k, ps in sets.items():
            self.d[k] = (self.d.get(k, (set(), 0))[0] | set(ps), self.epoch)

    def tick(self, n=1):
        for _ in range(n):
            self.epoch = self.pk.index_advance_epoch()
        self.d = {k: v for k, v in self.d.items() if v[1] >= self.epoch - 254}

    def evict_older(self, e):
        self.pk.index_evict_older(e)
        self.d = {k: v for k, v in self.d.items() if v[1] >= e}

    def forget(self, pod, hole=False):
        if hole:                                                    # publishing the slot as a hole scrubs it (§6b)
            self.pods["flags"][pod] |= 1
            self.pk.publish(self.pods)
        else:
            self.pk.index_remove_pod(pod)
        self.d = {k: (v[0] - {pod}, v[1]) for k, v in self.d.items() if v[0] - {pod}}

    def want(self):
        return sorted((k, p, self.epoch - s) for k, (ps, s) in self.d.items() for p in ps)

    def check(self, what):
        h, p, a = self.pk.index_export()
        assert sorted(zip(h.tolist(), p.tolist(), a.tolist())) == self.want(), what
        h2, p2, a2 = self.pk.index_export()
        assert h.tobytes() == h2.tobytes() and p.tobytes() == p2.tobytes() and a.tobytes() == a2.tobytes(), f"{what}: two exports differ"
        assert self.pk.index_selfcheck() == 0, what
        return h, p, a


def fresh(rng, n):
    return [int(x) for x in rng.integers(1, 1 << 63, n, dtype=np.uint64)]


def shapes(m, P, rng, n_live=32):
    """Every set shape in one index of n_live hashes: single pods (hash 0 among them), 2, exactly 24 (list full), 25 and P pods (dense
    rows; ~0 has one), and a dense set of 30 cut back to 24 by six removals (returns to its list)."""
    two, full, d25, dall, back = fresh(rng, 5)
    m.insert({0: [5], ONES: range(8, 33), two: [1, P - 1], full: range(24), d25: range(10, 35), dall: range(P), back: range(40, 70)})
    m.insert({h: [int(rng.integers(0, 64))] for h in fresh(rng, n_live - 7)})
    for pod in range(64, 70):
        m.forget(pod)
    assert len(m.d[back][0]) == 24 and len(m.d) == n_live


@pytest.mark.parametrize("P", [96, 2048, 4096])                       # the three lane-word types
def test_set_shapes_in_a_full_table_then_with_tombstones(pkg, P):
    rng = np.random.default_rng(P)
    m = Mirror(pkg, P, 64)
    with m.pk:
        shapes(m, P, rng)                                           # 32 live hashes: the limit of index_slots = 64, keys displaced
        m.check("full table")
        m.tick()
        keep = list(m.d)[::2]
        m.insert({h: [min(m.d[h][0])] for h in keep})               # restamped: they stay
        m.evict_older(m.epoch)
        assert len(m.d) == 16
        m.insert({h: [int(rng.integers(0, P)), 2] for h in fresh(rng, 16)})
        m.check("tombstones between live keys")
        m.forget(2, hole=True)
        m.check("a hole")


def test_every_age_of_the_window(pkg):
    rng = np.random.default_rng(1)
    m = Mirror(pkg, 96, 64)
    with m.pk:
        a, b, c, d, e, f = fresh(rng, 6)
        m.insert({a: [1], 0: [2, 3]})
        for ticks, sets in ((1, {b: range(30), ONES: [4]}), (189, {c: [5]}), (1, {d: [6, 7]}), (62, {e: [8]}), (1, {f: [9]})):
            m.tick(ticks)
            m.insert(sets)
        ages = m.check("ages")[2]
        assert set(ages.tolist()) == {0, 1, 63, 64, 253, 254}        # 64: past the trim's cap; 254: the last age a tag expresses
        m.tick()
        assert a not in m.d and 0 not in m.d
        assert 254 in m.check("one tick later")[2].tolist()


@pytest.mark.parametrize("max_cu", [None, "1"])
def test_sparse_table_many_trips(pkg, monkeypatch, max_cu):
    if max_cu:
        monkeypatch.setenv("EPPK_MAX_CU", max_cu)
    rng = np.random.default_rng(3)
    m = Mirror(pkg, 2048, 65536)                                     # 2049 tiles: three runs of the scan, the last of one tile
    with m.pk:
        m.insert({h: rng.choice(2048, int(rng.integers(1, 4)), replace=False).tolist() for h in fresh(rng, 3000)})
        m.insert({h: rng.choice(2048, 700, replace=False).tolist() for h in fresh(rng, 3)} | {ONES: [0, 2047]})
        m.tick(2)
        m.insert({h: [7] for h in list(m.d)[::3]})
        m.check("sparse")


def raw_export(pk, cap, fill=0xA5):
    """eppk_index_export into sentinel-filled arrays of cap + 1 entries -> (rc, total, hashes, pods, ages)."""
    h, p, a = np.full(cap + 1, fill, np.uint64), np.full(cap + 1, fill, np.uint32), np.full(cap + 1, fill, np.uint8)
    n = np.zeros(1, np.uint64)
    rc = pk._lib.eppk_index_export(pk._ctx, h.ctypes.data if cap else None, p.ctypes.data if cap else None, a.ctypes.data if cap else None, cap, n.ctypes.data_as(pk._lib.eppk_index_export.argtypes[5]))
    return rc, int(n[0]), h, p, a


def test_cap(pkg):
    import torch
    m = Mirror(pkg, 96, 64)
    with m.pk as pk:
        assert raw_export(pk, 0)[:2] == (0, 0) and raw_export(pk, 3)[:2] == (0, 0)      # an empty index
        shapes(m, 96, np.random.default_rng(4))
        total = len(m.want())
        assert raw_export(pk, 0)[:2] == (0, total)                                     # the count query
        rc, n, h, p, a = raw_export(pk, total)
        assert (rc, n) == (0, total) and (h[total], p[total], a[total]) == (0xA5, 0xA5, 0xA5)
        rc, n, h1, p1, a1 = raw_export(pk, total - 1)
        assert (rc, n) == (ERR_LIMIT, total)
        for got, full in ((h1, h), (p1, p), (a1, a)):
            assert np.array_equal(got[:total - 1], full[:total - 1]) and got[total - 1] == 0xA5
        # the device form: the same bytes, the slot behind them untouched, the sticky flag
        dh, dp, da = torch.full((total,), 0xA5, dtype=torch.int64, device="cuda"), torch.full((total,), 0xA5, dtype=torch.int32, device="cuda"), torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
        dn = torch.zeros(1, dtype=torch.int64, device="cuda")
        assert pk.launch_status() == 0
        assert pk._lib.eppk_index_export_device(pk._ctx, dh.data_ptr(), dp.data_ptr(), da.data_ptr(), total - 1, dn.data_ptr(), None) == 0
        assert pk.launch_status() == EXPORT_TRUNCATED and int(dn.item()) == total
        for got, full in ((dh, h), (dp, p), (da, a)):
            got = got.cpu().numpy().view(full.dtype)
            assert np.array_equal(got[:total - 1], full[:total - 1]) and got[total - 1] == 0xA5
    with pkg.BatchedPicker(CHAIN, max_pods=96, max_blocks=B, max_batch=64, index_slots=0) as pk0:
        assert raw_export(pk0, 0)[:2] == (0, 0) and raw_export(pk0, 3)[:2] == (0, 0)


def test_round_trip_into_another_table(pkg):
    rng = np.random.default_rng(5)
    P = 2048
    ma, mb = Mirror(pkg, P, 64), Mirror(pkg, P, 1024)
    with ma.pk as A, mb.pk as Bk:
        shapes(ma, P, rng, n_live=24)
        ma.tick(3)
        ma.insert({h: [11, 12] for h in fresh(rng, 4)} | {0: [6]})
        ma.tick(64)
        ma.insert({h: [13] for h in fresh(rng, 4)})
        h, p, a = ma.check("source")
        assert Bk.index_import(h, p, a) == 1 + int(a.max()) and int(a.max()) == 67
        mb.d, mb.epoch = {k: (set(v[0]), v[1] - ma.epoch + 68) for k, v in ma.d.items()}, 68
        mb.check("restored")
        # a batch that probes every exported hash: alone, and as the head of a chain of two
        hs = np.unique(h)
        rows = np.concatenate([np.stack([hs, hs]).T, np.stack([hs, np.roll(hs, 1)]).T])
        reqs = pkg.picker.make_req_rows(rng.integers(-1, 128, rows.shape[0]), np.repeat([1, 2], hs.size), rows, B)
        (pa, sa), (pb, sb) = A.pick_topk(reqs, 4), Bk.pick_topk(reqs, 4)
        assert np.array_equal(pa, pb) and np.array_equal(sa.view(np.uint64), sb.view(np.uint64))
        # one hash, two ages: refused in front of the first insert
        with pytest.raises(pkg._lib.EppkError) as e:
            Bk.index_import([int(hs[1]), 99, int(hs[1])], [1, 2, 3], [int(a[h == hs[1]][0]), 0, 200])
        assert e.value.code == ERR_ARG
        mb.check("after the refusal")
