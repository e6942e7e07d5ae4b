"""The placement planner of the displaced-key tests (tests/index_placement.py) held to its word, without a GPU: a restatement of where
index_insert_one puts a new key (index_placement.Table), applied to each plan's insert calls, finds every key exactly where the plan
says.  This is what keeps tests/test_gpu_displaced.py from silently testing nothing after a change of the bucket layout."""
import importlib.util
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ip = _load("index_placement")
gd = _load("test_gpu_displaced")


def test_the_restated_constants_are_the_kernels():
    """Bucket geometry and the hash multiplier, read out of the sources the planner restates."""
    with open(os.path.join(ROOT, "gateway-api-inference-extension_amd", "csrc", "eppk_kernels.hip.h")) as f:
        src = f.read()
    assert int(re.search(r"constexpr uint32_t kHomeMul = (0x[0-9A-Fa-f]+)u", src).group(1), 16) == ip.HOME_MUL
    k_bucket = int(re.search(r"constexpr uint32_t kBucket = (\d+)u", src).group(1))
    k_sub0 = int(re.search(r"constexpr uint32_t kKeySub0 = (\d+)u", src).group(1))
    assert k_bucket - k_sub0 == ip.KEYS_PER_BUCKET
    with open(os.path.join(ROOT, "gateway-api-inference-extension_amd", "csrc", "eppk.hip")) as f:
        host = f.read()
    assert "c->slots = cfg->index_slots * 2u;" in host          # physical words = 2 x index_slots -> index_slots / 4 buckets of kBucket words
    assert ip.n_buckets(1 << 10) == (1 << 10) * 2 // k_bucket


def test_home_bucket_by_hand():
    h = np.array([0x0123456789ABCDEF, 1, 0xFFFFFFFF00000000], dtype=np.uint64)
    for slots in (64, 1 << 17):
        lg = (slots // 4).bit_length() - 1
        want = [((((int(x) & 0xFFFFFFFF) ^ (int(x) >> 32)) * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - lg) for x in h]
        assert ip.home_bucket(h, slots).tolist() == want


def test_keys_for_buckets():
    slots = 1 << 12
    buckets, counts = [0, 5, 1023, 77], [7, 1, 12, 0]
    got = ip.keys_for_buckets(buckets, counts, slots, seed=3)
    again = ip.keys_for_buckets(buckets, counts, slots, seed=3)
    other = ip.keys_for_buckets(buckets, counts, slots, seed=4)
    allk = np.concatenate(got)
    assert np.unique(allk).size == allk.size == sum(counts)
    assert not np.any(allk == 0) and not np.any(allk == np.uint64(0xFFFFFFFFFFFFFFFF))
    for b, c, k, k2 in zip(buckets, counts, got, again):
        assert k.size == c and np.all(ip.home_bucket(k, slots) == b) and np.array_equal(k, k2)
    assert not np.array_equal(np.concatenate(other), allk)
    with pytest.raises(RuntimeError):
        ip.keys_for_buckets([3], [50], 1 << 20, seed=1, max_draws=1 << 20)     # cannot be built: raises, never returns fewer
    with pytest.raises(ValueError):
        ip.keys_for_buckets([3, 3], [1, 1], slots, seed=1)


def test_the_model_table_by_hand():
    """Six keys of one home bucket: five stay, the sixth flags the bucket and moves on; from the last bucket it wraps to bucket 0."""
    slots = 64                                                  # 16 buckets
    k = ip.keys_for_buckets([4, 15], [7, 6], slots, seed=9)
    t = ip.Table(slots)
    for h in k[0][:5].tolist():
        assert t.insert(h)[0] == 4
    assert 4 not in t.flags
    assert t.insert(int(k[0][5])) == (5, 0) and 4 in t.flags and 5 not in t.flags
    assert t.insert(int(k[0][5])) == (5, 0)                     # known key: where it is
    t.tombstone(int(k[0][1]))
    assert t.insert(int(k[0][6])) == (4, 1) and t.distance(int(k[0][5])) == 1      # a tombstone is a free word
    for h in k[1][:5].tolist():
        t.insert(h)
    assert t.insert(int(k[1][5])) == (0, 0) and t.distance(int(k[1][5])) == 1 and 15 in t.flags
    assert t.live() == 12 and t.non_empty_words() == 12


@pytest.mark.parametrize("which", ["main", "long"])
def test_every_plan_of_the_gpu_module_places_its_keys(which):
    chains, pl = gd.all_plans()[which]
    t = ip.verify(pl)                                           # distance 0 / 1 / 2 / wrapped per key, the buckets on the way full and flagged,
    assert t.live() < pl.index_slots // 2                       # absent keys absent behind the planned kind of home bucket, load limits
    assert t.non_empty_words() < 3 * ip.KEYS_PER_BUCKET * t.nb // 4
    assert t.live() == pl.n_keys()
    n_disp = {d: 0 for d in (ip.D1, ip.D2, ip.WRAP, ip.TOMB_D1, ip.ABSENT_OVF, ip.ABSENT)}
    for ch, keys, spec in zip(chains, pl.chains, pl.spec):
        assert ch.spec == spec and keys.size == len(spec)
        for h, how in zip(keys.tolist(), spec):
            if how in (ip.ABSENT, ip.ABSENT_OVF):
                assert h not in t.at and pl.absent[h] == (how == ip.ABSENT_OVF)
                n_disp[how] += 1
                continue
            d = t.distance(h)
            home = int(ip.home_bucket(np.uint64(h), pl.index_slots))
            if how == ip.HOME:
                assert d == 0
            elif how in (ip.D1, ip.TOMB_D1):
                assert d == 1 and home + 1 < t.nb
            elif how == ip.D2:
                assert d == 2 and home + 2 < t.nb
            else:
                assert home == t.nb - 1 and 1 <= d <= 64 and t.at[h][0] == d - 1
            if how != ip.HOME:
                n_disp[how] += 1
    assert all(n > 0 for n in n_disp.values()), n_disp          # every kind of placement occurs
    # fillers and chain keys are disjoint, and no filler is asked for by a request
    fill = set(pl.fillers.tolist()) | set(pl.tomb_fillers.tolist())
    asked = set(np.concatenate(pl.chains).tolist())
    assert not (fill & asked)
    # tombstoning the fillers of a TOMB_D1 key leaves its home bucket without a live key, still flagged, the key one bucket on
    for h in pl.tomb_fillers.tolist():
        t.tombstone(h)
    for keys, spec in zip(pl.chains, pl.spec):
        for h, how in zip(keys.tolist(), spec):
            if how == ip.TOMB_D1:
                home = int(ip.home_bucket(np.uint64(h), pl.index_slots))
                assert t.words[home] == [ip.TOMB] * ip.KEYS_PER_BUCKET and home in t.flags and t.distance(h) == 1


def test_a_plan_is_deterministic_for_its_seed():
    rows = [[ip.HOME, ip.D1, ip.D2, ip.WRAP, ip.ABSENT_OVF], [ip.TOMB_D1, ip.ABSENT, ip.WRAP]]
    a, b, c = ip.plan(rows, 1 << 10, 7), ip.plan(rows, 1 << 10, 7), ip.plan(rows, 1 << 10, 8)
    assert all(np.array_equal(x, y) for x, y in zip(a.chains, b.chains))
    assert [k for k, _ in a.calls] == [k for k, _ in b.calls] and all(np.array_equal(x[1], y[1]) for x, y in zip(a.calls, b.calls))
    assert not all(np.array_equal(x, y) for x, y in zip(a.chains, c.chains))
    ip.verify(a)
    with pytest.raises(RuntimeError):
        ip.plan([[ip.D2] * 32] * 4, 256, 1)                     # does not fit: raises


def test_the_row_layout_of_the_gpu_module():
    """Rows are scored four to a wavefront: the limit chains stand alone among rows that stop short at every g, and beside a 17-hit row."""
    cs, _ = gd.main_plan()
    rows = gd.layout(cs, gd.NBS, gd.B)
    assert len(rows) % 4 == 0
    alone = {}
    for r, (c, nb, lab) in enumerate(rows):
        if "alone@" in lab:
            others = [rows[q] for q in range(r - r % 4, r - r % 4 + 4) if q != r]
            assert all(o[2] == "short" and o[1] < 16 for o in others) and lab.endswith(f"@g{r % 4}")
            alone.setdefault(c, set()).add(r % 4)
        if "beside-m17" in lab:
            assert any(rows[q][0] == gd.M17 for q in range(r - r % 4, r - r % 4 + 4))
    lim = [c for c, ch in enumerate(cs) if ch.limit]
    assert lim and all(alone[c] == {0, 1, 2, 3} for c in lim)
    assert any(cs[c].name == "run{16,17}/d1" for c in lim)
