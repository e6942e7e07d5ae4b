"""GPU: the picker "weighted-random" (SEMANTICS.md §3c; include/eppk.h eppk_pick_weighted_random) against its numpy restatement
(tests/wrand_ref.py) on the oracle's totals, bit for bit: picks, and scores compared as uint64."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q, KV, L, PF = 1, 2, 3, 4
BASE = [(Q, 2), (KV, 2), (L, 1), (PF, 3)]           # BASELINE's full chain
DECODE = [(PF, 3), (KV, 5)]                          # example.yaml's decode profile
NEG = [(Q, 2), (KV, -3), (PF, 3)]                    # a negative weight: totals <= 0 occur
DUP = [(PF, 2), (Q, 1), (PF, 1)]                     # duplicated PREFIX: not a fused chain
SEEDS = (0, 0xDEADBEEFCAFEF00D)


@pytest.fixture(scope="module")
def ref():
    spec = importlib.util.spec_from_file_location("wrand_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "wrand_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _oracle_index(orc, wl):
    oix = orc.OracleIndex()
    oix.insert(wl.index_hashes, wl.index_pods)
    return oix


def _totals(orc, chain, pods, oix, reqs, mask=None):
    """[R, P] totals of the oracle (NaN = not a candidate)."""
    return np.stack([orc.score_row(chain, pods, oix, reqs[r], None if mask is None else mask[r]) for r in range(reqs.shape[0])])


def _holes(wl, frac, seed):
    rng = np.random.default_rng(seed)
    pods = wl.pods.copy()
    pods["flags"] = (rng.random(pods.shape[0]) < frac).astype(np.uint32)
    return pods


def _mixed_mask(wl, seed):
    """Rows by r % 4: 50 % of the pods, a subset of 1..8 pods, 50 % again, and every 37th row empty."""
    rng = np.random.default_rng(seed)
    R, P = wl.reqs.shape[0], wl.pods.shape[0]
    J = (P + 63) // 64
    bits = np.zeros((R, J * 64), dtype=bool)
    bits[:, :P] = rng.random((R, P)) < 0.5
    for r in range(1, R, 4):
        bits[r] = False
        bits[r, rng.choice(P, size=int(rng.integers(1, 9)), replace=False)] = True
    bits[::37] = False
    return np.packbits(bits.reshape(R, J, 64)[:, :, ::-1], axis=2).view(">u8").reshape(R, J).astype(np.uint64)


def _same(got, want, what):
    gp, gs = got
    wp, ws = want
    bad = np.nonzero(np.any(gp != wp, axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[:4]}: gpu {gp[bad[:2]]} ref {wp[bad[:2]]}"
    assert np.array_equal(gs.view(np.uint64), ws.view(np.uint64)), what


CASES = [(3, BASE), (3, DECODE), (3, NEG), (3, DUP), (2, BASE), (2, NEG), (4, BASE), (4, NEG)]
# the default library mode everywhere, EPPK_LISTS=0 (the prefix walk's dense route) on config 3, whose index holds the lists
RUNS = [(c, ch, "default") for c, ch in CASES] + [(c, ch, "lists0") for c, ch in CASES if c == 3]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("config,chain,lists", RUNS)
def test_matches_the_restatement(pkg, orc, ref, monkeypatch, config, chain, masked, lists):
    if lists == "lists0":
        monkeypatch.setenv("EPPK_LISTS", "0")
    wl = pkg.workload.make_workload(config, R=1536, B=None if config in (3, 5) else 8)
    pods = _holes(wl, 0.1, config)
    mask = _mixed_mask(wl, 100 + config) if masked else None
    oix = _oracle_index(orc, wl)
    T = _totals(orc, chain, pods, oix, wl.reqs, mask)
    with pkg.BatchedPicker(chain, max_pods=wl.pods.shape[0], max_blocks=wl.B, max_batch=wl.R, index_slots=wl.index_slots) as pk:
        pk.publish(pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        for k, seed in [(1, SEEDS[0]), (2, SEEDS[1]), (4, SEEDS[0]), (8, SEEDS[1])]:
            got = pk.pick_weighted_random(wl.reqs, seed, k, mask)
            want = ref.weighted_random(T, k, seed, np.arange(wl.R))
            _same(got, want, f"config {config} chain {chain} masked {masked} k {k} seed {seed:#x}")
            assert not np.any(pods["flags"][got[0][got[0] >= 0]] & 1)
        if masked:
            assert np.all(got[0][::37] == -1)


@pytest.fixture(scope="module")
def c5(pkg, orc):
    wl = pkg.workload.make_workload(5)
    return wl, _oracle_index(orc, wl)


def test_full_size_c5(pkg, orc, ref, c5):
    wl, oix = c5
    R, P = wl.reqs.shape[0], wl.pods.shape[0]
    with pkg.BatchedPicker(wl.chain, max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots) as pk:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        picks, scores = pk.pick_weighted_random(wl.reqs, 7, 1)
        p4, s4 = pk.pick_weighted_random(wl.reqs, 8, 4)
    rows = np.unique(np.concatenate([np.linspace(0, R - 1, 1000).astype(np.int64), np.arange(R - 24, R)]))
    T = _totals(orc, wl.chain, wl.pods, oix, wl.reqs[rows])
    _same((picks[rows], scores[rows]), ref.weighted_random(T, 1, 7, rows), "C5 k 1")
    _same((p4[rows], s4[rows]), ref.weighted_random(T, 4, 8, rows), "C5 k 4")
    # every row: the pick is a pod and its score is that pod's total
    assert np.all((picks[:, 0] >= 0) & (picks[:, 0] < P))
    for r in range(R):
        t = orc.score_row(wl.chain, wl.pods, oix, wl.reqs[r])
        assert scores[r, 0] == t[picks[r, 0]], r


def _chi2_z(counts, expect):
    """(chi^2 - df) / sqrt(2 df) with bins merged (ascending expectation) until each expects at least 5."""
    order = np.argsort(expect)
    oc, oe, acc_c, acc_e = [], [], 0.0, 0.0
    for i in order:
        acc_c += counts[i]
        acc_e += expect[i]
        if acc_e >= 5:
            oc.append(acc_c); oe.append(acc_e)
            acc_c = acc_e = 0.0
    if acc_e > 0 and oe:
        oc[-1] += acc_c
        oe[-1] += acc_e
    oc, oe = np.array(oc), np.array(oe)
    df = oc.size - 1
    return (float(((oc - oe) ** 2 / oe).sum()) - df) / np.sqrt(2 * df)


def test_distribution_of_one_repeated_row(pkg, orc, c5):
    wl, oix = c5
    R, P = 65536, wl.pods.shape[0]
    row = 12345
    reqs = np.ascontiguousarray(np.broadcast_to(wl.reqs[row], (R, wl.reqs.shape[1])))
    t = orc.score_row(wl.chain, wl.pods, oix, wl.reqs[row])
    w = np.where(t > 0, t, 0.0)
    allneg = [(Q, -1), (KV, -2)]
    with pkg.BatchedPicker(wl.chain, max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots) as pk:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        p1, s1 = pk.pick_weighted_random(reqs, 99, 1)
        p2, _ = pk.pick_weighted_random(reqs, 100, 2)
    assert np.all(w[p1[:, 0]] > 0)
    assert np.array_equal(s1[:, 0].view(np.uint64), t[p1[:, 0]].view(np.uint64))
    z = _chi2_z(np.bincount(p1[:, 0], minlength=P).astype(np.float64), R * w / w.sum())
    assert z < 6, z
    assert np.all(p2[:, 0] != p2[:, 1]) and np.all(p2 >= 0)
    with pkg.BatchedPicker(allneg, max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots) as pk:
        pk.publish(wl.pods)
        pn, sn = pk.pick_weighted_random(reqs, 5, 1)
    tn = orc.score_row(allneg, wl.pods, None, wl.reqs[row])
    assert np.all(tn <= 0)
    assert np.array_equal(sn[:, 0].view(np.uint64), tn[pn[:, 0]].view(np.uint64))
    z = _chi2_z(np.bincount(pn[:, 0], minlength=P).astype(np.float64), np.full(P, R / P))
    assert z < 6, z


def test_device_entry_point_on_a_stream_with_assumed_load(pkg, orc, ref):
    import torch
    wl = pkg.workload.make_workload(3, R=2000, P=700)
    E, k, seed = 4, 2, 0x1234
    oix = _oracle_index(orc, wl)
    with pkg.BatchedPicker(wl.chain, max_pods=1024, max_blocks=wl.B, max_batch=wl.R, index_slots=wl.index_slots) as pk:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        pk.set_assumed_load(E)
        st = torch.cuda.Stream()
        d_reqs = torch.from_numpy(wl.reqs.view(np.int64)).cuda()
        d_pick = torch.full((wl.R * k,), -7, dtype=torch.int32, device="cuda")
        d_score = torch.full((wl.R * k,), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            pk.pick_weighted_random_device(d_reqs.data_ptr(), wl.R, None, k, seed, d_pick.data_ptr(), d_score.data_ptr(), st.cuda_stream)
        st.synchronize()
        picks = d_pick.cpu().numpy().reshape(wl.R, k)
        scores = d_score.cpu().numpy().reshape(wl.R, k)
    pods = wl.pods.copy()
    per = (wl.R + E - 1) // E
    wp = np.full((wl.R, k), -1, dtype=np.int32)
    ws = np.zeros((wl.R, k))
    for lo in range(0, wl.R, per):
        hi = min(wl.R, lo + per)
        T = _totals(orc, wl.chain, pods, oix, wl.reqs[lo:hi])
        wp[lo:hi], ws[lo:hi] = ref.weighted_random(T, k, seed, np.arange(lo, hi))
        for p in wp[lo:hi, 0]:
            if p >= 0:
                pods["queue"][p] += 1
    _same((picks, scores), (wp, ws), "assumed load E = 4, device form")


@pytest.mark.parametrize("E", [1, 3, "R"])
def test_assumed_load_epochs_on_masked_rows_with_a_leading_queue(pkg, orc, ref, E):
    """Epochs of R, R/3 and one request with candidate masks and k = 2 on a chain that STARTS with QUEUE: between epochs the snapshot's
    queue gauges, the QUEUE range and with them the staged leading terms are rebuilt, and the word of request r hashes its index in
    the batch, not in its epoch.  Coarse queue gauges (0..2): one assumed request moves the range.  The numpy side is the loop of
    test_device_entry_point_on_a_stream_with_assumed_load: bump queue[round 0's pick] after every epoch."""
    chain = [(Q, 3), (KV, 1), (PF, 2), (Q, -1)]
    wl = pkg.workload.make_workload(3, R=60, P=300, B=8)
    R, k, seed = wl.R, 2, 0xF00D0000F00D
    E = R if E == "R" else E
    pods = wl.pods.copy()
    pods["queue"] = np.random.default_rng(5).integers(0, 3, pods.shape[0])
    mask = _mixed_mask(wl, 321)
    oix = _oracle_index(orc, wl)
    with pkg.BatchedPicker(chain, max_pods=300, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots) as pk:
        pk.publish(pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        pk.set_assumed_load(E)
        got = pk.pick_weighted_random(wl.reqs, seed, k, mask)
    per = (R + E - 1) // E
    wp = np.full((R, k), -1, dtype=np.int32)
    ws = np.zeros((R, k))
    for lo in range(0, R, per):
        hi = min(R, lo + per)
        T = _totals(orc, chain, pods, oix, wl.reqs[lo:hi], mask[lo:hi])
        wp[lo:hi], ws[lo:hi] = ref.weighted_random(T, k, seed, np.arange(lo, hi))
        for p in wp[lo:hi, 0]:
            if p >= 0:
                pods["queue"][p] += 1
    _same(got, (wp, ws), f"assumed load E = {E}, masked, k = 2, leading QUEUE")
    assert np.any(wp[:, 0] < 0) and np.any(wp[:, 1] < 0) and np.any(wp[:, 1] >= 0)     # empty rows, padded rows, full rows


def test_errors_and_bad_rows(pkg):
    import torch
    wl = pkg.workload.make_workload(3, R=300, P=500)
    with pkg.BatchedPicker(wl.chain, max_pods=512, max_blocks=wl.B, max_batch=wl.R, index_slots=wl.index_slots) as pk:
        picks = np.zeros(wl.R * 9, dtype=np.int32)
        scores = np.zeros(wl.R * 9)
        args = lambda n, k: (pk._ctx, wl.reqs.ctypes.data, n, None, k, 1, picks.ctypes.data, scores.ctypes.data)
        assert pk._lib.eppk_pick_weighted_random(*args(wl.R, 1)) == -4         # EPPK_ERR_NO_SNAPSHOT
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        assert pk._lib.eppk_pick_weighted_random(*args(wl.R, 0)) == -1         # EPPK_ERR_ARG: k out of range
        assert pk._lib.eppk_pick_weighted_random(*args(wl.R, 9)) == -1
        assert pk._lib.eppk_pick_weighted_random(*args(wl.R + 1, 1)) == -2     # EPPK_ERR_LIMIT: more than max_batch
        bad = wl.reqs.copy()
        bad[17, 0] = (np.uint64(wl.B + 5) << np.uint64(32)) | (bad[17, 0] & np.uint64(0xFFFFFFFF))   # n_blocks > max_blocks
        with pytest.raises(pkg.EppkError) as e:
            pk.pick_weighted_random(bad, 1, 2)
        assert e.value.code == -1
        k = 3
        d_reqs = torch.from_numpy(bad.view(np.int64)).cuda()
        d_pick = torch.full((wl.R * k,), -7, dtype=torch.int32, device="cuda")
        d_score = torch.full((wl.R * k,), -7.0, dtype=torch.float64, device="cuda")
        assert pk.launch_status() == 0
        pk.pick_weighted_random_device(d_reqs.data_ptr(), wl.R, None, k, 2, d_pick.data_ptr(), d_score.data_ptr())
        assert pk.launch_status() == 1                                          # EPPK_LAUNCH_BAD_REQUEST_ROW
        gp = d_pick.cpu().numpy().reshape(wl.R, k)
        gs = d_score.cpu().numpy().reshape(wl.R, k)
        assert np.all(gp[17] == -1) and np.all(gs[17] == 0.0)
        hp, hs = pk.pick_weighted_random(wl.reqs, 2, k)
        good = np.arange(wl.R) != 17
        assert np.array_equal(gp[good], hp[good]) and np.array_equal(gs[good].view(np.uint64), hs[good].view(np.uint64))


@pytest.mark.parametrize("members", [2, 3])
@pytest.mark.parametrize("masked", [False, True])
def test_device_group_equals_one_context(pkg, members, masked):
    wl = pkg.workload.make_workload(3, R=1500, P=900, masked=masked)
    with pkg.BatchedPicker(wl.chain, max_pods=1024, max_blocks=wl.B, max_batch=wl.R, index_slots=wl.index_slots) as pk:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        one = [pk.pick_weighted_random(wl.reqs, 31, k, wl.mask) for k in (1, 4)]
    with pkg.DeviceGroup(wl.chain, [0] * members, max_pods=1024, max_blocks=wl.B, max_batch=wl.R, index_slots=wl.index_slots,
                         min_shard=64) as g:
        g.publish(wl.pods)
        g.index_insert(wl.index_hashes, wl.index_pods)
        grp = [g.pick_weighted_random(wl.reqs, 31, k, wl.mask) for k in (1, 4)]
    for (a, b), (c, d) in zip(one, grp):
        assert np.array_equal(a, c)
        assert np.array_equal(b.view(np.uint64), d.view(np.uint64))
