"""GPU: chain totals of listed pods (SEMANTICS.md §3l; include/eppk.h eppk_score_lists, eppk_pick_rendezvous_scored) against the oracle's
score_row, bit for bit (scores as uint64).  Rows, index and lists are those of tests/test_gpu_prefix_costs.py (block counts on both sides of
every group width, misses, listed / full / overflowed / all-pod sets, the reserved hashes, a hole, ids out of range, a pod twice); on top
of them adapters -1 / 0 / 127 and gauges with ONE pod at the queue minimum and ONE at the maximum, so that a mask row can drop either."""
import bounded_ref as bref
import numpy as np
import pytest
from test_gpu_prefix_costs import HOLE, build, walk

pytestmark = pytest.mark.gpu
U64 = np.uint64
SORT, WITHIN = 1, 2
CHAIN = ((1, 3), (2, 2), (3, 1), (4, 4))                 # QUEUE x 3, KV x 2, LORA x 1, PREFIX x 4
NEG = ((4, -2), (1, 3), (2, 1))                           # a negative weight in front: totals pass through -0.0
QMIN_POD, QMAX_POD = 63, 1                                # both are in the lists' pool
_refs = {}


def setup(pkg, orc, P, B, chain=CHAIN, **kw):
    """build()'s picker with gauges and adapters; the oracle's index of the same pairs (made once per shape)."""
    pk, model, reqs, lists, pods = build(pkg, P, B, chain=chain, **kw)
    rng = np.random.default_rng(P + B)
    pods["queue"] = rng.integers(5, 50, P)
    pods["queue"][[QMIN_POD, QMAX_POD]] = [1, 99]
    pods["kv_util"] = rng.random(P)
    pods["max_lora"], pods["running"] = 4, rng.integers(0, 9, P)
    pods["active"] = rng.integers(0, 2 ** 63, (P, 2)).astype(U64) & rng.integers(0, 2 ** 63, (P, 2)).astype(U64)
    pods["waiting"] = rng.integers(0, 2 ** 63, (P, 2)).astype(U64) & rng.integers(0, 2 ** 63, (P, 2)).astype(U64)
    reqs[:, 0] = (reqs[:, 0] & U64(0xFFFFFFFF00000000)) | np.array([0xFFFFFFFF, 0, 127], dtype=U64)[np.arange(len(reqs)) % 3]
    pk.publish(pods)
    key = ("index", P, B, kw.get("R_min", 0))
    if kw.get("slots", 1) and key not in _refs:
        _refs[key] = orc.OracleIndex()
        for h, s in model.items():
            _refs[key].insert([h] * len(s), sorted(s))
    return pk, _refs.get(key) if kw.get("slots", 1) else None, model, reqs, lists, pods


def pack(bits):
    R, P = bits.shape
    full = np.zeros((R, (P + 63) // 64 * 64), dtype=bool)
    full[:, :P] = bits
    return np.packbits(full.reshape(R, -1, 64), axis=2, bitorder="little").view("<u8").reshape(R, -1).astype(U64)


def mask_rows(R, P):
    """By r % 6: every pod; without the minimum pod; without the maximum pod; pod 64 alone; nobody; without the listed pod 0."""
    bits = np.ones((R, P), dtype=bool)
    bits[1::6, QMIN_POD] = bits[2::6, QMAX_POD] = bits[5::6, 0] = False
    bits[3::6] = bits[4::6] = False
    bits[3::6, 64] = True
    return bits


def reference(orc, chain, pods, oix, reqs, lists, mask=None, within=False):
    R, k = lists.shape
    pick, score = np.full((R, k), -1, dtype=np.int32), np.zeros((R, k))
    for r in range(R):
        m = None if mask is None else mask[r]
        if within:                                         # the list is the filter: a mask row with exactly the listed pods (that the mask admits)
            bits = np.zeros((1, len(pods)), dtype=bool)
            ok = lists[r][(lists[r] >= 0) & (lists[r] < len(pods))]
            bits[0, ok] = True
            m = pack(bits)[0] if m is None else pack(bits)[0] & m
        tot = orc.score_row(list(chain), pods, oix, reqs[r], m)
        for j, p in enumerate(lists[r]):
            if 0 <= p < len(pods) and not np.isnan(tot[p]):
                pick[r, j], score[r, j] = p, tot[p]
    return pick, score


def ordered(pick, score):
    """eppk_pick_topk's order: valid first, total descending, pod ascending, position ascending."""
    o = np.stack([sorted(range(pick.shape[1]), key=lambda j: (pick[r, j] < 0, -score[r, j], pick[r, j], j)) for r in range(len(pick))])
    return np.take_along_axis(pick, o, 1), np.take_along_axis(score, o, 1)


def same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, "picks", np.argwhere(got[0] != want[0])[:4].tolist())
    bad = np.argwhere(got[1].view(U64) != want[1].view(U64))
    assert bad.size == 0, (what, "scores", bad[:4].tolist(), got[1][tuple(bad[0])], want[1][tuple(bad[0])])


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("P,B", [(200, 8), (2000, 70), (4096, 256)])
def test_totals(pkg, orc, P, B, k, masked):
    pk, oix, model, reqs, lists, pods = setup(pkg, orc, P, B)
    bits = mask_rows(len(reqs), P) if masked else None
    mask = pack(bits) if masked else None
    if (P, B, masked) not in _refs:
        _refs[P, B, masked] = reference(orc, CHAIN, pods, oix, reqs, lists, mask)
    cols = slice(0, 8) if k > 1 else slice(3, 4)
    want = tuple(np.ascontiguousarray(a[:, cols]) for a in _refs[P, B, masked])
    lists = np.ascontiguousarray(lists[:, cols])
    with pk:
        same(pk.score_lists(reqs, lists, 0, mask), want)
    nb = (reqs[:, 0] >> U64(32)).astype(np.int64)
    matched = walk(model, reqs, lists, P, {HOLE}, B)[1]
    assert np.any((matched > 0) & (matched < nb[:, None])) and np.any(want[0] >= 0) and np.any(want[0] < 0)
    if masked:                                             # both normaliser paths, and a listed active pod that the mask excludes
        both, some = bits[:, QMIN_POD] & bits[:, QMAX_POD], bits.any(axis=1)
        assert np.any(both[want[0].max(axis=1) >= 0]) and np.any((~both & some)[want[0].max(axis=1) >= 0])
        assert k == 1 or np.any((lists[5::6] == 0) & (want[0][5::6] < 0))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("k", [1, 4, 8])
def test_sort_restores_topk(pkg, orc, k, masked):
    import torch
    P, B = 200, 8
    pk, _, _, reqs, _, _ = setup(pkg, orc, P, B, chain=NEG)
    R = len(reqs)
    mask = pack(mask_rows(R, P)) if masked else None
    with pk:
        want = pk.pick_topk(reqs, k, mask)
        perm = np.random.default_rng(k).permuted(want[0], axis=1)
        assert masked == bool(np.any(want[0] < 0)) and (k == 1 or np.any(perm != want[0]))
        same(pk.score_lists(reqs, perm, SORT, mask), want, "host form")
        d_reqs, d_l = torch.from_numpy(reqs.view(np.int64)).cuda(), torch.from_numpy(perm).cuda()
        d_m = torch.from_numpy(mask.view(np.int64)).cuda() if masked else None
        d_s = torch.full((R, k), -7.0, dtype=torch.float64, device="cuda")
        pk.score_lists_device(d_reqs.data_ptr(), R, d_l.data_ptr(), k, SORT, d_l.data_ptr(), d_s.data_ptr(), d_m.data_ptr() if masked else None)
        torch.cuda.synchronize()
        assert pk.launch_status() == 0
        same((d_l.cpu().numpy(), d_s.cpu().numpy()), want, "device form, in place")


@pytest.mark.parametrize("masked", [False, True])
def test_within_list(pkg, orc, masked):
    P, B = 2000, 70
    pk, oix, _, reqs, lists, pods = setup(pkg, orc, P, B)
    lists[0] = [-1, P, HOLE, 70000, 7, -1, -1, -1]        # one valid pod: QUEUE score 1.0
    lists[1] = [-1, P, HOLE, 70000, -5, P + 1, -1, -1]    # none
    bits = mask_rows(len(reqs), P) if masked else np.ones((len(reqs), P), dtype=bool)
    mask = pack(bits) if masked else None
    want = reference(orc, CHAIN, pods, oix, reqs, lists, mask, within=True)
    listed = np.zeros_like(bits)
    for r, row in enumerate(lists):
        listed[r, row[(row >= 0) & (row < P)]] = True
    with pk:
        got = pk.score_lists(reqs, lists, WITHIN, mask)
        same(got, want)
        same(pk.score_lists(reqs, lists, WITHIN | SORT, mask), ordered(*want), "sorted")
        tp, ts = pk.pick_topk(reqs, 8, pack(listed & bits))
    assert want[0][0].tolist().count(7) == 1 and np.all(want[0][1] < 0)
    for r in range(len(reqs)):                             # every valid entry carries top-k's total under the list's own mask row
        for p, s in zip(got[0][r], got[1][r]):
            assert p < 0 or ts[r][tp[r] == p].view(U64).tolist() == [s.view(U64)], (r, p)


@pytest.mark.parametrize("chain,slots", [(CHAIN[:3], 1 << 16), (CHAIN, 0)])
def test_no_walk(pkg, orc, chain, slots, monkeypatch):
    P, B, got = 200, 8, {}
    for max_cu in ((None, "1") if slots == 0 else (None,)):
        if max_cu:
            monkeypatch.setenv("EPPK_MAX_CU", max_cu)
        pk, oix, _, reqs, lists, pods = setup(pkg, orc, P, B, chain=chain, slots=slots, R_min=1537 if slots == 0 else 0)
        mask = pack(mask_rows(len(reqs), P))
        with pk:
            got[max_cu] = pk.score_lists(reqs, lists, 0, mask), pk.score_lists(reqs, lists, SORT)
            g = pk.launch_geometry()
        assert g[:2] == (0, 0) and g[3] == 256 and (not max_cu or (1537 + 7) // 8 >= 3 * g[2] * 4), g
    want = reference(orc, chain, pods, oix, reqs, lists, mask), ordered(*reference(orc, chain, pods, oix, reqs, lists))
    for max_cu, (a, b) in got.items():
        same(a, want[0], max_cu)
        same(b, want[1], max_cu)
    assert slots != 0 or len(reqs) == 1537


def test_bad_row_and_refusals(pkg, orc):
    import torch
    P, B, k = 200, 8, 8
    pk, oix, _, reqs, lists, pods = setup(pkg, orc, P, B)
    R = len(reqs)
    want = reference(orc, CHAIN, pods, oix, reqs, lists)
    picks, scores = np.zeros((R, k), dtype=np.int32), np.zeros((R, k))
    with pkg.BatchedPicker(list(CHAIN), max_pods=P, max_blocks=B, max_batch=64) as fresh:
        call = lambda p, n, kk, fl, ls, op, os: p._lib.eppk_score_lists(p._ctx, reqs.ctypes.data, n, None, ls, kk, fl, op, os)      # noqa: E731
        assert call(fresh, R, k, 0, lists.ctypes.data, picks.ctypes.data, scores.ctypes.data) == -4                      # no snapshot
    with pk:
        args = (lists.ctypes.data, picks.ctypes.data, scores.ctypes.data)
        assert [call(pk, R, kk, fl, *args) for kk, fl in ((0, 0), (9, 0), (k, 4), (k, 0x80000001))] == [-1] * 4
        assert call(pk, R, k, 0, None, *args[1:]) == call(pk, R, k, SORT, args[0], None, args[2]) == call(pk, R, k, 0, *args[:2], None) == -1
        assert call(pk, pk.max_batch + 1, k, 0, *args) == -2
        assert call(pk, R, k, 0, args[0], None, args[2]) == 0 and call(pk, R, k, SORT, *args[:2], None) == 0           # the nullable outputs
        reqs[3, 0] = (U64(B + 5) << U64(32)) | U64(0xFFFFFFFF)
        reqs[7, 0] = (U64(2) << U64(32)) | U64(128)
        with pytest.raises(pkg.EppkError) as e:
            pk.score_lists(reqs, lists)
        assert e.value.code == -1 and "row 3" in str(e.value) and pk.launch_status() == 0
        d_reqs, d_l = torch.from_numpy(reqs.view(np.int64)).cuda(), torch.from_numpy(lists).cuda()
        d_p, d_s = torch.full((R, k), -7, dtype=torch.int32, device="cuda"), torch.full((R, k), -7.0, dtype=torch.float64, device="cuda")
        stride = reqs.shape[1] * 8
        rc = pk._lib.eppk_score_lists_device(pk._ctx, d_reqs.data_ptr(), 2 ** 31 // stride + 1, None, d_l.data_ptr(), k, 0, d_p.data_ptr(), d_s.data_ptr(), None)
        assert rc == -2 and pk.launch_status() == 0
        pk.score_lists_device(d_reqs.data_ptr(), R, d_l.data_ptr(), k, 0, d_p.data_ptr(), d_s.data_ptr())
        torch.cuda.synchronize()
        assert pk.launch_status() == 1                     # EPPK_LAUNCH_BAD_REQUEST_ROW
    want[0][[3, 7]], want[1][[3, 7]] = -1, 0.0
    same((d_p.cpu().numpy(), d_s.cpu().numpy()), want)


@pytest.mark.parametrize("form", ["session", "prefix"])
def test_pick_form(pkg, orc, form):
    import torch
    P, B, k, seed = 200, 8, 4, 11
    pk, oix, _, reqs, _, pods = setup(pkg, orc, P, B, R_min=300)
    R = len(reqs)
    key = np.random.default_rng(5).integers(0, 2 ** 64, R, dtype=U64) if form == "session" else None
    depth = 0 if form == "session" else 2
    with pk:
        rdv = pk.pick_rendezvous(reqs, k, seed, key=key, depth=depth)[0]
        want = ordered(*reference(orc, CHAIN, pods, oix, reqs, rdv))
        assert np.any(want[0][:, 0] != rdv[:, 0])          # somewhere hash rank 0 is not the chain's choice: the order is not rendezvous's
        same(pk.score_lists(reqs, rdv, SORT), want, "score_lists")
        same(pk.pick_rendezvous_scored(reqs, k, seed, key=key, depth=depth), want, "host form")
        d = {n: torch.zeros(sz, dtype=t, device="cuda") for n, sz, t in [("lists", R * k, torch.int32), ("ls", R * k, torch.float64), ("pick", R, torch.int32),
                                                                         ("score", R, torch.float64), ("rank", R, torch.uint8), ("load", P, torch.int32)]}
        d_reqs = torch.from_numpy(reqs.view(np.int64)).cuda()
        d_key = torch.from_numpy(key.view(np.int64)).cuda() if key is not None else None
        cap = int(1.25 * R / P) + 1
        pk.pick_rendezvous_scored_device(d_reqs.data_ptr(), R, k, seed, 0, d["lists"].data_ptr(), d["ls"].data_ptr(),
                                         d_key=d_key.data_ptr() if key is not None else None, depth=depth)
        pk.bounded_resolve_device(d["lists"].data_ptr(), d["ls"].data_ptr(), R, k, None, cap, bref.SPILL, d["load"].data_ptr(), d["pick"].data_ptr(),
                                  d["score"].data_ptr(), d["rank"].data_ptr())
        torch.cuda.synchronize()
        assert pk.launch_status() == 0
    out = {n: t.cpu().numpy() for n, t in d.items()}
    same((out["lists"].reshape(R, k), out["ls"].reshape(R, k)), want, "device form")
    wp, ws, wr, wl, _ = bref.resolve(want[0], want[1], P, None, cap, bref.SPILL)
    assert np.array_equal(out["pick"], wp) and np.array_equal(out["rank"], wr) and np.array_equal(out["load"].view(np.uint32), wl)
    assert np.array_equal(out["score"].view(U64), ws.view(U64)) and np.any(wr > 0)
