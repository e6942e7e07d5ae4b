"""GPU: the prefix-hit summary per request and the hybrid pick (SEMANTICS.md §3m; include/eppk.h eppk_prefix_summary, eppk_pick_hybrid)
against a dict hash -> set(pods) filled by the same index calls and the §3 walk written out below; everything exact (scores as uint64)."""
import index_placement as ip
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U64 = np.uint64
NONE, NOADAPTER, B = 0xFFFFFFFF, np.uint64(0xFFFFFFFF), 256
HOLE, GONE, PA, PB, PF = 5, 9, 70, 71, 72                 # a hole; a pod removed after the inserts; the holders of 127 / 128 / 73 blocks
CHAIN = ((1, 3), (2, 2), (3, 1), (4, 4))                  # QUEUE x 3, KV x 2, LORA x 1, PREFIX x 4
ROWS = ["n0", "n63", "n64", "n65", "n256", "one", "sizes", "lacks", "emptied", "miss0", "hole", "c200", "displaced"]


def summary(model, reqs, P, mask=None):
    """{walk, best, holders, first} of §3m, u32 [R, 4]."""
    out = np.zeros((len(reqs), 4), dtype=np.uint32)
    out[:, 3] = NONE
    for r, row in enumerate(reqs):
        nb, adapter = int(row[0] >> U64(32)), int(row[0] & NOADAPTER)
        if nb > B or 128 <= adapter < NONE:
            continue
        matched = {}
        for i in range(nb):
            s = model.get(int(row[1 + i]))
            if not s:
                break
            out[r, 0] += 1
            for p in s:
                matched[p] = matched.get(p, 0) + 1
        cand = {p: m for p, m in matched.items() if p < P and p != HOLE and (mask is None or (int(mask[r, p >> 6]) >> (p & 63)) & 1)}
        if cand:
            best = max(cand.values())
            out[r, 1:] = best, sum(m == best for m in cand.values()), min(p for p, m in cand.items() if m == best)
    return out


def build(pkg, P, slots=1 << 13, chain=((4, 1),)):
    """A picker over P pods (pod HOLE a hole, pod GONE removed, both after the inserts), its model and one request row per name in ROWS."""
    rng = np.random.default_rng(P)
    trio, some = {0, 63, P - 1}, lambda n, lo=100: set(range(lo, lo + n))
    sets = {"n0": [], "n63": [trio] * 63, "n64": [trio] * 64, "n65": [trio] * 65, "n256": [trio] * 256,      # all hit: 1 and 2 and 4 trips
            "one": [{P - 1}] * 3,
            "sizes": [some(24), some(25), {100}, some(25, 101), some(24, 101)],      # the list at its cap, the first dense row, listed / dense in turn
            "lacks": [{1}, {1, 3}, {3}, {3}],                                          # pod 3 lacks block 0 and still holds the most
            "emptied": [{2}, {GONE}, {2}],                                             # a present key whose set is emptied: the walk ends there
            "miss0": [{4}] * 3,
            "hole": [{HOLE, 7}, {HOLE, 8}, {HOLE, 7}],
            "c200": [{PA, PB}] * 127 + [{PB, PF}] + [{PF}] * 72,                       # 127 -> 128: a carry through every plane
            "displaced": [{6}] * 7}                                                    # seven keys of one home bucket: two live in the next one
    model, reqs, hs_all, ps_all = {}, np.zeros((len(ROWS), B + 1), dtype=U64), [], []
    for r, name in enumerate(ROWS):
        n = len(sets[name])
        hs = ip.keys_for_buckets([3], [7], slots or 64, P)[0] if name == "displaced" else rng.integers(1, 2 ** 63, n, dtype=np.int64).astype(U64)
        reqs[r, 0], reqs[r, 1:1 + n] = (U64(n) << U64(32)) | NOADAPTER, hs
        for i, s in enumerate(sets[name]):
            if slots and not (name == "miss0" and i == 0):
                model[int(hs[i])] = set(s) - {HOLE, GONE}
                hs_all.append(np.full(len(s), hs[i], dtype=U64))
                ps_all.append(np.array(sorted(s), dtype=np.uint32))
    pods = np.zeros(P, dtype=pkg.picker.POD_DTYPE)
    pods["queue"], pods["kv_util"] = rng.integers(1, 50, P), rng.random(P)
    pk = pkg.BatchedPicker(list(chain), max_pods=P, max_blocks=B, max_batch=64, index_slots=slots)
    pk.publish(pods)
    if slots:
        pk.index_insert(np.concatenate(hs_all), np.concatenate(ps_all))
        pk.index_remove_pod(GONE)
    pods["flags"][HOLE] = 1
    pk.publish(pods)                                                                   # (the index forgets a hole: scrubbed at publish)
    return pk, model, reqs


def mask_rows(P):
    """Without pod 0 (a tie's first) and PB (the only best holder of c200); every fifth row empty."""
    bits = np.ones((len(ROWS), (P + 63) // 64 * 64), dtype=bool)
    bits[:, P:] = bits[:, [0, PB]] = bits[4::5] = False
    return np.packbits(bits.reshape(len(ROWS), -1, 64), axis=2, bitorder="little").view("<u8").reshape(len(ROWS), -1).astype(U64)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("max_cu", [None, "1"])
@pytest.mark.parametrize("P", [1000, 2000, 4096])                                      # a u16, a u32 and a u64 lane word; pod P - 1 is its top used bit
def test_summary_equals_the_walk(pkg, monkeypatch, P, max_cu, masked):
    if max_cu:
        monkeypatch.setenv("EPPK_MAX_CU", max_cu)
    pk, model, reqs = build(pkg, P)
    mask = mask_rows(P) if masked else None
    want = summary(model, reqs, P, mask)
    with pk:
        got = pk.prefix_summary(reqs, mask)
    assert got.dtype == np.uint32 and np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    w = dict(zip(ROWS, want.tolist()))
    if masked:
        assert w["c200"] == [200, 127, 1, PA] and w["n63"] == [63, 63, 2, 63] and w["n256"] == [256, 0, 0, NONE]
    else:
        assert w["c200"] == [200, 128, 1, PB] and w["n256"] == [256, 256, 3, 0] and w["one"] == [3, 3, 1, P - 1] and w["sizes"] == [5, 4, 23, 101]
        assert w["lacks"] == [4, 3, 1, 3] and w["emptied"] == [1, 1, 1, 2] and w["miss0"] == w["n0"] == [0, 0, 0, NONE]
        assert w["hole"] == [3, 2, 1, 7] and w["displaced"] == [7, 7, 1, 6] and w["n65"] == [65, 65, 3, 0]


def test_bad_rows_refusals_and_no_index(pkg):
    import torch
    P = 1000
    pk, model, reqs = build(pkg, P)
    R, out = len(reqs), np.zeros((len(reqs), 4), dtype=np.uint32)
    with pkg.BatchedPicker([(4, 1)], max_pods=P, max_blocks=B, max_batch=64) as fresh:
        assert fresh._lib.eppk_prefix_summary(fresh._ctx, reqs.ctypes.data, R, None, out.ctypes.data) == -4                # no snapshot
    with pk:
        assert pk._lib.eppk_prefix_summary(pk._ctx, reqs.ctypes.data, R, None, None) == -1
        assert pk._lib.eppk_prefix_summary(pk._ctx, reqs.ctypes.data, pk.max_batch + 1, None, out.ctypes.data) == -2
        reqs[3, 0] = (U64(B + 5) << U64(32)) | NOADAPTER
        reqs[7, 0] = (U64(2) << U64(32)) | U64(128)
        with pytest.raises(pkg.EppkError) as e:
            pk.prefix_summary(reqs)
        assert e.value.code == -1 and "row 3" in str(e.value) and pk.launch_status() == 0
        d_reqs, d_out = torch.from_numpy(reqs.view(np.int64)).cuda(), torch.full((R, 4), -7, dtype=torch.int32, device="cuda")
        pk.prefix_summary_device(d_reqs.data_ptr(), R, d_out.data_ptr())
        torch.cuda.synchronize()
        assert pk.launch_status() == 1                                                 # EPPK_LAUNCH_BAD_REQUEST_ROW
    want = summary(model, reqs, P)
    assert want[3].tolist() == want[7].tolist() == [0, 0, 0, NONE] and np.array_equal(d_out.cpu().numpy().view(np.uint32), want)
    pk, _, reqs = build(pkg, P, slots=0)
    with pk:
        assert np.array_equal(pk.prefix_summary(reqs, mask_rows(P)), summary({}, reqs, P))


def same(got, want, what):
    for g, w, name in zip(got, want, ("picks", "scores", "route")):
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4].tolist())


def device_lists(call, R, k):
    """What a *_device pick form leaves in fresh device buffers: ([R, k] picks, [R, k] scores as uint64, the route bytes)."""
    import torch
    d_p, d_s = torch.full((R, k), -7, dtype=torch.int32, device="cuda"), torch.full((R, k), -7.0, dtype=torch.float64, device="cuda")
    d_r = torch.full((R,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                                                           # (the fills run on torch's stream, the call on the context's)
    call(d_p.data_ptr(), d_s.data_ptr(), d_r.data_ptr())
    torch.cuda.synchronize()
    return d_p.cpu().numpy(), d_s.cpu().numpy().view(U64), d_r.cpu().numpy()


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("form", ["session", "prefix"])
def test_hybrid_rows_are_topk_or_rendezvous(pkg, form, masked, k):
    import torch
    P, seed, min_hit = 1000, 11, 64
    pk, model, reqs = build(pkg, P, chain=CHAIN)
    R, mask = len(reqs), mask_rows(P) if masked else None
    key = np.random.default_rng(5).integers(0, 2 ** 64, R, dtype=U64) if form == "session" else None
    depth = 0 if form == "session" else 2
    warm = summary(model, reqs, P, mask)[:, 1] >= min_hit
    assert {63, 64, 65} <= set(summary(model, reqs, P, mask)[:, 1].tolist())           # min_hit - 1, min_hit, min_hit + 1
    with pk:
        top, rdv = pk.pick_topk(reqs, k, mask), pk.pick_rendezvous_scored(reqs, k, seed, 0, key, depth, mask=mask)
        want = [np.where(warm[:, None], t, c) for t, c in zip(top, rdv)]
        want = want[0], want[1].view(U64), warm.astype(np.uint8)
        assert np.any(top[0][warm] != rdv[0][warm]) and np.any(top[0][~warm] != rdv[0][~warm])
        got = pk.pick_hybrid(reqs, k, seed, min_hit, key, depth, mask=mask)
        same((got[0], got[1].view(U64), got[2]), want, "host form")
        d_reqs = torch.from_numpy(reqs.view(np.int64)).cuda()
        d_key = torch.from_numpy(key.view(np.int64)).cuda() if key is not None else None
        d_mask = torch.from_numpy(mask.view(np.int64)).cuda() if masked else None
        dev = device_lists(lambda p, s, r: pk.pick_hybrid_device(d_reqs.data_ptr(), R, k, seed, min_hit, p, s, r, d_key.data_ptr() if key is not None else None, depth,
                                                                 d_mask=d_mask.data_ptr() if masked else None), R, k)
        same(dev, want, "device form")
        assert pk.launch_status() == 0
        a = [np.full((R, k), -7, dtype=np.int32), np.full((R, k), -7.0), np.full(R, 7, dtype=np.uint8)]
        rc = pk._lib.eppk_pick_hybrid(pk._ctx, reqs.ctypes.data, R, key.ctypes.data if key is not None else None, depth, None, None, k, seed, 0,
                                      a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data)
        assert rc == -1 and np.all(a[0] == -7) and np.all(a[1] == -7.0) and np.all(a[2] == 7)                              # min_hit = 0


def test_hybrid_scratch_grows_and_a_bad_row_is_cold(pkg):
    import torch
    P, k, seed, min_hit = 1000, 4, 3, 3
    pk, model, reqs = build(pkg, P, chain=CHAIN)
    with pk:
        for n in (5, 300, 5):                                                          # max_batch is 64: the second call replaces the scratch
            rows = np.tile(reqs, (n // len(reqs) + 1, 1))[:n].copy()
            rows[2, 0] = (U64(B + 1) << U64(32)) | NOADAPTER
            d_reqs = torch.from_numpy(rows.view(np.int64)).cuda()
            top = device_lists(lambda p, s, r: pk._check(pk._lib.eppk_pick_topk_device(pk._ctx, d_reqs.data_ptr(), n, None, k, p, s, None), "topk"), n, k)
            rdv = device_lists(lambda p, s, r: pk.pick_rendezvous_scored_device(d_reqs.data_ptr(), n, k, seed, 0, p, s, depth=2), n, k)
            got = device_lists(lambda p, s, r: pk.pick_hybrid_device(d_reqs.data_ptr(), n, k, seed, min_hit, p, s, r, depth=2), n, k)
            warm = summary(model, rows, P)[:, 1] >= min_hit
            assert warm.any() and not warm.all() and not warm[2] and np.all(got[0][2] == -1) and np.all(got[1][2] == 0)
            same(got, (np.where(warm[:, None], top[0], rdv[0]), np.where(warm[:, None], top[1], rdv[1]), warm.astype(np.uint8)), n)
        assert pk.launch_status() == 1
