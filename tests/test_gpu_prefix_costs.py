"""GPU: costs per list entry from the prefix index (SEMANTICS.md §3k; include/eppk.h eppk_prefix_costs, eppk_pick_cost_cached) against
a dict hash -> set(pods) filled by the same index_insert calls and the walk of §3k written out below; everything exact, as uint32."""
import costed_ref as cref
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U64 = np.uint64
NOADAPTER = U64(0xFFFFFFFF)
MAX_COST = 0x00FFFFFF
HOLE = 5                                             # inserted as a member, then published as a hole
SIZES = [1, 24, 25, 3, 1, 0, 2, 25]                  # pod-set sizes by block (0: every pod): listed, full list, first overflow, dense


def walk(model, reqs, lists, n_pods, holes, max_blocks, unit=1, base=None):
    """(cost, matched) of §3k, u32 [R, k]."""
    R, k = lists.shape
    matched = np.zeros((R, k), dtype=np.int64)
    nbs = (reqs[:, 0] >> U64(32)).astype(np.int64)
    for r in range(R):
        sets = []
        for i in range(nbs[r] if nbs[r] <= max_blocks else 0):
            s = model.get(int(reqs[r, 1 + i]))
            if not s:
                break
            sets.append(s)
        for j, p in enumerate(lists[r]):
            if 0 <= p < n_pods and p not in holes:
                matched[r, j] = sum(int(p) in s for s in sets)
    b = (np.clip(nbs * unit, 1, 2 ** 32 - 1) if base is None else np.asarray(base, dtype=np.int64))[:, None].repeat(k, 1)
    cost = np.where((b >= 1) & (b <= MAX_COST), np.maximum(1, b - np.minimum(b, matched * unit)), b)
    return cost.astype(np.uint32), matched.astype(np.uint32)


def build(pkg, P, B, R_min=0, slots=1 << 16, chain=((1, 1),)):
    """A picker over P pods (pod HOLE a hole, published after the inserts), its model, request rows and lists of 8 entries."""
    rng = np.random.default_rng(1000 * P + B)
    G = 16 if B <= 16 else 32 if B <= 32 else 64
    front, rows, model, hs_all, ps_all = [0, 63, 64, P - 1, HOLE], [], {}, [], []
    rest = np.setdiff1d(np.arange(P), front)

    def chain_row(nb, miss=(), lacks=None, size=None, first=()):
        hs = rng.integers(1, 2 ** 63, nb, dtype=np.int64).astype(U64)
        hs[:len(first)] = first
        order = rng.permutation(rest)                                           # the row's own holders: the same pods in every larger set
        for i in range(nb):
            if i in miss:                                                       # (blocks behind a miss ARE inserted: they must not count)
                continue
            n = SIZES[(i + len(rows)) % 8] if size is None else size
            pods = np.concatenate([np.roll(front, i + len(rows)), order])[:n or P]
            if lacks and i == lacks[0]:
                pods = pods[pods != lacks[1]]
            model[int(hs[i])] = set(pods.tolist())
            hs_all.append(np.full(pods.size, hs[i], dtype=U64))
            ps_all.append(pods.astype(np.uint32))
        rows.append(hs)

    for nb in sorted({min(n, B) for n in (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256)}):
        chain_row(nb)
    for m in sorted({0, G - 1, G, B - 1}):
        if m < B:
            chain_row(B, miss={m}, size=24 if m else None)
    chain_row(min(B, 6), lacks=(2, 64), size=24)                                # pod 64 misses block 2, holds 3..5
    chain_row(min(B, 5), size=0)                                                # every pod holds the whole prompt
    chain_row(min(B, 4), first=[0, 2 ** 64 - 1])                                # the reserved hashes
    while len(rows) < R_min:
        chain_row(int(rng.integers(0, B + 1)), miss={int(rng.integers(0, B + 1))})
    reqs = np.zeros((len(rows), B + 1), dtype=U64)
    for r, hs in enumerate(rows):
        reqs[r, 0] = (U64(len(hs)) << U64(32)) | NOADAPTER
        reqs[r, 1:1 + len(hs)] = hs
    pool = np.array([0, 63, -1, 64, P - 1, P, HOLE, 70000, 1, 7], dtype=np.int32)
    lists = np.stack([np.roll(pool, -r)[:8] for r in range(len(rows))])
    lists[1::2, 7] = lists[1::2, 0]                                             # a pod twice in a list
    pods = np.zeros(P, dtype=pkg.picker.POD_DTYPE)
    pk = pkg.BatchedPicker(list(chain), max_pods=P, max_blocks=B, max_batch=max(len(rows), 64), index_slots=slots)
    pk.publish(pods)
    if slots:
        pk.index_insert(np.concatenate(hs_all), np.concatenate(ps_all))
    assert any(HOLE in s for s in model.values())
    pods["flags"][HOLE] = 1
    pk.publish(pods)
    for members in model.values():                                              # the index forgets a hole (scrubbed at publish)
        members.discard(HOLE)
    return pk, model, reqs, lists, pods


def same(got, want, what=""):
    for g, w, name in zip(got, want, ("cost", "matched")):
        assert g.dtype == np.uint32 and np.array_equal(g, w), (what, name, np.argwhere(g != w)[:4].tolist())


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("P,B", [(200, 8), (2000, 70), (4096, 256)])
def test_matched_equals_the_walk(pkg, P, B, k):
    pk, model, reqs, lists, _ = build(pkg, P, B)
    lists = np.ascontiguousarray(lists[:, :k] if k > 1 else lists[:, 3:4])
    with pk:
        got = pk.prefix_costs(reqs, lists)
    want = walk(model, reqs, lists, P, {HOLE}, B)
    same(got, want)
    assert np.any((want[1] > 0) & (want[1] < (reqs[:, 0] >> U64(32))[:, None])) and (k == 1 or want[1].max() >= B - 1)


@pytest.mark.parametrize("unit", [1, 3])
def test_costs(pkg, unit):
    import torch
    P, B, k = 200, 8, 8
    pk, model, reqs, lists, _ = build(pkg, P, B)
    R = reqs.shape[0]
    base = np.random.default_rng(unit).integers(1, 40, R).astype(np.uint32)
    base[:2] = [0, MAX_COST + 1]
    with pk:
        for b in (base, None):
            want = walk(model, reqs, lists, P, {HOLE}, B, unit, b)
            same(pk.prefix_costs(reqs, lists, unit, b), want, b is None)
            if b is not None:
                assert np.all(want[0][0] == 0) and np.all(want[0][1] == MAX_COST + 1)
        whole = want[1][R - 2] == 5                                             # the row every pod holds whole: cost 1, not 0
        assert np.any(whole) and np.all(want[0][R - 2][whole] == 1)
        reqs[3, 0] = (U64(B + 5) << U64(32)) | NOADAPTER                        # a bad row
        with pytest.raises(pkg.EppkError) as e:
            pk.prefix_costs(reqs, lists, unit, base)
        assert e.value.code == -1 and pk.launch_status() == 0
        d_reqs, d_lists = torch.from_numpy(reqs.view(np.int64)).cuda(), torch.from_numpy(lists).cuda()
        d_base = torch.from_numpy(base.view(np.int32)).cuda()
        d_out = torch.full((2, R, k), -7, dtype=torch.int32, device="cuda")
        pk.prefix_costs_device(d_reqs.data_ptr(), R, d_lists.data_ptr(), k, d_base.data_ptr(), unit, d_out[0].data_ptr(), d_out[1].data_ptr())
        assert pk.launch_status() == 1                                          # EPPK_LAUNCH_BAD_REQUEST_ROW
        want = walk(model, reqs, lists, P, {HOLE}, B, unit, base)
        assert np.all(want[1][3] == 0) and np.all(want[0][3] == base[3])
        same(tuple(d_out.cpu().numpy().view(np.uint32)), want, "device form with a bad row")


def test_no_index_matches_nothing(pkg):
    pk, _, reqs, lists, _ = build(pkg, 200, 8, slots=0)
    with pk:
        same(pk.prefix_costs(reqs, lists, 2), walk({}, reqs, lists, 200, {HOLE}, 8, 2))


def test_after_maintenance(pkg):
    P, B = 2000, 70
    pk, model, reqs, lists, _ = build(pkg, P, B)
    with pk:
        pk.index_remove_pod(63)
        epoch = pk.index_advance_epoch()
        keep = [h for i, h in enumerate(sorted(model)) if i % 3 or h in (0, 2 ** 64 - 1)]       # refreshed: stamped with the new epoch
        pk.index_insert(np.array(keep, dtype=U64), np.full(len(keep), 7, dtype=np.uint32))
        assert pk.index_evict_older(epoch) > 0
        got = pk.prefix_costs(reqs, lists)
    model = {h: (model[h] - {63}) | {7} for h in keep}
    want = walk(model, reqs, lists, P, {HOLE}, B)
    same(got, want)
    assert np.any(want[1] > 0)


def test_many_passes_per_wavefront(pkg, monkeypatch):
    P, B, got = 200, 8, {}
    for max_cu in (None, "1"):
        if max_cu:
            monkeypatch.setenv("EPPK_MAX_CU", max_cu)
        pk, model, reqs, lists, _ = build(pkg, P, B, R_min=1537)
        with pk:
            got[max_cu] = pk.prefix_costs(reqs, lists, 2)
            g = pk.launch_geometry()
        same(got[max_cu], walk(model, reqs, lists, P, {HOLE}, B, 2), max_cu)
        assert reqs.shape[0] == 1537 and g[:2] == (0, 0) and g[3] == 256
        assert g[2] > 4 if not max_cu else (1537 + 3) // 4 >= 3 * g[2] * 4, g    # G = 16: four requests per pass, four wavefronts per workgroup


def test_pick_form_charges_the_cached_entry_less(pkg):
    """QUEUE x 3 + PREFIX x 1 and two idle pods: they lead every list, the row's best holders follow.  A cap below a long prompt: the idle
    pods cannot take it even alone, the entry that caches it can -- rank >= 1 BECAUSE of the per-entry cost."""
    import torch
    P, B, k, cap = 200, 8, 4, 5
    bands = ((cref.SHED, 0), (cref.SPILL, 1))
    pk, model, reqs, _, pods = build(pkg, P, B, R_min=300, chain=((1, 3), (4, 1)))
    R = reqs.shape[0]
    pods["queue"] = np.random.default_rng(3).integers(1, 3, P)
    pods["queue"][100:102] = 0
    band = (np.arange(R) % 3 == 0).astype(np.uint8)
    with pk:
        pk.publish(pods)
        lists, scores = pk.pick_topk(reqs, k)
        cost, _ = walk(model, reqs, lists, P, {HOLE}, B)
        wp, ws, wr, wl, _ = cref.resolve(lists, scores, P, cost, bands, band, None, cap, np.zeros(P, dtype=np.uint32), per_entry=True)
        rows = np.nonzero((wr >= 1) & (wr < k))[0]
        assert any(cost[r, 0] > cap >= cost[r, wr[r]] for r in rows)            # entry 0 could not fit even alone; the cached entry did
        hp, hs, hr, hl = pk.pick_costed_cached(reqs, k, cap, bands=bands, band=band, load=np.zeros(P, dtype=np.uint32))
        d = {n: torch.zeros(sz, dtype=t, device="cuda") for n, sz, t in [("pick", R, torch.int32), ("score", R, torch.float64), ("rank", R, torch.uint8),
                                                                         ("load", P, torch.int32)]}
        d_reqs, d_band = torch.from_numpy(reqs.view(np.int64)).cuda(), torch.from_numpy(band).cuda()
        pk.pick_costed_cached_device(d_reqs.data_ptr(), R, None, k, None, 1, d_band.data_ptr(), bands, None, cap, d["load"].data_ptr(),
                                     d["pick"].data_ptr(), d["score"].data_ptr(), d["rank"].data_ptr())
        assert pk.launch_status() == 0
    dev = {n: t.cpu().numpy() for n, t in d.items()}
    for p_, s_, r_, l_ in ((hp, hs, hr, hl), (dev["pick"], dev["score"], dev["rank"], dev["load"].view(np.uint32))):
        assert np.array_equal(p_, wp) and np.array_equal(r_, wr) and np.array_equal(l_, wl) and np.array_equal(s_.view(U64), ws.view(U64))
