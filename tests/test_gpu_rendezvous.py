"""GPU: the picker "rendezvous" (SEMANTICS.md §3j; include/eppk.h eppk_pick_rendezvous) against tests/rendezvous_ref.py, exactly: picks,
and scores as uint64.  The kernel has ONE geometry, so no pod count changes its path: the pod counts are the sides of the 64-pod word,
and 1537 requests are no multiple of the eight of a pass nor of the sixteen wavefronts of a workgroup."""
import bounded_ref as bref
import numpy as np
import pytest
import rendezvous_ref as ref

pytestmark = pytest.mark.gpu
U64 = np.uint64
NOADAPTER = U64(0xFFFFFFFF)


def _picker(pkg, P, R, holes=0.1, max_pods=None, B=0):
    pods = np.zeros(P, dtype=pkg.picker.POD_DTYPE)
    pods["flags"] = (np.random.default_rng(P).random(P) < holes).astype(np.uint32)
    pk = pkg.BatchedPicker([(1, 1)], max_pods=max_pods or P, max_blocks=B, max_batch=R)
    pk.publish(pods)
    return pk, pods


def _pack(bits):
    full = np.zeros((bits.shape[0], (bits.shape[1] + 63) // 64 * 64), dtype=bool)
    full[:, :bits.shape[1]] = bits
    return np.packbits(full.reshape(len(bits), -1, 64)[:, :, ::-1], axis=2).view(">u8").reshape(len(bits), -1).astype(U64)


def _mixed_mask(R, P, flags, seed):
    """Rows by r % 4: half the pods, 1..8 pods, half again; rows 36, 73, ... empty; row 5 names the holes only."""
    rng = np.random.default_rng(seed)
    bits = rng.random((R, P)) < 0.5
    for r in range(1, R, 4):
        bits[r] = False
        bits[r, rng.choice(P, size=min(P, int(rng.integers(1, 9))), replace=False)] = True
    bits[36::37] = False
    bits[5:6] = (flags & 1) != 0
    return _pack(bits)


def _keys(R, seed):
    """Random keys; 0 and 2^64 - 1 in front; keys 4..7 differ in their upper 32 bits only."""
    key = np.random.default_rng(seed).integers(0, 2 ** 64, R, dtype=U64)
    key[:2] = np.array([0, 2 ** 64 - 1], dtype=U64)[:R]
    key[4:8] = (U64(0x1234) | (np.arange(4, dtype=U64) << U64(32)))[:max(0, min(R, 8) - 4)]
    return key


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, np.nonzero(np.any(got[0] != want[0], axis=1))[0][:4])
    assert np.array_equal(got[1].view(U64), want[1].view(U64)), what


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("R", [1, 1537])
@pytest.mark.parametrize("P,max_pods", [(1, 1), (63, 63), (64, 64), (65, 65), (130, 200), (4096, 4096)])
def test_matches_the_restatement(pkg, P, max_pods, R, masked):
    pk, pods = _picker(pkg, P, R, max_pods=max_pods)
    mask = _mixed_mask(R, P, pods["flags"], 100 + P) if masked else None
    cand, key = ref.candidates(R, P, pods["flags"], mask), _keys(R, 7 + P)
    pod_key = np.random.default_rng(P).integers(0, 2 ** 64, P, dtype=U64)
    with pk:
        for k, seed, pkey in [(1, 0, None), (2, 0xDEADBEEFCAFEF00D, pod_key), (8, 0, pod_key), (8, 0xDEADBEEFCAFEF00D, None)]:
            got = pk.pick_rendezvous(None, k, seed, key=key, pod_key=pkey, mask=mask)
            _same(got, ref.rendezvous(key, k, seed, cand, pkey), (k, seed))
    if masked and R > 37:
        assert np.all(got[0][36::37] == -1) and np.all(got[0][5] == -1) and np.any(got[0][:, 0] >= 0) and np.any(got[0][:, 7] < 0)


@pytest.mark.parametrize("P", [200, 4096])
def test_ties_go_to_the_lowest_pod(pkg, P):
    """Every pod key is shared by three pods in different lanes and words (67 is coprime to P): equal hashes in every round."""
    R, k, pod_key = 257, 8, (((np.arange(P) * 67) % P) // 3).astype(U64)
    pk, pods = _picker(pkg, P, R, holes=0.0)
    with pk:
        for mask in (None, _mixed_mask(R, P, pods["flags"], 9)):
            got = pk.pick_rendezvous(None, k, 5, key=_keys(R, 3), pod_key=pod_key, mask=mask)
            _same(got, ref.rendezvous(_keys(R, 3), k, 5, ref.candidates(R, P, None, mask), pod_key))
            assert all(np.unique(row[row >= 0]).size == np.count_nonzero(row >= 0) for row in got[0])
            assert np.any(got[1][:, 0] == got[1][:, 1])                                         # ties did occur at the top


@pytest.mark.parametrize("depth", [1, 4, 13])
def test_prefix_form(pkg, depth):
    import torch
    B, P, k, d = 8, 300, 3, min(depth, 8)                                                       # depth 13 = max_blocks + 5
    nbs = sorted({0, 1, min(depth - 1, B), d, min(depth + 1, B), B}) * 9 + [B, B]
    reqs = np.random.default_rng(depth).integers(1, 2 ** 63, (len(nbs), B + 1), dtype=np.int64).astype(U64)
    reqs[:, 0] = (np.array(nbs, dtype=U64) << U64(32)) | NOADAPTER
    reqs[-1, 1:d + 1] = reqs[-2, 1:d + 1]                                   # the last two rows share their first `depth` blocks
    R = len(nbs)
    pk, pods = _picker(pkg, P, R, B=B)
    want = ref.rendezvous(ref.prefix_keys(reqs, depth), k, 11, ref.candidates(R, P, pods["flags"]))
    with pk:
        _same(pk.pick_rendezvous(reqs, k, 11, depth=depth), want)
        assert np.array_equal(want[0][-1], want[0][-2]) and (depth > B or not np.array_equal(reqs[-1], reqs[-2]))
        reqs[3, 0] = (U64(B + 5) << U64(32)) | NOADAPTER                                        # n_blocks > max_blocks
        with pytest.raises(pkg.EppkError) as e:
            pk.pick_rendezvous(reqs, k, 11, depth=depth)
        d_reqs = torch.from_numpy(reqs.view(np.int64)).cuda()
        d_pick = torch.full((R, k), -7, dtype=torch.int32, device="cuda")
        d_score = torch.full((R, k), -7.0, dtype=torch.float64, device="cuda")
        assert e.value.code == -1 and pk.launch_status() == 0
        pk.pick_rendezvous_device(d_reqs.data_ptr(), R, k, 11, d_pick.data_ptr(), d_score.data_ptr(), depth=depth)
        assert pk.launch_status() == 1                                                          # EPPK_LAUNCH_BAD_REQUEST_ROW
    want[0][3], want[1][3] = -1, 0.0
    _same((d_pick.cpu().numpy(), d_score.cpu().numpy()), want, "device form with a bad row")


@pytest.mark.parametrize("masked", [False, True])
def test_many_trips_per_wavefront(pkg, monkeypatch, masked):
    R, P, k, key, got = 1537, 130, 4, _keys(1537, 21), {}
    for max_cu in (None, "1"):
        if max_cu:
            monkeypatch.setenv("EPPK_MAX_CU", max_cu)
        pk, pods = _picker(pkg, P, R)
        mask = _mixed_mask(R, P, pods["flags"], 3) if masked else None
        with pk:
            got[max_cu] = pk.pick_rendezvous(None, k, 9, key=key, mask=mask)
            g = pk.launch_geometry()
        _same(got[max_cu], ref.rendezvous(key, k, 9, ref.candidates(R, P, pods["flags"], mask)), max_cu)
        assert g[2] > 4 if not max_cu else (g[:2] == (0, 0) and g[3] == 1024 and (R + 7) // 8 >= 3 * g[2] * 16), g   # >= 3 passes per wavefront


@pytest.mark.parametrize("how", ["hole", "mask"])
def test_minimal_disruption(pkg, how):
    R, P, k, gone, key = 1000, 130, 3, 77, _keys(1000, 5)
    pod_key = np.random.default_rng(2).integers(0, 2 ** 64, P, dtype=U64)
    full = ref.rendezvous(key, k + 1, 1, np.ones((R, P), dtype=bool), pod_key)[0]               # the old list and the next candidate
    want = np.stack([np.array([p for p in row if p != gone][:k]) for row in full])
    assert np.any(full[:, :k] == gone) and np.any(np.all(full[:, :k] != gone, axis=1))
    pk, pods = _picker(pkg, P, R, holes=0.0)
    with pk:
        before = pk.pick_rendezvous(None, k, 1, key=key, pod_key=pod_key)[0]
        pods["flags"][gone] = how == "hole"
        pk.publish(pods)
        mask = _pack(np.arange(P)[None, :].repeat(R, 0) != gone) if how == "mask" else None
        after = pk.pick_rendezvous(None, k, 1, key=key, pod_key=pod_key, mask=mask)[0]
    assert np.array_equal(before, full[:, :k]) and np.array_equal(after, want)


def test_chwbl_is_rendezvous_into_the_bounded_resolve(pkg):
    import torch
    R, P, k, key = 3000, 100, 4, _keys(3000, 8)
    cap = int(1.25 * R / P) + 1
    pk, pods = _picker(pkg, P, R)
    lists, scores = ref.rendezvous(key, k, 3, ref.candidates(R, P, pods["flags"]))
    wp, ws, wr, wl, _ = bref.resolve(lists, scores, P, None, cap, bref.SPILL)
    with pk:
        st = torch.cuda.Stream()
        d_key = torch.from_numpy(key.view(np.int64)).cuda()
        d = {n: torch.zeros(sz, dtype=t, device="cuda") for n, sz, t in [("lists", R * k, torch.int32), ("ls", R * k, torch.float64), ("pick", R, torch.int32),
                                                                         ("score", R, torch.float64), ("rank", R, torch.uint8), ("load", P, torch.int32)]}
        torch.cuda.synchronize()
        pk.pick_rendezvous_device(None, R, k, 3, d["lists"].data_ptr(), d["ls"].data_ptr(), d_key=d_key.data_ptr(), stream=st.cuda_stream)
        pk.bounded_resolve_device(d["lists"].data_ptr(), d["ls"].data_ptr(), R, k, None, cap, bref.SPILL, d["load"].data_ptr(), d["pick"].data_ptr(),
                                  d["score"].data_ptr(), d["rank"].data_ptr(), st.cuda_stream)
        st.synchronize()
        assert pk.launch_status() == 0
    out = {n: t.cpu().numpy() for n, t in d.items()}
    assert np.array_equal(out["pick"], wp) and np.array_equal(out["rank"], wr) and np.array_equal(out["load"].view(np.uint32), wl)
    assert np.array_equal(out["score"].view(U64), ws.view(U64)) and wl.max() >= cap and np.any(wr > 0)          # the cap did bind


def test_refusals_change_nothing(pkg):
    R, P, k, key = 100, 70, 2, _keys(100, 1)
    pods = np.zeros(P, dtype=pkg.picker.POD_DTYPE)
    picks, scores, reqs = np.full(R * 9, 77, dtype=np.int32), np.full(R * 9, 0.5), np.zeros((R, 5), dtype=U64)
    with pkg.BatchedPicker([(1, 1)], max_pods=P, max_blocks=4, max_batch=R) as pk:
        call = lambda kk, kp, depth: pk._lib.eppk_pick_rendezvous(pk._ctx, reqs.ctypes.data, R, kp, depth, None, None, kk, 4,      # noqa: E731
                                                                   picks.ctypes.data, scores.ctypes.data)
        assert call(k, key.ctypes.data, 0) == -4                                                # EPPK_ERR_NO_SNAPSHOT
        pk.publish(pods)
        assert call(0, key.ctypes.data, 0) == -1 and call(9, key.ctypes.data, 0) == -1          # EPPK_ERR_ARG: k out of range
        assert call(k, None, 0) == -1 and np.all(picks == 77) and np.all(scores == 0.5)         # neither keys nor a depth
        for E in (0, 2):                                                                        # assumed load on changes nothing
            pk.set_assumed_load(E)
            _same(pk.pick_rendezvous(None, k, 4, key=key), ref.rendezvous(key, k, 4, np.ones((R, P), dtype=bool)), E)
