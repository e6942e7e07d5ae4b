"""Differential fuzzing of the picker "weighted-random" (SEMANTICS.md §3c; pick_wrand_kernel) against the oracle's totals fed to the
numpy restatement (tests/wrand_ref.py): picks equal, scores equal as uint64, no tolerance.  Random chains (empty, all-zero, QUEUE / KV
not leading, six entries), pod counts at the edges of every lane word, `max_pods` of a wider lane-word class than the pods need, block
counts across both counter-plane widths, coarse gauges, masks with empty / single / tiny rows, holes, tiny index tables, both list
modes; every instantiation at its edges; launch geometry; the picker behind index maintenance; the descent where x meets a node sum
exactly (words chosen through the inverse of the mixer).  Seeds are fixed: a failure names its case.  The tests without a `gpu` mark
hold the generator to the coverage the others rely on, and the chosen words to the boundaries they are meant to hit."""
import importlib.util
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu

Q, KV, L, PF = 1, 2, 3, 4
BASE = [(Q, 2), (KV, 2), (L, 1), (PF, 3)]
NEG = [(Q, 2), (KV, -3), (PF, 3)]
MIX = [(PF, 1), (Q, -1), (KV, 2), (Q, 3)]            # QUEUE behind PREFIX, twice, once with a negative weight
HIGH = 0x9E3779B97F4A7C15                             # a seed with the top bit set
N_SEEDS = 260
LW_TOP = (1024, 2048, 4096)                           # the largest max_pods of the lane words u16 / u32 / u64
LW_NAME = ("u16", "u32", "u64")


@pytest.fixture(scope="module")
def ref():
    spec = importlib.util.spec_from_file_location("wrand_ref", os.path.join(os.path.dirname(os.path.abspath(__file__)), "wrand_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _lw_class(max_pods):
    return 0 if max_pods <= 1024 else 1 if max_pods <= 2048 else 2


def _totals(orc, chain, pods, oix, reqs, mask=None):
    """[R, P] totals of the oracle (NaN = not a candidate)."""
    if reqs.shape[0] == 0:
        return np.zeros((0, pods.shape[0]))
    return np.stack([orc.score_row(chain, pods, oix, reqs[r], None if mask is None else mask[r]) for r in range(reqs.shape[0])])


def _same(got, want, what):
    gp, gs = got
    wp, ws = want
    bad = np.nonzero(np.any(gp != wp, axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[:4]}: gpu {gp[bad[:2]]} ref {wp[bad[:2]]}"
    sbad = np.nonzero(np.any(gs.view(np.uint64) != ws.view(np.uint64), axis=1))[0]
    assert sbad.size == 0, f"{what}: scores of {sbad.size} rows differ, first {sbad[:4]}: gpu {gs[sbad[:2]]} ref {ws[sbad[:2]]}"


def _subset_mask(rng, R, P, lo, hi, every=1):
    """[R, J] mask words: row r (r % every == 0) = a subset of lo..hi pods, the other rows every pod."""
    J = (P + 63) // 64
    bits = np.zeros((R, J * 64), dtype=bool)
    bits[:, :P] = True
    for r in range(0, R, every):
        bits[r] = False
        bits[r, rng.choice(P, size=min(P, int(rng.integers(lo, hi + 1))), replace=False)] = True
    return np.packbits(bits.reshape(R, J, 64)[:, :, ::-1], axis=2).view(">u8").reshape(R, J).astype(np.uint64)


def _mask_bits(mask, P):
    """[R, J] mask words -> [R, P] bool."""
    return ((mask[:, np.arange(P) // 64] >> (np.arange(P) % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)


# ---- the generator (the structure of test_gpu_fuzz._case, with this picker's own edges) ----------------------------------------------

def _case(pkg, seed):
    rng = np.random.default_rng(seed)
    P = int(rng.choice([1, 3, 63, 64, 65, 200, 1000, 1024, 1025, 1500, 2048, 2049, 2500, 4095, 4096]))
    B = int(rng.choice([0, 1, 5, 8, 31, 33, 63, 64, 70, 130, 256]))
    R = int(rng.integers(1, 200))
    max_pods = P
    up = rng.random(2)
    if up[0] < 0.25 and _lw_class(P) < 2:                  # a lane word wider than the pods need (one class up; two now and then)
        max_pods = LW_TOP[min(2, _lw_class(P) + (2 if up[1] < 0.3 else 1))]
    n_sc = int(rng.integers(0, 7))
    chain = [(int(rng.choice([Q, KV, L, PF])), int(rng.integers(-3, 6))) for _ in range(n_sc)]
    pods = pkg.workload.make_pods(int(rng.integers(1, 1 << 30)), P, 128)
    coarse = bool(rng.random() < 0.5)
    if coarse:                                             # coarse gauges: exact ties, qmax == qmin inside a subset, totals of exactly 0
        pods["queue"] = rng.integers(0, 3, P)
        pods["kv_util"] = rng.integers(0, 3, P) / 2.0
    # index: a few chains of random hashes (sometimes the reserved values), each block cached on a few pods
    n_chains = int(rng.integers(1, 6))
    chains = rng.integers(1, 2**63, (n_chains, max(B, 1)), dtype=np.uint64)
    if rng.random() < 0.3:
        chains[0, 0] = 0
    if rng.random() < 0.3 and B > 1:
        chains[-1, 1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    ih, ip = [], []
    for ci in range(n_chains):
        depth = int(rng.integers(0, B + 1))
        for b in range(depth):
            for pod in rng.integers(0, P, int(rng.integers(1, 6))):
                ih.append(chains[ci, b]); ip.append(pod)
    ih = np.asarray(ih, dtype=np.uint64); ip = np.asarray(ip, dtype=np.uint32)
    n_keys = max(len(set(ih.tolist())), 1)
    slots = 64
    while slots < (2 if rng.random() < 0.3 else 4) * n_keys:
        slots *= 2
    hs = chains[rng.integers(0, n_chains, R)].copy()
    for r in range(R):                                     # break chains at random depths
        if B and rng.random() < 0.7:
            cut = int(rng.integers(0, B))
            hs[r, cut:] = rng.integers(1, 2**63, B - cut, dtype=np.uint64)
    nblk = rng.integers(0, B + 1, R) if B else np.zeros(R, dtype=np.int64)
    reqs = pkg.picker.make_req_rows(rng.integers(-1, 128, R), nblk, hs[:, :B] if B else None, B)
    mask = None
    if rng.random() < 0.5:
        W = (P + 63) // 64
        mask = rng.integers(0, 2**63, (R, W), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (R, W), dtype=np.uint64)
        if rng.random() < 0.5:                             # sparse subsets
            mask &= rng.integers(0, 2**63, (R, W), dtype=np.uint64) & rng.integers(0, 2**63, (R, W), dtype=np.uint64)
        if P % 64:
            mask[:, -1] &= np.uint64((1 << (P % 64)) - 1)
        if seed % 2 == 0 and P >= 63:                      # every third row a handful of pods: k pads, positive totals run out mid-list
            small = _subset_mask(np.random.default_rng(seed ^ 0x5B5E7), R, P, 1, 12)
            mask[2::3] = small[2::3]
        mask[0, :] = 0
        if R > 1:
            mask[1, :] = 0; mask[1, 0] = np.uint64(1)
    if seed % 4 == 3:                                      # holes of the snapshot (SEMANTICS.md §6b), from a stream of their own
        hr = np.random.default_rng(seed ^ 0xA11CE)
        pods["flags"] = (hr.random(P) < hr.choice([0.05, 0.5, 0.95])).astype(np.uint32)
    k = 1 + seed % 8
    lists0 = bool(seed % 3 == 0 and B and ih.size)
    return dict(seed=seed, chain=chain, pods=pods, ih=ih, ip=ip, slots=slots, reqs=reqs, mask=mask, P=P, max_pods=max_pods, B=B, R=R,
                k=k, coarse=coarse, lists0=lists0)


def _info(c):
    return (f"seed {c['seed']}: chain {c['chain']} P {c['P']} max_pods {c['max_pods']} B {c['B']} R {c['R']} k {c['k']} "
            f"masked {c['mask'] is not None} holes {int((c['pods']['flags'] & 1).sum())} coarse {c['coarse']} slots {c['slots']} "
            f"lists {'off' if c['lists0'] else 'on'}")


def _case_totals(orc, c):
    oix = orc.OracleIndex()
    if c["B"] and c["ih"].size:
        oix.insert(c["ih"], c["ip"], snapshot=c["pods"])   # (pairs that name a hole are ignored, like on the device)
    return _totals(orc, c["chain"], c["pods"], oix, c["reqs"], c["mask"])


def _run_case(pkg, orc, ref, monkeypatch, c):
    import torch
    if c["lists0"]:
        monkeypatch.setenv("EPPK_LISTS", "0")
    T = _case_totals(orc, c)
    R, k = c["R"], c["k"]
    with pkg.BatchedPicker(c["chain"], max_pods=c["max_pods"], max_blocks=c["B"], max_batch=R, index_slots=c["slots"] if c["B"] else 0) as pk:
        pk.publish(c["pods"])
        if c["B"] and c["ih"].size:
            pk.index_insert(c["ih"], c["ip"])
        for seed in (0, HIGH):
            got = pk.pick_weighted_random(c["reqs"], seed, k, c["mask"])
            _same(got, ref.weighted_random(T, k, seed, np.arange(R)), _info(c) + f" rng seed {seed:#x}")
        # the device entry point without a score output: the same picks
        d_reqs = torch.from_numpy(c["reqs"].view(np.int64)).cuda()
        d_mask = None if c["mask"] is None else torch.from_numpy(np.ascontiguousarray(c["mask"]).view(np.int64)).cuda()
        d_pick = torch.full((R * k,), -7, dtype=torch.int32, device="cuda")
        pk.pick_weighted_random_device(d_reqs.data_ptr(), R, None if d_mask is None else d_mask.data_ptr(), k, HIGH, d_pick.data_ptr(), None)
        torch.cuda.synchronize()
        assert pk.launch_status() == 0, _info(c)
        dp = d_pick.cpu().numpy().reshape(R, k)
        bad = np.nonzero(np.any(dp != got[0], axis=1))[0]
        assert bad.size == 0, _info(c) + f" device entry point without scores: rows {bad[:5]}"


@gpu
@pytest.mark.parametrize("seed", range(N_SEEDS))
def test_fuzz_weighted_random(pkg, orc, ref, monkeypatch, seed):
    _run_case(pkg, orc, ref, monkeypatch, _case(pkg, 7000 + seed))


def test_the_generator_covers_what_the_fuzz_is_for(pkg, orc):
    """No GPU: the generator and the oracle's totals alone.  What test_fuzz_weighted_random is relied on for must be IN its cases:
    every (lane word, counter planes, masked) instantiation of the kernel in at least 4 of them; the lane words that a `max_pods`
    above the pods' own class can select (u32, u64 -- nothing is below u16) reached that way; each route of the rule -- S == 0
    from round 0, positive candidates exhausted before the last round, 0 < |C| < k, no candidate -- in at least 2 % of all rows;
    and the chain shapes the kernel's staging of the leading run depends on.  A row's route follows from its totals alone
    (S is a sum of the positive totals: S == 0 iff there is none), so the totals are classified, one row per (case, seed) pair.
    Measured with these 260 seeds (53 236 rows): S == 0 at round 0 in 34.0 %, positives exhausted mid-list 5.1 % (the generator's
    rows of 1..12 pods are there for this route), padded 9.3 %, no candidate 6.2 %; the rarest instantiation (u32, 9 planes,
    masked) in 10 cases; 53 empty or all-zero chains, 107 with QUEUE / KV behind LORA / PREFIX, 24 masked + QUEUE + coarse."""
    inst = {}
    upclass = set()
    rows = dict(s0=0, switch=0, padded=0, none=0)
    n_rows = 0
    zero_chain = behind = masked_q_coarse = 0
    for s in range(N_SEEDS):
        c = _case(pkg, 7000 + s)
        key = (LW_NAME[_lw_class(c["max_pods"])], 6 if c["B"] <= 63 else 9, c["mask"] is not None)
        inst[key] = inst.get(key, 0) + 1
        if _lw_class(c["max_pods"]) > _lw_class(c["P"]):
            upclass.add(key[0])
        kinds = [kd for kd, _ in c["chain"]]
        zero_chain += all(w == 0 for _, w in c["chain"])
        behind += any(kd in (Q, KV) and any(e in (L, PF) for e in kinds[:i]) for i, kd in enumerate(kinds))
        masked_q_coarse += c["mask"] is not None and Q in kinds and c["coarse"]
        T = _case_totals(orc, c)
        cand = ~np.isnan(T)
        n = cand.sum(axis=1)
        pos = (cand & (np.where(cand, T, 0.0) > 0.0)).sum(axis=1)
        k = c["k"]
        n_rows += 2 * c["R"]                                # (both seeds of the case see the same totals)
        rows["none"] += 2 * int((n == 0).sum())
        rows["padded"] += 2 * int(((n > 0) & (n < k)).sum())
        rows["s0"] += 2 * int(((n > 0) & (pos == 0)).sum())
        rows["switch"] += 2 * int(((pos > 0) & (pos < np.minimum(n, k))).sum())
    shares = {kk: v / n_rows for kk, v in rows.items()}
    what = f"rows {n_rows} shares {shares} instantiations {inst} wider-class {sorted(upclass)} zero-chain {zero_chain} " \
           f"Q/KV behind L/PF {behind} masked+QUEUE+coarse {masked_q_coarse}"
    print(what)
    for lw in LW_NAME:
        for npl in (6, 9):
            for m in (False, True):
                assert inst.get((lw, npl, m), 0) >= 4, what
    assert upclass == {"u32", "u64"}, what
    for kk, v in shares.items():
        assert v >= 0.02, what
    assert zero_chain >= 5 and behind >= 10 and masked_q_coarse >= 10, what


# ---- every instantiation, named ------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("npl", [6, 9])
@pytest.mark.parametrize("lw", [0, 1, 2], ids=LW_NAME)
def test_every_instantiation_at_its_edges(pkg, orc, ref, lw, npl, masked):
    """pick_wrand_kernel<lane word, counter planes, MASKED> at the top of its pod range and at its bottom (one pod for u16: 63 of 64
    lanes own nothing), the largest block count of 6 planes, the smallest and the largest of 9; k = 8 on subsets of 1..12 pods pads
    in some rows and not in others."""
    R, k = 300, 8
    for P in (LW_TOP[lw], 1 if lw == 0 else LW_TOP[lw - 1] + 1):
        for B in ((63,) if npl == 6 else (64, 256)):
            wl = pkg.workload.make_workload(3, R=R, P=P, B=B, seed=0xED6E + P + B)
            # the workload's index holds the shared half of every prompt; the first 8 prompts are cached whole on two pods each (a
            # prefix count of B itself: the top counter plane), and every fifth request is shorter than B blocks
            ih = np.concatenate([wl.index_hashes, np.repeat(wl.reqs[:8, 1:].reshape(-1), 2)])
            ip = np.concatenate([wl.index_pods, np.tile(np.array([[(7 * r) % P, (7 * r + P // 2) % P] for r in range(8)], dtype=np.uint32)[:, None, :],
                                                        (1, B, 1)).reshape(-1)])
            nb = np.where(np.arange(R) % 5 == 4, np.arange(R) % (B + 1), B)
            reqs = pkg.picker.make_req_rows(wl.adapter, nb, wl.reqs[:, 1:], B)
            oix = orc.OracleIndex()
            oix.insert(ih, ip)
            mask = _subset_mask(np.random.default_rng(P * 1000 + B), R, P, 1, 12, every=2) if masked else None
            for chain in (BASE, NEG, MIX):
                T = _totals(orc, chain, wl.pods, oix, reqs, mask)
                with pkg.BatchedPicker(chain, max_pods=LW_TOP[lw], max_blocks=B, max_batch=R, index_slots=2 * wl.index_slots) as pk:
                    pk.publish(wl.pods)
                    pk.index_insert(ih, ip)
                    got = pk.pick_weighted_random(reqs, HIGH, k, mask)
                _same(got, ref.weighted_random(T, k, HIGH, np.arange(R)),
                      f"pick_wrand_kernel<{LW_NAME[lw]}, {npl}, {masked}> P {P} B {B} chain {chain}")


# ---- launch geometry -----------------------------------------------------------------------------------------------------------------

def _sane_rows(picks, cand_bits, P, what):
    """Every row: entries distinct, each a candidate, -1 only as padding (behind min(k, |C|) picks)."""
    R, k = picks.shape
    n = np.full(R, P) if cand_bits is None else cand_bits.sum(axis=1)
    for r in range(R):
        row = picks[r]
        m = min(k, int(n[r]))
        assert np.all(row[:m] >= 0) and np.all(row[:m] < P) and np.all(row[m:] == -1), f"{what} row {r}: {row} with {n[r]} candidates"
        assert np.unique(row[:m]).size == m, f"{what} row {r}: {row}"
        if cand_bits is not None:
            assert np.all(cand_bits[r, row[:m]]), f"{what} row {r}: {row} not all candidates"


@gpu
@pytest.mark.parametrize("shape", ["P4096_B256", "P65_B5_masked"])
def test_launch_geometry(pkg, orc, ref, shape):
    """Batches of 0, 1, 15, 16, 17 requests (16 wavefronts = one workgroup) and one of more requests than the persistent grid has
    wavefronts (16 per workgroup; a compute unit holds 32 wavefronts, so at most 2 workgroups on each of 256 units), so that every
    wavefront loops -- on the shape with the largest LDS footprint and on a small masked one.  The oracle scores a sample of the
    large batch (first 64, last 64, 256 evenly spaced); every row is checked for distinct candidates and padding."""
    import torch
    big = 16 * 2 * 256 + 16 * 5 + 3
    P, B, masked = (4096, 256, False) if shape == "P4096_B256" else (65, 5, True)
    k, seed = 4, HIGH + 5
    wl = pkg.workload.make_workload(3, R=big, P=P, B=B, seed=0x6E0 + P)
    chain = NEG if masked else BASE
    oix = orc.OracleIndex()
    oix.insert(wl.index_hashes, wl.index_pods)
    mask = _subset_mask(np.random.default_rng(P), big, P, 0, 9, every=3) if masked else None
    bits = _mask_bits(mask, P) if masked else None
    with pkg.BatchedPicker(chain, max_pods=P, max_blocks=B, max_batch=big, index_slots=wl.index_slots) as pk:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        # no request: EPPK_OK and nothing written, on both entry points
        picks = np.full(8, -7, dtype=np.int32)
        scores = np.full(8, -7.0)
        assert pk._lib.eppk_pick_weighted_random(pk._ctx, wl.reqs.ctypes.data, 0, None, k, seed, picks.ctypes.data, scores.ctypes.data) == 0
        assert np.all(picks == -7) and np.all(scores == -7.0)
        d_reqs = torch.from_numpy(wl.reqs.view(np.int64)).cuda()
        d_mask = torch.from_numpy(mask.view(np.int64)).cuda() if masked else None
        d_pick = torch.full((big * k,), -7, dtype=torch.int32, device="cuda")
        d_score = torch.full((big * k,), -7.0, dtype=torch.float64, device="cuda")
        mptr = d_mask.data_ptr() if masked else None
        pk.pick_weighted_random_device(d_reqs.data_ptr(), 0, mptr, k, seed, d_pick.data_ptr(), d_score.data_ptr())
        torch.cuda.synchronize()
        assert bool((d_pick == -7).all()) and bool((d_score == -7.0).all())
        for R in (1, 15, 16, 17, big):
            what = f"{shape} R {R}"
            m = None if mask is None else mask[:R]
            got = pk.pick_weighted_random(wl.reqs[:R], seed, k, m)
            rows = np.arange(R) if R <= 384 else np.unique(np.concatenate([np.arange(64), np.arange(R - 64, R), np.linspace(0, R - 1, 256).astype(np.int64)]))
            T = _totals(orc, chain, wl.pods, oix, wl.reqs[rows], None if m is None else m[rows])
            _same((got[0][rows], got[1][rows]), ref.weighted_random(T, k, seed, rows), what)
            _sane_rows(got[0], None if bits is None else bits[:R], P, what)
            # the host entry point without a score output, and the device one (a launch of exactly R rows into sentinel-filled arrays)
            hp = np.full((R, k), -7, dtype=np.int32)
            assert pk._lib.eppk_pick_weighted_random(pk._ctx, wl.reqs.ctypes.data, R, None if m is None else m.ctypes.data, k, seed, hp.ctypes.data, None) == 0
            assert np.array_equal(hp, got[0]), what + " host entry point without scores"
            d_pick.fill_(-7); d_score.fill_(-7.0)
            pk.pick_weighted_random_device(d_reqs.data_ptr(), R, mptr, k, seed, d_pick.data_ptr(), d_score.data_ptr())
            torch.cuda.synchronize()
            dp = d_pick.cpu().numpy().reshape(big, k)
            ds = d_score.cpu().numpy().reshape(big, k)
            assert np.array_equal(dp[:R], got[0]) and np.array_equal(ds[:R].view(np.uint64), got[1].view(np.uint64)), what + " device entry point"
            assert np.all(dp[R:] == -7) and np.all(ds[R:] == -7.0), what + " wrote behind its last row"
        assert pk.launch_status() == 0


# ---- behind index maintenance --------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("mode", ["default", "quadmin4"])
@pytest.mark.parametrize("seed", range(30))
def test_weighted_random_after_index_maintenance(pkg, orc, ref, monkeypatch, seed, mode):
    """The operation loop of test_gpu_fuzz.test_fuzz_index_maintenance (bulk insert, learn from picks, pod removal, epoch tick +
    eviction, republish with holes, per-pod trim) with this picker as the probe after every step, and as the teacher: the learn step
    inserts round 0 of a weighted-random batch, what a scheduler on this picker does.  EPPK_QUAD_MIN=4: the index is kept canonical
    for the quad route."""
    import torch
    if mode == "quadmin4":
        monkeypatch.setenv("EPPK_QUAD_MIN", "4")
    rng = np.random.default_rng(9000 + seed)
    P = int(rng.choice([40, 300, 1500, 4096]))
    B = int(rng.choice([4, 8, 16]))
    chain = [[(KV, 1), (PF, 5)], [(Q, 1), (KV, 2), (L, 1), (PF, 4)], [(PF, 3), (KV, -1)], [(PF, 2), (Q, 1), (PF, 1)]][seed % 4]
    pods = pkg.workload.make_pods(int(rng.integers(1, 1 << 30)), P, 128)
    universe = rng.integers(1, 2**63, (24, B), dtype=np.uint64)          # 24 chains of B blocks
    R, k = 96, 3

    def probe_batch():
        hs = universe[rng.integers(0, universe.shape[0], R)].copy()
        for r in range(R):
            if rng.random() < 0.5:
                cut = int(rng.integers(0, B))
                hs[r, cut:] = rng.integers(1, 2**63, B - cut, dtype=np.uint64)
        return pkg.picker.make_req_rows(rng.integers(-1, 128, R), np.full(R, B), hs, B)

    with pkg.BatchedPicker(chain, max_pods=P, max_blocks=B, max_batch=R, index_slots=8192) as pk:
        pk.publish(pods)
        oix = orc.OracleIndex()
        for step in range(14):
            op = rng.choice(["insert", "insert", "insert_picks", "remove_pod", "tick_evict", "republish", "trim"])
            what = f"seed {seed} mode {mode} P {P} B {B} chain {chain} step {step} after {op}"
            if op == "insert":
                ci = rng.integers(0, universe.shape[0], 3)
                ih = np.concatenate([universe[c, : int(rng.integers(1, B + 1))] for c in ci])
                ip = rng.integers(0, P, ih.size).astype(np.uint32)
                pk.index_insert(ih, ip); oix.insert(ih, ip, snapshot=pods)
            elif op == "republish":                         # endpoint churn: some slots become holes, some holes are handed out again
                pods = pods.copy()
                flip = rng.random(P) < 0.15
                pods["flags"] = np.where(flip, pods["flags"] ^ 1, pods["flags"]).astype(np.uint32)
                pods["queue"] = rng.integers(0, 64, P)
                pk.publish(pods); oix.scrub_inactive(pods)
            elif op == "insert_picks":                      # learn round 0 of a weighted-random batch
                reqs = probe_batch()
                lseed = int(rng.integers(0, 2**63))
                picks, scores = pk.pick_weighted_random(reqs, lseed, k)
                want = ref.weighted_random(_totals(orc, chain, pods, oix, reqs), k, lseed, np.arange(R))
                _same((picks, scores), want, what + " (the batch that is learnt)")
                d_reqs = torch.from_numpy(reqs.view(np.int64)).cuda()
                d_picks = torch.from_numpy(np.ascontiguousarray(picks[:, 0])).cuda()
                pk.index_insert_picks_device(d_reqs.data_ptr(), d_picks.data_ptr(), R)
                torch.cuda.synchronize()
                oix.insert_picks(reqs, B, np.ascontiguousarray(want[0][:, 0]))
            elif op == "trim":                              # per-pod capacity, oldest epochs first (SEMANTICS.md §6c)
                cap = int(rng.integers(1, 12))
                assert pk.index_trim_pods(cap) == oix.trim_pods(P, cap), what
            elif op == "remove_pod":
                pod = int(rng.integers(0, P))
                pk.index_remove_pod(pod); oix.remove_pod(pod)
            else:
                e = pk.index_advance_epoch(); eo = oix.advance_epoch()
                assert e == eo
                keep = int(rng.integers(1, 3))
                assert pk.index_evict_older(max(e - keep, 0)) == oix.evict_older(max(e - keep, 0)), what
            assert pk.index_dropped() == 0
            assert pk.index_size() == oix.size(), what
            assert pk.index_selfcheck() == 0, what
            reqs = probe_batch()
            pseed = int(rng.integers(0, 2**64, dtype=np.uint64))
            got = pk.pick_weighted_random(reqs, pseed, k)
            _same(got, ref.weighted_random(_totals(orc, chain, pods, oix, reqs), k, pseed, np.arange(R)), what)


# ---- the descent at exact boundaries -------------------------------------------------------------------------------------------------
# A random word never makes x EQUAL a node sum, and never makes the rounding of x - A matter; the rule (SEMANTICS.md §3c step 6) says
# what happens there, so these cases choose the word: splitmix64 is a bijection, and the seed that gives request 0 a wanted word in
# round 0 is its inverse minus the golden-ratio step.

def _unmix(u):
    """The inverse of splitmix64's mixer (SEMANTICS.md §3b) on Python ints."""
    M = (1 << 64) - 1
    u ^= u >> 31; u ^= u >> 62
    u = u * pow(0x94D049BB133111EB, -1, 1 << 64) & M
    u ^= u >> 27; u ^= u >> 54
    u = u * pow(0xBF58476D1CE4E5B9, -1, 1 << 64) & M
    u ^= u >> 30; u ^= u >> 60
    return u


def _seed_for(u):
    """The seed under which round 0 of request 0 draws the word u."""
    return (_unmix(u) - 0x9E3779B97F4A7C15) & ((1 << 64) - 1)


def _descend_as(ref, w, x, rule):
    """wrand_ref.descend for one row with the comparison of the rule, or one of two wrong ones."""
    lv = ref.tree(w)
    q = 0
    for m in range(ref.LEVELS - 1, -1, -1):
        a, b = lv[m][0, 2 * q], lv[m][0, 2 * q + 1]
        left = {"rule": b == 0.0 or x < a, "x <= A": b == 0.0 or x <= a, "no B == 0": x < a}[rule]
        if not left:
            x = x - a
        q = 2 * q + (0 if left else 1)
    return 64 * (q % 64) + q // 64


def _boundary_cases(pkg):
    """(name, chain, pods, candidates, word, the wrong rule this case tells from the right one).  64 pods; pod 0 is the first leaf of
    the root's left half, pod 32 the first leaf of its right half (a left child at every level below the root)."""
    def pods(queue, kv):
        p = pkg.workload.make_pods(77, 64, 128)
        p["queue"] = 3
        p["kv_util"] = 0.25
        for i, (q, v) in enumerate(zip(queue, kv)):
            p["queue"][32 * i] = q
            p["kv_util"][32 * i] = v
        return p
    low = 0x5A5
    return [
        # two equal weights: S = 2, x = S / 2 = A exactly -> NOT x < A: right, to pod 32
        ("x == A", [(KV, 2)], pods((3, 3), (0.5, 0.5)), (0, 32), (1 << 63) | low, "x <= A"),
        # x = 0 over a left half that weighs 0 (pod 0: total 0, a candidate all the same): 0 < 0 is false -> right
        ("x == 0 == A", [(KV, 2)], pods((3, 3), (1.0, 0.5)), (0, 32), low, "x <= A"),
        # A = 3 * 2^-53 left, B = 1.9375 right, the largest word: x = pred(S) and x - A rounds UP to B exactly; every node below the
        # root has pod 32's leaf on the left and 0.0 on the right: "B == 0 -> left" is what keeps the descent on the pod
        ("x - A rounds to B", [(Q, 1), (KV, 1)], pods((5, 0), (1.0 - 3 * 2.0 ** -53, 0.0625)), (0, 32), ((1 << 53) - 1) << 11 | low, "no B == 0"),
    ]


def _boundary_setup(pkg, orc, ref, case, how):
    name, chain, pods, cands, u, wrong = case
    reqs = pkg.picker.make_req_rows(np.array([-1]), np.array([0]), None, 0)
    mask = None
    pods = pods.copy()
    if how == "masked":
        mask = np.array([[sum(1 << c for c in cands)]], dtype=np.uint64)
    else:                                                  # every other slot a hole (SEMANTICS.md §6b)
        pods["flags"] = 1
        pods["flags"][list(cands)] = 0
    T = _totals(orc, chain, pods, None, reqs, mask)
    return chain, pods, reqs, mask, T, _seed_for(u), u, wrong


@pytest.mark.parametrize("how", ["masked", "holes"])
@pytest.mark.parametrize("case", range(3))
def test_boundary_cases_are_live(pkg, orc, ref, case, how):
    """No GPU: under the seed computed for it the reference draws the wanted word, and its pick differs from what the named wrong
    comparison would pick -- so the GPU test below tells them apart."""
    chain, pods, reqs, mask, T, seed, u, wrong = _boundary_setup(pkg, orc, ref, _boundary_cases(pkg)[case], how)
    assert int(ref.words(seed, [0], 0)[0]) == u
    cand = ~np.isnan(T)
    w = np.where(cand & (np.where(cand, T, 0.0) > 0.0), T, 0.0)
    S = ref.tree(w)[ref.LEVELS][0, 0]
    x = ((u >> 11) * 2.0 ** -53) * S
    want = ref.weighted_random(T, 1, seed, [0])[0][0, 0]
    assert _descend_as(ref, w, x, "rule") == want == 32
    assert _descend_as(ref, w, x, wrong) != want, (wrong, T[0, [0, 32]])


@gpu
@pytest.mark.parametrize("max_pods", [64, 4096])
@pytest.mark.parametrize("how", ["masked", "holes"])
@pytest.mark.parametrize("case", range(3))
def test_descent_at_exact_boundaries(pkg, orc, ref, case, how, max_pods):
    """x equal to a node sum, x = 0 over an empty left half, and x - A rounding up to B over nodes whose right child is 0.0: the
    words are chosen (see _seed_for), two candidates among 64 pods, by mask and by holes, narrowest and widest lane word; k = 2, so
    that the second round runs on what the first left behind."""
    c = _boundary_cases(pkg)[case]
    chain, pods, reqs, mask, T, seed, u, wrong = _boundary_setup(pkg, orc, ref, c, how)
    with pkg.BatchedPicker(chain, max_pods=max_pods, max_blocks=0, max_batch=4, index_slots=0) as pk:
        pk.publish(pods)
        got = pk.pick_weighted_random(reqs, seed, 2, mask)
    _same(got, ref.weighted_random(T, 2, seed, [0]), f"{c[0]} ({how}, max_pods {max_pods}); the comparison '{wrong}' picks another pod")
