"""No GPU: tests/value_cases.py (snapshot values at the edges of their types) held to the coverage tests/test_gpu_values.py relies on
over the same seeds; and the oracle held to the independent numpy restatement (tests/golden/gen_golden.py) on those cases, bit for
bit: the reference is pinned at these values where the kernels are held to it."""
import importlib.util
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


vc = _load("value_cases", "value_cases.py")
SEEDS = [vc.SEED0 + i for i in range(vc.N_SEEDS)]
SMALL = [s for s in SEEDS if vc.pods_of(s) <= 200]


@pytest.fixture(scope="module")
def gg():
    return _load("gen_golden", "golden", "gen_golden.py")


def _oracle_index(orc, c):
    oix = orc.OracleIndex()
    if c["B"] and c["ih"].size:
        oix.insert(c["ih"], c["ip"], snapshot=c["pods"])
    return oix


def test_fused_kind_on_the_chains_the_library_is_known_to_classify():
    """The (chain, kind) table of test_gpu_parity.test_which_kernel_serves_a_chain, which the GPU suite holds the library to."""
    Q, KV, L, PF = vc.Q, vc.KV, vc.L, vc.PF
    for chain, kind in [([(Q, 2), (KV, 2), (L, 1), (PF, 3)], 1), ([(PF, 3), (L, 1)], 1), ([(PF, 3), (KV, 5)], 2),
                        ([(L, 1), (Q, 2), (PF, 3), (KV, 2)], 2), ([(L, 1), (Q, 2), (KV, 2), (Q, 1), (PF, 3)], 0), ([(PF, 3), (Q, 1), (PF, 3)], 0),
                        ([], 1), ([(Q, 1)] * 8, 1), ([(Q, 1)] * 4 + [(L, 1), (PF, 1), (Q, 1), (KV, 1)], 2), ([(L, 1), (PF, 1), (Q, 1), (KV, 1), (Q, 1)], 0)]:
        assert vc.fused_kind(chain) == kind, chain


def test_the_generator_covers_what_the_gpu_module_is_for(orc, gg):
    """Over the seeds SEED0 .. SEED0 + N_SEEDS - 1: every queue / kv_util mode, every max_lora value, every weight, every
    chain length 0..8, fused chains of 7 and 8 entries (and interpreted tails of 7 and 8), chains the library does not fuse, an
    all-zero and an all-negative chain; a masked row whose candidates span 2^31 and more of queue; a row that lost every pod at a
    snapshot-wide queue extreme and one that kept both; winning totals that are negative and exactly +0.0; every special kv_util
    value and the LoRA seams on some pod; and a total that depends on the order of the chain's additions."""
    qmodes, kvmodes, plans, lengths, weights, loras = set(), set(), set(), set(), set(), set()
    fused_len, tail_len, kinds = set(), set(), set()
    kv_specials = set()
    wide_masked = lost_extreme = kept_extremes = negative_win = zero_win = order_matters = 0
    full_sets = empty_sets = zero_lora_full = 0
    adapters = set()
    shapes = set()
    for s in SEEDS:
        c = vc.make_case(s)
        what = vc.info(c)
        assert vc.fused_kind(c["chain"]) == c["kind"], what
        assert c["R"] <= 200 and len(c["chain"]) <= 8, what
        qmodes.add(c["qmode"]); kvmodes.add(c["kvmode"]); plans.add(c["plan"]); lengths.add(len(c["chain"]))
        weights.update(w for _, w in c["chain"]); loras.update(c["pods"]["max_lora"].tolist())
        kinds.add(c["kind"]); shapes.add((c["P"], c["B"]))
        if c["kind"] == 1:
            fused_len.add(len(c["chain"]))
        if c["kind"] == 2:
            tail_len.add(len(c["chain"]))
        if c["kvmode"] == "b":
            kv_specials.update(c["pods"]["kv_util"].view(np.uint64).tolist())
        act, wai = c["pods"]["active"], c["pods"]["waiting"]
        ones = np.uint64(0xFFFFFFFFFFFFFFFF)
        full = (act == ones).all(axis=1) | (wai == ones).all(axis=1)
        full_sets += int(full.sum()); empty_sets += int(((act == 0).all(axis=1) & (wai == 0).all(axis=1)).sum())
        zero_lora_full += int((full & (c["pods"]["max_lora"] == 0)).sum())
        adapter, n_blocks, hashes = vc.request_fields(c)
        adapters.update(adapter.tolist())
        live = (c["pods"]["flags"] & 1) == 0
        q = c["pods"]["queue"].astype(np.int64)
        if c["mask"] is not None:
            bits = vc.mask_bits(c["mask"], c["P"]) & live[None, :]
            assert not bits[0].any() and (c["R"] < 2 or bits[1].sum() <= 1), what
            has = bits.any(axis=1)
            hi = np.where(bits, q[None, :], -1).max(axis=1)
            lo = np.where(bits, q[None, :], 1 << 40).min(axis=1)
            wide_masked += int((has & (hi - lo >= 1 << 31)).sum())
            qlo, qhi = q[live].min(), q[live].max()
            if qhi > qlo:
                lost_extreme += int((has & ((lo > qlo) | (hi < qhi))).sum())
                kept_extremes += int((has & (lo == qlo) & (hi == qhi)).sum())
        picks, scores, _ = orc.pick_batch(c["chain"], c["pods"], _oracle_index(orc, c), c["reqs"], c["B"], c["mask"])
        won = picks >= 0
        negative_win += int((won & (scores < 0.0)).sum())
        zero_win += int((won & (scores == 0.0) & ~np.signbit(scores)).sum())
        if c["P"] <= 200 and len(c["chain"]) >= 2:
            idx = vc.index_dict(c)
            fwd, cand = gg.numpy_totals(c["chain"], c["pods"], idx, adapter, n_blocks, hashes, c["mask"])
            rev, _ = gg.numpy_totals(c["chain"][::-1], c["pods"], idx, adapter, n_blocks, hashes, c["mask"])
            order_matters += int((cand & (fwd.view(np.uint64) != rev.view(np.uint64)) & (fwd != rev)).sum())
    what = (f"lengths {sorted(lengths)} fused {sorted(fused_len)} tails {sorted(tail_len)} weights {sorted(weights)} max_lora {sorted(loras)} "
            f"rows: wide masked {wide_masked} lost an extreme {lost_extreme} kept both {kept_extremes} negative win {negative_win} "
            f"+0.0 win {zero_win}; totals that depend on the order {order_matters}; pods with a full set {full_sets} "
            f"(max_lora 0: {zero_lora_full}) with empty sets {empty_sets}; shapes {len(shapes)}")
    print(what)
    assert qmodes == set(vc.QUEUE_MODES) and kvmodes == set(vc.KV_MODES) and plans == set(vc.CHAIN_PLANS), what
    assert loras == set(vc.MAX_LORAS) and weights == set(vc.WEIGHTS) and lengths == set(range(9)), what
    assert {7, 8} <= fused_len and {7, 8} <= tail_len and kinds == {0, 1, 2}, what
    assert kv_specials == set(np.array(vc.KV_SPECIALS).view(np.uint64).tolist()), what
    assert set(vc.SEAM_ADAPTERS) <= adapters, what
    assert {p for p, _ in shapes} == set(vc.PODS) and {b for _, b in shapes} == set(vc.BLOCKS), what
    assert wide_masked >= 1 and lost_extreme >= 1 and kept_extremes >= 1, what
    assert negative_win >= 1 and zero_win >= 1 and order_matters >= 1, what
    assert full_sets >= 1 and empty_sets >= 1 and zero_lora_full >= 1, what


def test_the_once_per_mode_cases_cover_every_mode():
    assert {q for q, _ in vc.VALUE_MODES} == set(vc.QUEUE_MODES) and {k for _, k in vc.VALUE_MODES} == set(vc.KV_MODES)


def test_the_quad_route_is_reached_by_enough_cases():
    """The cases that take pick_quad_kernel under EPPK_QUAD_MIN=4 (value_cases.quad_route_exists): enough of them, with masks and
    without, in every queue and kv_util mode."""
    cs = [c for c in (vc.make_case(s) for s in SEEDS) if vc.quad_route_exists(c)]
    what = f"{len(cs)} cases: {sorted((c['qmode'], c['kvmode'], c['mask'] is not None) for c in cs)}"
    assert len(cs) >= 12 and {c["qmode"] for c in cs} == set(vc.QUEUE_MODES) and {c["kvmode"] for c in cs} == set(vc.KV_MODES), what
    assert {c["mask"] is not None for c in cs} == {False, True}, what


@pytest.mark.parametrize("seed", SMALL)
def test_oracle_equals_the_numpy_restatement_at_these_values(orc, gg, seed):
    """oracle/oracle.c (per-request loops) against tests/golden/gen_golden.py (whole matrices) on the cases with P <= 200: picks,
    scores and ordered fallbacks, bit for bit."""
    c = vc.make_case(seed)
    what = vc.info(c)
    adapter, n_blocks, hashes = vc.request_fields(c)
    idx = vc.index_dict(c)
    oix = _oracle_index(orc, c)
    op, osc, _ = orc.pick_batch(c["chain"], c["pods"], oix, c["reqs"], c["B"], c["mask"])
    with np.errstate(invalid="ignore", over="ignore"):
        npk, nsc = gg.numpy_pick(c["chain"], c["pods"], idx, adapter, n_blocks, hashes, c["mask"])
        ntp, nts = gg.numpy_topk(c["chain"], c["pods"], idx, adapter, n_blocks, hashes, c["mask"], c["k"])
    assert np.array_equal(op, npk), what + f" rows {np.nonzero(op != npk)[0][:5]}"
    assert np.array_equal(osc.view(np.uint64), nsc.view(np.uint64)), what
    otp, ots = orc.pick_topk(c["chain"], c["pods"], oix, c["reqs"], c["k"], c["mask"])
    assert np.array_equal(otp, ntp), what + f" topk {c['k']}"
    assert np.array_equal(ots.view(np.uint64), nts.view(np.uint64)), what + f" topk {c['k']}"
    btp, bts = orc.pick_topk_batch(c["chain"], c["pods"], oix, c["reqs"], c["B"], c["k"], c["mask"])
    assert np.array_equal(btp, otp) and np.array_equal(bts.view(np.uint64), ots.view(np.uint64)), what + " (orc_pick_topk)"


@pytest.mark.parametrize("block_chars", [8, 16, 24, 32, 40, 56, 64, 72, 128])
def test_host_hashing_equals_xxhash_at_every_block_size(pkg, orc, block_chars):
    """The host reference of hash_prompts_kernel (picker.hash_prompt, eppk_xxh64) against python-xxhash, an independent XXH64: messages
    of block_chars + 8 bytes per link of the chain -- 2 and 3 words (the short path below four), 4 (one stripe), 5, 6 (a stripe and
    tail words), 8 .. 17 (several stripes) -- and prompts of k * block_chars - 1, k * block_chars, k * block_chars + 1 bytes, some longer
    than max_blocks blocks.  Where python-xxhash is not installed the oracle's own XXH64 (oracle/oracle.c) stands in: the test never skips."""
    try:
        import xxhash
        ref64 = lambda data, seed: xxhash.xxh64(data, seed=seed).intdigest()
    except ImportError:
        ref64 = orc.xxh64
    lib = pkg.load_library()
    rng = np.random.default_rng(block_chars)
    B = 6
    for n in sorted({n for k in range(8) for n in (k * block_chars - 1, k * block_chars, k * block_chars + 1) if n >= 0}):
        prompt = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        for seed in (0, 0x9E3779B97F4A7C15):
            assert lib.eppk_xxh64(prompt, n, seed) == ref64(prompt, seed), (n, seed)
        prev = ref64(b"adapter-63", 0)
        want = []
        for i in range(min(n // block_chars, B)):
            prev = ref64(prompt[i * block_chars:(i + 1) * block_chars] + prev.to_bytes(8, "little"), 0)
            want.append(prev)
        got = pkg.picker.hash_prompt(b"adapter-63", prompt, block_chars, B)
        assert got.tolist() == want, (block_chars, n)
