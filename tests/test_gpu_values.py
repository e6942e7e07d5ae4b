"""The pick kernels held to the oracle on SNAPSHOT values at the edges of their types (tests/value_cases.py): queue over all of u32,
kv_util with a full mantissa / NaN / +-inf / -0.0 / subnormal, max_lora 0 .. 2^32 - 1 with full and empty adapter sets, chains of 0..8
scorers with weights up to +-(2^31 - 1).  Picks as int32, scores as uint64, no tolerance, no case filtered out.  Every seed through
pick / pick_topk in the four library modes (this module sets the switches itself: conftest's MODE_MODULES does not list it); the other
entry points once per value mode; republish; assumed load wrapping at 2^32 - 1; every (lane word, planes, masked) instantiation; and
hash_prompts_kernel at every path of its block loop.  tests/test_value_cases_cpu.py holds the generator to its coverage and the oracle
to the numpy restatement on the same seeds."""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


vc = _load("value_cases")
SEEDS = [vc.SEED0 + i for i in range(vc.N_SEEDS)]
MODES = {"default": {}, "quadmin4": {"EPPK_QUAD_MIN": "4"}, "quad0": {"EPPK_QUAD": "0"}, "lists0": {"EPPK_LISTS": "0"}}
LW_TOP = (1024, 2048, 4096)                           # the largest max_pods of the lane words u16 / u32 / u64
LW_NAME = ("u16", "u32", "u64")
HIGH = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def ref():
    return _load("wrand_ref")


@pytest.fixture
def library_mode(request, monkeypatch):
    for name in ("EPPK_QUAD_MIN", "EPPK_QUAD", "EPPK_LISTS"):
        monkeypatch.delenv(name, raising=False)
    for name, value in MODES[request.param].items():
        monkeypatch.setenv(name, value)
    return request.param


def _oracle_index(orc, c, pods=None):
    oix = orc.OracleIndex()
    if c["B"] and c["ih"].size:
        oix.insert(c["ih"], c["ip"], snapshot=c["pods"] if pods is None else pods)
    return oix


def _picker(pkg, c, max_pods=None, max_batch=None):
    pk = pkg.BatchedPicker(c["chain"], max_pods=max_pods or c["P"], max_blocks=c["B"], max_batch=max_batch or c["R"],
                           index_slots=c["slots"] if c["B"] else 0)
    pk.publish(c["pods"])
    if c["B"] and c["ih"].size:
        pk.index_insert(c["ih"], c["ip"])
    return pk


def _same(got, want, what):
    gp, gs = np.asarray(got[0]), np.asarray(got[1])
    wp, ws = np.asarray(want[0]), np.asarray(want[1])
    assert gp.shape == wp.shape, what
    bad = np.nonzero((gp != wp).reshape(gp.shape[0], -1).any(axis=1))[0]
    assert bad.size == 0, f"{what}: picks of {bad.size} rows differ, first {bad[:5]}: gpu {gp[bad[:3]]} oracle {wp[bad[:3]]}"
    sbad = np.nonzero((gs.view(np.uint64) != ws.view(np.uint64)).reshape(gs.shape[0], -1).any(axis=1))[0]
    assert sbad.size == 0, f"{what}: scores of {sbad.size} rows differ, first {sbad[:5]}: gpu {gs[sbad[:3]]!r} oracle {ws[sbad[:3]]!r}"


def _totals(orc, c, oix):
    """[R, P] totals of the oracle (NaN = not a candidate)."""
    return np.stack([orc.score_row(c["chain"], c["pods"], oix, c["reqs"][r], None if c["mask"] is None else c["mask"][r]) for r in range(c["R"])])


# ---- every seed, four library modes ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=8)
def _want(orc, seed):
    """The case of `seed` and the oracle's answers to it, computed once for the four library modes (which run one after the other)."""
    c = vc.make_case(seed)
    oix = _oracle_index(orc, c)
    return (c, orc.pick_batch(c["chain"], c["pods"], oix, c["reqs"], c["B"], c["mask"])[:2],
            orc.pick_topk(c["chain"], c["pods"], oix, c["reqs"], c["k"], c["mask"]))


@pytest.mark.parametrize("library_mode", list(MODES), indirect=True)
@pytest.mark.parametrize("seed", SEEDS)
def test_values_pick_and_fallbacks(pkg, orc, library_mode, seed):
    """pick and pick_topk (k = 1 + case number % 5) of every case against the oracle.  The kernel a chain was built for is the one that
    runs (chain_is_fused), and under EPPK_QUAD_MIN=4 a fused chain with a PREFIX scorer and an index takes pick_quad_kernel."""
    c, want, want_k = _want(orc, seed)
    what = f"mode {library_mode} {vc.info(c)}"
    with _picker(pkg, c) as pk:
        assert pk.chain_is_fused() == c["kind"], what
        launches = pk.quad_stats()[0]
        got = pk.pick(c["reqs"], c["mask"])
        if library_mode == "quadmin4" and vc.quad_route_exists(c):
            assert pk.quad_stats()[0] > launches, what + ": the quad route was not taken"
        got_k = pk.pick_topk(c["reqs"], c["k"], c["mask"])
        assert pk.launch_status() == 0, what
    _same(got, want, what)
    _same(got_k, want_k, what + f" topk {c['k']}")


# ---- the other entry points, once per value mode --------------------------------------------------------------------------------------

ENTRY_PLANS = ("fused8", "tail8", "three_trailing", "between", "negative", "fused7")


def _mode_case(i, **kw):
    q, kv = vc.VALUE_MODES[i]
    return vc.make_case(32000 + i, qmode=q, kvmode=kv, **kw)


@pytest.mark.parametrize("i", range(len(vc.VALUE_MODES)), ids=[q + kv for q, kv in vc.VALUE_MODES])
def test_values_device_candidates_and_learn_entry_points(pkg, orc, i):
    """pick_device (masked, with scores), the candidates form (k = 1 and 3) and pick_learn_device followed by a second pick that reads
    what was learnt."""
    import torch
    c = _mode_case(i, plan=ENTRY_PLANS[i], P=(65, 1500)[i % 2], B=5, R=70, masked=True)
    c["slots"] = 2048                                      # room for what the batch teaches: up to R * B new keys (a table holds slots / 2)
    what = vc.info(c)
    R, B = c["R"], c["B"]
    oix = _oracle_index(orc, c)
    want = orc.pick_batch(c["chain"], c["pods"], oix, c["reqs"], B, c["mask"])[:2]
    with _picker(pkg, c) as pk:
        d_reqs = torch.from_numpy(c["reqs"].view(np.int64)).cuda()
        d_mask = torch.from_numpy(np.ascontiguousarray(c["mask"]).view(np.int64)).cuda()
        d_pick = torch.full((R,), -7, dtype=torch.int32, device="cuda")
        d_score = torch.full((R,), -7.0, dtype=torch.float64, device="cuda")
        pk.pick_device(d_reqs.data_ptr(), R, d_mask.data_ptr(), d_pick.data_ptr(), d_score.data_ptr())
        torch.cuda.synchronize()
        _same((d_pick.cpu().numpy(), d_score.cpu().numpy()), want, what + " pick_device")
        cp, cs = pk.pick_candidates(c["reqs"], c["mask"], 1)
        _same((cp[:, 0], cs[:, 0]), want, what + " candidates form")
        _same(pk.pick_candidates(c["reqs"], c["mask"], 3), orc.pick_topk(c["chain"], c["pods"], oix, c["reqs"], 3, c["mask"]), what + " candidates form, k 3")
        # learn (unmasked): the picks, then the index they leave behind
        plain = orc.pick_batch(c["chain"], c["pods"], oix, c["reqs"], B)[:2]
        pk.pick_learn_device(d_reqs.data_ptr(), R, None, d_pick.data_ptr(), d_score.data_ptr())
        torch.cuda.synchronize()
        _same((d_pick.cpu().numpy(), d_score.cpu().numpy()), plain, what + " pick_learn_device")
        oix.insert_picks(c["reqs"], B, plain[0])
        assert pk.index_dropped() == 0 and pk.index_size() == oix.size() and pk.index_selfcheck() == 0, what
        _same(pk.pick(c["reqs"], c["mask"]), orc.pick_batch(c["chain"], c["pods"], oix, c["reqs"], B, c["mask"])[:2], what + " after learning")
        assert pk.launch_status() == 0, what


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("i", range(len(vc.VALUE_MODES)), ids=[q + kv for q, kv in vc.VALUE_MODES])
def test_values_random_pickers(pkg, orc, ref, i, masked):
    """pick_random_topk against the oracle's, pick_weighted_random (k = 1, 4) against tests/wrand_ref.py fed with the oracle's totals."""
    c = _mode_case(i, plan=ENTRY_PLANS[(i + 1) % 6], P=(1000, 65)[i % 2], B=(5, 70)[i % 2], R=60, masked=masked)
    what = vc.info(c)
    oix = _oracle_index(orc, c)
    T = _totals(orc, c, oix)
    with _picker(pkg, c) as pk:
        for k, seed in ((3, 7), (2, HIGH)):
            _same(pk.pick_random_topk(c["reqs"], k, seed, c["mask"]),
                  orc.pick_random_topk(c["chain"], c["pods"], oix, c["reqs"], c["B"], k, seed, c["mask"]), what + f" random-top-{k}")
        for k in (1, 4):
            _same(pk.pick_weighted_random(c["reqs"], HIGH, k, c["mask"]), ref.weighted_random(T, k, HIGH, np.arange(c["R"])), what + f" weighted-random k {k}")
        assert pk.launch_status() == 0, what


@pytest.mark.timeout(120)
@pytest.mark.parametrize("i", range(len(vc.VALUE_MODES)), ids=[q + kv for q, kv in vc.VALUE_MODES])
def test_values_through_a_resident_unit(pkg, orc, monkeypatch, i):
    """Small unmasked batches answered by the resident workgroup (EPPK_RESIDENT=1), across a publish of other extreme values."""
    monkeypatch.setenv("EPPK_RESIDENT", "1")
    c = _mode_case(i, plan=("fused7", "fused8")[i % 2], P=(1000, 2500, 65)[i % 3], B=5, R=24, masked=False, holes=False)
    what = vc.info(c)
    oix = _oracle_index(orc, c)
    with _picker(pkg, c, max_batch=256) as pk:
        on, b0, _ = pk.resident_stats()
        assert on, what
        for n in (24, 7):
            _same(pk.pick(c["reqs"][:n]), orc.pick_batch(c["chain"], c["pods"], oix, c["reqs"][:n], c["B"])[:2], what + f" resident n {n}")
        assert pk.resident_stats()[1] > b0, what + ": no batch went through the resident workgroup"
        q, kv = vc.VALUE_MODES[(i + 1) % len(vc.VALUE_MODES)]
        pods2 = vc.make_pods(np.random.default_rng(33000 + i), c["P"], q, kv)
        pk.publish(pods2)
        _same(pk.pick(c["reqs"][:9]), orc.pick_batch(c["chain"], pods2, oix, c["reqs"][:9], c["B"])[:2], what + " resident, after a publish")
        assert pk.launch_status() == 0, what


@pytest.mark.parametrize("i", range(len(vc.VALUE_MODES)), ids=[q + kv for q, kv in vc.VALUE_MODES])
def test_values_through_a_one_device_group(pkg, orc, i):
    c = _mode_case(i, plan=ENTRY_PLANS[(i + 2) % 6], P=(1500, 65)[i % 2], B=5, R=90, masked=bool(i % 2))
    what = vc.info(c)
    oix = _oracle_index(orc, c)
    with pkg.DeviceGroup(c["chain"], [0], max_pods=c["P"], max_blocks=c["B"], max_batch=c["R"], index_slots=c["slots"]) as g:
        g.publish(c["pods"])
        if c["ih"].size:
            g.index_insert(c["ih"], c["ip"])
        _same(g.pick(c["reqs"], c["mask"]), orc.pick_batch(c["chain"], c["pods"], oix, c["reqs"], c["B"], c["mask"])[:2], what + " group pick")
        _same(g.pick_topk(c["reqs"], 3, c["mask"]), orc.pick_topk(c["chain"], c["pods"], oix, c["reqs"], 3, c["mask"]), what + " group topk")
        assert g.member_launch_status(0) == 0, what


# ---- republish ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("library_mode", ["default", "quadmin4"], indirect=True)
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("P,new", [(65, ("a", "b")), (1500, ("a", "b")), (1000, ("b", "a")), (2500, ("e", "c"))])
def test_values_republished_over_round_ones(pkg, orc, library_mode, P, new, masked):
    """A snapshot of the old round values (queue 0..63, kv_util in 1/1024), a pick, then a snapshot of extreme values over it with the same
    pod count, and back: both snapshot buffers, the terms and the top tables are rebuilt from the values of the moment."""
    old = vc.make_case(34000 + P, qmode="f", kvmode="d", plan="tail8" if P == 1000 else "fused8", P=P, B=5, R=80, masked=masked, holes=False)
    pods2 = vc.make_pods(np.random.default_rng(34500 + P), P, *new)
    what = f"mode {library_mode} {vc.info(old)} -> queue mode {new[0]} kv_util mode {new[1]}"
    oix = _oracle_index(orc, old)
    with _picker(pkg, old) as pk:
        for step, pods in enumerate((old["pods"], pods2, old["pods"], pods2)):
            if step:
                pk.publish(pods)
            _same(pk.pick(old["reqs"], old["mask"]), orc.pick_batch(old["chain"], pods, oix, old["reqs"], old["B"], old["mask"])[:2], what + f" publish {step}")
            _same(pk.pick_topk(old["reqs"], 4, old["mask"]), orc.pick_topk(old["chain"], pods, oix, old["reqs"], 4, old["mask"]), what + f" publish {step} topk")
        assert pk.launch_status() == 0, what


# ---- assumed load at the top of u32 ---------------------------------------------------------------------------------------------------

Q, KV, L, PF = vc.Q, vc.KV, vc.L, vc.PF


@pytest.mark.parametrize("chain", [[(Q, -1)], [(Q, -65537), (KV, 3), (L, 1), (PF, 7)], [(PF, 7), (Q, -1000003), (KV, 1)],
                                   [(L, 1), (Q, -65537), (KV, 3), (Q, -1), (PF, 3)]], ids=["q", "fused", "tail", "generic"])
@pytest.mark.parametrize("epochs", [1, 3, "R"])
def test_assumed_load_wraps_gauges_at_the_top_of_u32(pkg, orc, chain, epochs):
    """Several pods at 2^32 - 1 and 2^32 - 2 and a negative QUEUE weight: picks land on them, the bump wraps them to 0 (SEMANTICS.md §2b:
    modulo 2^32), which moves qmin AND qmax between epochs.  A second and third batch run on the bumped gauges."""
    c = vc.make_case(35000, qmode="a", kvmode="a", chain=chain, P=65, B=5, R=64, masked=False, holes=False)
    pods = c["pods"].copy()
    pods["queue"][[3, 17, 40, 63, 64]] = vc.U32
    pods["queue"][[0, 18, 41, 62]] = vc.U32 - 1
    E = c["R"] if epochs == "R" else epochs
    what = f"epochs {E} chain {chain}"
    oix = _oracle_index(orc, c, pods)
    fresh = vc.make_case(35001, qmode="a", kvmode="a", chain=chain, P=65, B=5, R=64, masked=False, holes=False)["reqs"]
    with pkg.BatchedPicker(chain, max_pods=65, max_blocks=5, max_batch=64, index_slots=c["slots"]) as pk:
        pk.publish(pods)
        if c["ih"].size:
            pk.index_insert(c["ih"], c["ip"])
        pk.set_assumed_load(E)
        opods = pods.copy()
        for b, reqs in enumerate((c["reqs"], fresh, c["reqs"][:33])):
            want = orc.pick_batch_assumed(chain, opods, oix, reqs, 5, E)
            _same(pk.pick(reqs), want, what + f" batch {b}")
        assert pk.launch_status() == 0, what
    assert (opods["queue"] < pods["queue"]).sum() >= 3, what + ": too few gauges wrapped -- the case does not test what it is for"


# ---- every instantiation --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("npl", [6, 9])
@pytest.mark.parametrize("lw", [0, 1, 2], ids=LW_NAME)
def test_every_instantiation_on_extreme_values(pkg, orc, ref, lw, npl, masked):
    """The (lane word, counter planes, masked) table of test_gpu_wrand_fuzz.test_every_instantiation_at_its_edges: one case of special
    queue and kv_util values at the top of each pod range, through the pick, the ordered fallbacks and the weighted-random picker."""
    n = 4 * lw + 2 * (npl == 9) + masked
    c = vc.make_case(36000 + n, qmode="be"[n % 2], kvmode="b", plan=("fused8", "tail8", "three_trailing")[n % 3], P=LW_TOP[lw],
                     B=63 if npl == 6 else 64, R=48, masked=masked)
    what = f"<{LW_NAME[lw]}, {npl}, {masked}> {vc.info(c)}"
    oix = _oracle_index(orc, c)
    with _picker(pkg, c) as pk:
        assert pk.chain_is_fused() == c["kind"], what
        _same(pk.pick(c["reqs"], c["mask"]), orc.pick_batch(c["chain"], c["pods"], oix, c["reqs"], c["B"], c["mask"])[:2], what)
        _same(pk.pick_topk(c["reqs"], 5, c["mask"]), orc.pick_topk(c["chain"], c["pods"], oix, c["reqs"], 5, c["mask"]), what + " topk 5")
        _same(pk.pick_weighted_random(c["reqs"], HIGH, 4, c["mask"]), ref.weighted_random(_totals(orc, c, oix), 4, HIGH, np.arange(c["R"])), what + " weighted-random")
        assert pk.launch_status() == 0, what


# ---- device prompt hashing ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("block_chars", [8, 16, 24, 32, 40, 56, 64, 72, 128])
def test_device_prompt_hashing_at_every_block_size(pkg, block_chars):
    """hash_prompts_kernel against the host chain (picker.hash_prompt).  A link hashes block_chars + 8 bytes: 2 and 3 words (the short
    path below four), 4 (one stripe, no tail), 5, 6, 7 (a stripe and 1..3 tail words), 8 and more (several stripes).  Prompts of
    k * block_chars - 1, k * block_chars and k * block_chars + 1 bytes for k = 0..8 and of random lengths, with max_blocks = 6: the
    longer ones have more blocks than a row holds.  The row stride, 8 * block_chars + 8 bytes, is a multiple of 8 as the entry point
    demands and (but for block_chars = 8, where that cannot be) not one of block_chars."""
    import torch
    rng = np.random.default_rng(1100 + block_chars)
    B, stride = 6, 8 * block_chars + 8
    edges = sorted({n for k in range(9) for n in (k * block_chars - 1, k * block_chars, k * block_chars + 1) if 0 <= n <= stride})
    lens = np.array(edges + list(rng.integers(0, stride + 1, 40)) + [stride], dtype=np.uint32)
    R = lens.size
    prompts = rng.integers(0, 256, (R, stride), dtype=np.uint8)
    adapters = rng.integers(-1, 128, R).astype(np.int32)
    adapters[:5] = vc.SEAM_ADAPTERS
    lib = pkg.load_library()
    names = [(b"adapter-%d" % a) if a >= 0 else b"base" for a in adapters]
    seeds = np.array([lib.eppk_xxh64(m, len(m), 0) for m in names], dtype=np.uint64)
    want = np.zeros((R, 1 + B), dtype=np.uint64)
    for r in range(R):
        h = pkg.picker.hash_prompt(names[r], prompts[r, :lens[r]].tobytes(), block_chars, B)
        assert h.size == min(int(lens[r]) // block_chars, B)
        want[r, 1:1 + h.size] = h
        want[r, 0] = np.uint64(np.uint32(adapters[r])) | (np.uint64(h.size) << np.uint64(32))
    assert (lens > B * block_chars).sum() >= 5
    with pkg.BatchedPicker([(2, 1)], max_pods=64, max_blocks=B, max_batch=R) as pk:
        d_p = torch.from_numpy(prompts).cuda()
        d_l = torch.from_numpy(lens.view(np.int32)).cuda()
        d_s = torch.from_numpy(seeds.view(np.int64)).cuda()
        d_a = torch.from_numpy(adapters).cuda()
        d_rows = torch.full((R, 1 + B), -1, dtype=torch.int64, device="cuda")
        pk.hash_prompts_device(d_p.data_ptr(), stride, d_l.data_ptr(), d_s.data_ptr(), d_a.data_ptr(), R, block_chars, d_rows.data_ptr())
        torch.cuda.synchronize()
        got = d_rows.cpu().numpy().view(np.uint64)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"block_chars {block_chars}: rows {bad[:5]} of lengths {lens[bad[:5]]} differ"
