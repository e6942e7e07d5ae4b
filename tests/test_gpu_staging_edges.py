"""The pick kernels' table staging at every edge of its copy, bit for bit against the oracle.

pick_quad_body and pick_fast_body copy the snapshot's tables into LDS in front of their loops (csrc/eppk_kernels.hip.h: stage_issue /
stage_write / stage_rest): base[] (J * 64 words), the prefix-term table (pwn = (max_blocks + 1)^2 words: odd for an even max_blocks), for
an interpreted tail the two post[] planes, for masked picks the snapshot's three sets; and they zero the "listed" bits, the histogram and
the scratch words behind the tables.  A first trip covers 4 (base) or 2 (the others) 16-byte pairs per thread, further trips take the rest,
the odd last word is a load of its own.  A word that is not copied, or copied over its neighbour, must change a pick or a score here:

  * pods 1, 64, 65 and 4096 (J = 1, 1, 2, 64), the LAST pod with the best base score: rows without a prefix pick it;
  * max_blocks 1, 2, 31, 32 and 63 (pwn = 4, 9, 1024, 1089, 4096: even and odd, below, at and above one trip of 512 threads), with rows of
    n_blocks = max_blocks whose blocks are all cached on the winning pod: the table's last word is their prefix term.  Beyond 32 blocks
    the quad kernel defers such rows: the work-list pass of the same workgroup stages the fast kernel's layout over the quad layout;
  * rows with a reserved hash next to ordinary rows (deferred as well, in every shape);
  * workgroups of 64 and 512 threads (quad kernel), 64 and 1024 (fast kernel);
  * a masked batch, an interpreted tail (a pod-only scorer behind PREFIX), and launches back to back on one context across publishes
    that change J.
"""
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


tq = _load("test_gpu_quad")
assert_same, pairs_by_pod = tq.assert_same, tq.pairs_by_pod

Q, KV, L, PF = 1, 2, 3, 4
FUSED = [(Q, 2), (KV, 2), (L, 1), (PF, 3)]
TAILED = [(Q, 2), (L, 1), (PF, 3), (KV, 2)]                 # KV behind PREFIX: the fast kernel's interpreted tail (post[] planes)
PODS = (1, 64, 65, 4096)
BLOCKS = (1, 2, 31, 32, 63)
N_GROUPS, R = 8, 256
KNOBS = ("EPPK_QUAD", "EPPK_QUAD_MIN", "EPPK_QUAD_PAUSE", "EPPK_QUAD_TAIL", "EPPK_QUAD_THREADS", "EPPK_FAST_THREADS", "EPPK_LISTS", "EPPK_MAX_CU",
         "EPPK_MAX_WG_PER_CU", "EPPK_RESIDENT")
# route -> (switches, the thread knob, workgroup sizes)
ROUTES = {"quad": ({"EPPK_QUAD_MIN": "4", "EPPK_QUAD_PAUSE": "0"}, "EPPK_QUAD_THREADS", (64, 512)),
          "fast": ({"EPPK_QUAD": "0"}, "EPPK_FAST_THREADS", (64, 1024))}
RESERVED = {9: 0, 42: 0xFFFFFFFFFFFFFFFF}                     # row -> its reserved hash (each among ordinary rows of its wavefront)


def set_env(monkeypatch, route, threads):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    env, knob, _ = ROUTES[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv(knob, str(threads))


def make_pods(pkg, P, seed, limit=None):
    """P pods, the last one alone at the shortest queue and the emptiest cache."""
    pods = pkg.workload.make_pods(seed, P, 128)
    pods["queue"] = np.maximum(pods["queue"], 1)
    pods["kv_util"] = np.maximum(pods["kv_util"], 1.0 / 1024.0)
    pods["queue"][-1] = 0
    pods["kv_util"][-1] = 0.0
    return pods


def group_pods(g, P):
    ps = {(g * 37 + o) % P for o in (5, 23, 42, 71)}
    if g == 0:
        ps.add(P - 1)
    return tuple(sorted(ps))


def make_rows(pkg, P, B, seed):
    """({hash: pods}, rows, kinds): eight prefix groups of B blocks, every block of a group on the group's pods; row r of group r % 8
    and kind (r // 8) % 8."""
    sm = pkg.workload.splitmix64
    chains = sm(seed * 7 + 1, N_GROUPS * B).reshape(N_GROUPS, B)
    private = sm(seed * 7 + 2, R * B).reshape(R, B)
    asrc = sm(seed * 7 + 3, R)
    sets = {int(h): group_pods(g, P) for g in range(N_GROUPS) for h in chains[g]}
    hashes = np.zeros((R, B), dtype=np.uint64)
    nb = np.zeros(R, dtype=np.uint32)
    adapter = np.where((asrc & np.uint64(3)) == 0, -1, (asrc >> np.uint64(8)) % np.uint64(128)).astype(np.int32)
    kinds = (np.arange(R) // N_GROUPS) % 8
    for r in range(R):
        g, kind = r % N_GROUPS, int(kinds[r])
        hashes[r] = chains[g]
        nb[r] = B
        if kind == 2:                                        # leaves its group half-way
            hashes[r, B // 2:] = private[r, B // 2:]
        elif kind == 3:
            nb[r] = B - 1
        elif kind == 4:                                      # no prefix, no adapter: the best base score alone
            nb[r], adapter[r] = 0, -1
        elif kind == 5:                                      # nothing cached
            hashes[r] = private[r]
        elif kind == 6:
            nb[r] = min(B, 17)
    for r, h in RESERVED.items():
        kinds[r] = 8
        nb[r] = B
        hashes[r] = chains[r % N_GROUPS]
        hashes[r, min(B - 1, 20 if h else 0)] = np.uint64(h)
    return sets, pkg.picker.make_req_rows(adapter, nb, hashes, B), kinds


_CORPUS = {}


def corpus(pkg, orc, P, B, chain=FUSED, masked=False):
    """The batch of a shape and the oracle's answer, computed once per module run and left unchanged."""
    key = (P, B, tuple(chain), masked)
    if key not in _CORPUS:
        pods = make_pods(pkg, P, 0x57A6 + P)
        sets, reqs, kinds = make_rows(pkg, P, B, 100 * P + B)
        calls = pairs_by_pod(sets)
        oix = orc.OracleIndex()
        for h, p in calls:
            oix.insert(h, p)
        mask = None
        if masked:                                           # about half of the pods, the last one in every second row
            W = (P + 63) // 64
            mask = pkg.workload.splitmix64(900 + P + B, R * W).reshape(R, W).copy()
            if P % 64:
                mask[:, -1] &= np.uint64((1 << (P % 64)) - 1)
            last = np.uint64(1 << ((P - 1) % 64))
            mask[::2, -1] |= last
            mask[1::2, -1] &= ~last
            mask[1::2, 0] |= np.uint64(1)
        opicks, oscores, _ = orc.pick_batch(chain, pods, oix, reqs, B, mask)
        if not masked:
            assert (opicks[kinds == 4] == P - 1).all(), "rows without a prefix go to the last pod: the corpus is not what it says"
        if chain is FUSED and not masked:
            full = (kinds <= 1) | (kinds == 7)
            assert np.isin(opicks[full], np.concatenate([group_pods(g, P) for g in range(N_GROUPS)])).all(), "a fully cached row goes to a pod of its group"
        _CORPUS[key] = dict(pods=pods, reqs=reqs, kinds=kinds, calls=calls, mask=mask, opicks=opicks, oscores=oscores, slots=4096)
    return _CORPUS[key]


def run(pkg, c, chain, P, B, route, threads, what, fused=1):
    """`fused`: what chain_is_fused() says of the chain -- 1 = the fused kernels, 2 = with an interpreted tail."""
    with pkg.BatchedPicker(chain, max_pods=P, max_blocks=B, max_batch=R, index_slots=c["slots"]) as pk:
        assert pk.chain_is_fused() == fused, f"{what}: chain_is_fused() = {pk.chain_is_fused()}"
        pk.publish(c["pods"])
        for h, p in c["calls"]:
            pk.index_insert(h, p)
        picks, scores = pk.pick(c["reqs"], c["mask"])
        g = pk.launch_geometry()
        ql, qd = pk.quad_stats()
        assert pk.launch_status() == 0
    assert_same(picks, scores, c["opicks"], c["oscores"])
    if route == "quad":
        assert ql == 1 and g[:2][1] == threads and g[2:] == (0, 0), f"{what}: not one launch of the quad kernel at {threads} threads: {ql} {g}"
    else:
        assert ql == 0 and g[:2] == (0, 0) and g[3] == threads, f"{what}: not the fast kernel at {threads} threads: {ql} {g}"
    return qd


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("P", PODS)
def test_every_table_edge_on_the_quad_kernel_and_its_tail(pkg, orc, monkeypatch, P, B):
    c = corpus(pkg, orc, P, B)
    n_full = int(((c["kinds"] <= 1) | (c["kinds"] == 7)).sum())
    for threads in ROUTES["quad"][2]:
        set_env(monkeypatch, "quad", threads)
        qd = run(pkg, c, FUSED, P, B, "quad", threads, f"P={P} B={B}")
        assert qd >= len(RESERVED), f"P={P} B={B} threads={threads}: rows with a reserved hash are deferred to the tail, {qd} were"
        if B > 32:
            assert qd >= len(RESERVED) + n_full, f"P={P} B={B} threads={threads}: rows cached beyond 32 blocks are deferred, {qd} of {n_full} were"
        assert qd < R, "ordinary rows are the quad kernel's own"


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("P", PODS)
def test_every_table_edge_on_the_fast_kernel(pkg, orc, monkeypatch, P, B):
    c = corpus(pkg, orc, P, B)
    for threads in ROUTES["fast"][2]:
        set_env(monkeypatch, "fast", threads)
        run(pkg, c, FUSED, P, B, "fast", threads, f"P={P} B={B}")


@pytest.mark.parametrize("P,B", [(4096, 32), (65, 31)])
def test_a_masked_batch_stages_the_snapshot_sets(pkg, orc, monkeypatch, P, B):
    c = corpus(pkg, orc, P, B, masked=True)
    for route, (_, _, sizes) in ROUTES.items():
        for threads in sizes:
            set_env(monkeypatch, route, threads)
            run(pkg, c, FUSED, P, B, route, threads, f"masked P={P} B={B}")


@pytest.mark.parametrize("P,B", [(4096, 32), (65, 31), (64, 2)])
def test_an_interpreted_tail_stages_both_post_planes(pkg, orc, monkeypatch, P, B):
    """pwn odd (B = 32, 2): the planes sit at an 8-byte aligned address behind the prefix-term table."""
    c = corpus(pkg, orc, P, B, chain=TAILED)
    for threads in ROUTES["fast"][2]:
        set_env(monkeypatch, "fast", threads)
        run(pkg, c, TAILED, P, B, "fast", threads, f"tailed P={P} B={B}", fused=2)


@pytest.mark.parametrize("route", list(ROUTES))
def test_launches_back_to_back_across_publishes_that_change_j(pkg, orc, monkeypatch, route):
    """One context: 4096 pods (J = 64), 64 (J = 1), 65 (J = 2), 4096 again -- every table moves in LDS with J, and what the launch before
    left there must not be read."""
    B, threads = 32, ROUTES[route][2][1]
    set_env(monkeypatch, route, threads)
    sets, reqs, _ = make_rows(pkg, 64, B, 7)                 # (every listed pod exists under each snapshot)
    calls = pairs_by_pod(sets)
    oix = orc.OracleIndex()
    for h, p in calls:
        oix.insert(h, p)
    with pkg.BatchedPicker(FUSED, max_pods=4096, max_blocks=B, max_batch=R, index_slots=4096) as pk:
        for h, p in calls:
            pk.index_insert(h, p)
        for n, P in enumerate((4096, 64, 65, 4096)):
            pods = make_pods(pkg, P, 31 + n)
            opicks, oscores, _ = orc.pick_batch(FUSED, pods, oix, reqs, B)
            pk.publish(pods, epoch=n + 1)
            picks, scores = pk.pick(reqs)
            assert_same(picks, scores, opicks, oscores)
        assert pk.quad_stats()[0] == (4 if route == "quad" else 0)
        assert pk.launch_status() == 0
