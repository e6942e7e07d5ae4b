"""GPU: the pickers behind the Filter phase's metric predicates (SEMANTICS.md §2c; include/eppk.h eppk_pick_filtered): picks and binary64
scores against the ORACLE fed with the candidate rows of the numpy restatement (tests/filter_ref.py), bit for bit; argument checks.

The module is not in the conftest's MODE_MODULES: it sets the library switches itself (monkeypatch) before it creates a context."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = {"default": {}, "quadmin4": {"EPPK_QUAD_MIN": "4"}, "quad0": {"EPPK_QUAD": "0"}}
# (P, R, holes): up to the full 2048 x 4096; a ragged last mask word with holes; below a wavefront's four requests
SHAPES = [(4096, 2048, False), (1000, 300, True), (130, 3, False)]
KS = (1, 3, 8)


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fc():
    return _load("filter_cases")


def _case(pkg, orc, fc, P, R, holes):
    """A generator case (snapshot values, programs, classes, masks, adapters) under the full chain, with config 3's hashes and index."""
    wl = pkg.workload.make_workload(3, R=R, P=P)
    c = fc.make_case(fc.SEED0 + 400 + P % 89 + R % 7, P=P, R=R, holes=holes)
    reqs = wl.reqs.copy()
    reqs[:, 0] = (reqs[:, 0] & ~np.uint64(0xFFFFFFFF)) | c["adapter"].view(np.uint32).astype(np.uint64)
    oix = orc.OracleIndex()
    oix.insert(wl.index_hashes, wl.index_pods, snapshot=c["pods"])
    masks, verdict = fc.ref.filter_mask_words(c["pods"], c["programs"], c["adapter"], c["cls"], c["mask"])
    return dict(c, wl=wl, reqs=reqs, B=wl.B, oix=oix, want_mask=masks, want_verdict=verdict, topk={})


@pytest.fixture(scope="module")
def cases(pkg, orc, fc):
    """Built once, shared by the modes: the restatement's masks, and (filled on first use) the oracle's lists on them."""
    return {(P, R): _case(pkg, orc, fc, P, R, holes) for P, R, holes in SHAPES}


def _oracle_topk(orc, c, k):
    if k not in c["topk"]:
        c["topk"][k] = orc.pick_topk_batch(c["wl"].chain, c["pods"], c["oix"], c["reqs"], c["B"], k, mask=c["want_mask"], threads=8)
    return c["topk"][k]


def _picker(pkg, c):
    wl = c["wl"]
    pk = pkg.BatchedPicker(wl.chain, max_pods=c["P"], max_blocks=wl.B, max_batch=c["R"], index_slots=wl.index_slots)
    pk.publish(c["pods"])
    pk.index_insert(wl.index_hashes, wl.index_pods)
    return pk


def _same_lists(got, want, what):
    gp, gs = got
    wp, ws = want
    bad = np.nonzero(np.any(gp != wp, axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[:4]}: gpu {gp[bad[:2]]} oracle {wp[bad[:2]]}"
    assert np.array_equal(gs.view(np.uint64), ws.view(np.uint64)), f"{what}: scores differ (bitwise)"


@pytest.mark.parametrize("P,R", [(P, R) for P, R, _ in SHAPES])
@pytest.mark.parametrize("mode", list(MODES))
def test_pick_filtered_equals_the_oracle_on_the_restatement_masks(pkg, orc, fc, cases, monkeypatch, mode, P, R):
    for name, value in MODES[mode].items():
        monkeypatch.setenv(name, value)
    c = cases[(P, R)]
    with _picker(pkg, c) as pk:
        pk.set_filters(c["programs"])
        for k in KS:
            picks, scores, verdict = pk.pick_filtered(c["reqs"], k, cls=c["cls"], mask=c["mask"])
            assert np.array_equal(verdict, c["want_verdict"]), f"{mode} k {k}: verdicts"
            _same_lists((picks, scores), _oracle_topk(orc, c, k), f"{mode} k {k} {fc.info(c)}")
            shed = (verdict & fc.ref.SHED) != 0
            assert (shed.any() or R < 4) and np.all(picks[shed] == -1) and np.all(scores[shed] == 0.0)


def test_pick_filtered_device_keeps_the_masks_on_the_device(pkg, orc, fc, cases):
    import torch
    c = cases[(1000, 300)]
    dev = torch.device("cuda", 0)
    k = 3
    with _picker(pkg, c) as pk:
        pk.set_filters(c["programs"])
        d_reqs = torch.from_numpy(c["reqs"].view(np.int64)).to(dev)
        d_mask = torch.from_numpy(c["mask"].view(np.int64).copy()).to(dev)
        d_cls = torch.from_numpy(c["cls"]).to(dev)
        d_pick = torch.empty((c["R"], k), dtype=torch.int32, device=dev)
        d_score = torch.empty((c["R"], k), dtype=torch.float64, device=dev)
        d_verdict = torch.empty(c["R"], dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        pk.pick_filtered_device(d_reqs.data_ptr(), c["R"], d_cls.data_ptr(), d_mask.data_ptr(), k, d_pick.data_ptr(), d_score.data_ptr(), d_verdict.data_ptr())
        torch.cuda.synchronize(dev)
        _same_lists((d_pick.cpu().numpy(), d_score.cpu().numpy()), _oracle_topk(orc, c, k), "device form")
        assert np.array_equal(d_verdict.cpu().numpy(), c["want_verdict"])
        assert np.array_equal(d_mask.cpu().numpy().view(np.uint64), c["mask"]), "the caller's mask rows are not written"


@pytest.mark.parametrize("P,R", [(1000, 300), (130, 3)])
def test_the_other_pickers_compose_through_filter_masks(pkg, fc, cases, P, R):
    c = cases[(P, R)]
    with _picker(pkg, c) as pk:
        pk.set_filters(c["programs"])
        masks, verdict = pk.filter_masks(c["reqs"], cls=c["cls"], mask=c["mask"])
        assert np.array_equal(masks, c["want_mask"]) and np.array_equal(verdict, c["want_verdict"])
        for k, seed in ((1, 0), (3, 0xDEADBEEFCAFEF00D), (8, 7)):
            got = pk.pick_weighted_random(c["reqs"], seed, k, masks)
            want = pk.pick_weighted_random(c["reqs"], seed, k, c["want_mask"])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
            got = pk.pick_random_topk(c["reqs"], k, seed, masks)
            want = pk.pick_random_topk(c["reqs"], k, seed, c["want_mask"])
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
            assert np.all(got[0][(verdict & fc.ref.SHED) != 0] == -1)


@pytest.mark.parametrize("masked", [False, True])
def test_without_programs_pick_filtered_is_pick_topk(pkg, cases, masked):
    c = cases[(1000, 300)]
    mask = c["mask"] if masked else None
    with _picker(pkg, c) as pk:
        for k in KS:
            picks, scores, verdict = pk.pick_filtered(c["reqs"], k, cls=c["cls"], mask=mask)
            wp, ws = pk.pick_topk(c["reqs"], k, mask)
            assert np.array_equal(picks, wp) and np.array_equal(scores.view(np.uint64), ws.view(np.uint64)) and not verdict.any()


def _progs(pkg, n):
    return (pkg._lib.FilterProgram * n)()


def test_argument_validation_names_what_it_rejects(pkg, fc, cases):
    c = cases[(130, 3)]
    lib = pkg.load_library()
    ARG = -1
    with _picker(pkg, c) as pk:
        def err():
            return (lib.eppk_last_error(pk._ctx) or b"").decode()

        pk.set_filters(c["programs"])
        good = pk.filter_masks(c["reqs"], cls=c["cls"], mask=c["mask"])
        pr = _progs(pkg, 5)
        assert lib.eppk_set_filters(pk._ctx, pr, 5) == ARG and "5 programs" in err()
        pr = _progs(pkg, 2)
        pr[1].n_stages = 5
        assert lib.eppk_set_filters(pk._ctx, pr, 2) == ARG and "program 1" in err() and "5 stages" in err()
        pr = _progs(pkg, 2)
        pr[1].reserved = 1
        assert lib.eppk_set_filters(pk._ctx, pr, 2) == ARG and "program 1" in err() and "reserved" in err()
        for field, value, word in (("kind", 0, "kind"), ("kind", 7, "kind"), ("on_empty", 2, "on_empty"), ("reserved", 9, "reserved")):
            pr = _progs(pkg, 3)
            for g in range(3):
                pr[g].n_stages = 3
                for s in range(3):
                    pr[g].stage[s].kind = 1
            setattr(pr[2].stage[1], field, value)
            assert lib.eppk_set_filters(pk._ctx, pr, 3) == ARG, (field, value)
            assert "program 2 stage 1" in err() and word in err(), err()
        # a refused call leaves the programs in force as they were
        again = pk.filter_masks(c["reqs"], cls=c["cls"], mask=c["mask"])
        assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
        with pytest.raises(pkg.EppkError) as ei:
            pk.set_filters([[(1, 0, 0)] * 5])
        assert ei.value.code == ARG
        # the host-buffer forms name the lowest row whose class has no program, and deliver nothing
        cls = np.array([0, 4, 9], dtype=np.uint8)
        for call in (lambda: pk.filter_masks(c["reqs"], cls=cls), lambda: pk.pick_filtered(c["reqs"], 1, cls=cls)):
            with pytest.raises(pkg.EppkError) as ei:
                call()
            assert ei.value.code == ARG and "row 1" in str(ei.value) and "class 4" in str(ei.value)
        out = np.full((3, 3), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        v = np.full(3, 0x5A, dtype=np.uint8)
        assert lib.eppk_filter_masks(pk._ctx, c["reqs"].ctypes.data, 3, cls.ctypes.data, None, out.ctypes.data, v.ctypes.data) == ARG
        assert np.all(out == 0x5A5A5A5A5A5A5A5A) and np.all(v == 0x5A)
        for k in (0, 9):
            with pytest.raises(pkg.EppkError) as ei:
                pk.pick_filtered(c["reqs"], k)
            assert ei.value.code == ARG and "k out of range" in str(ei.value)
        bad = c["reqs"].copy()
        bad[2, 0] = np.uint64(128)                                            # adapter 128
        with pytest.raises(pkg.EppkError) as ei:
            pk.filter_masks(bad)
        assert ei.value.code == ARG and "row 2" in str(ei.value)
        assert lib.eppk_filter_masks(pk._ctx, None, 3, None, None, out.ctypes.data, None) == ARG
        assert lib.eppk_set_filters(None, None, 0) == ARG
    with pkg.BatchedPicker(c["wl"].chain, max_pods=130, max_blocks=c["B"], max_batch=4) as pk:
        with pytest.raises(pkg.EppkError) as ei:
            pk.filter_masks(c["reqs"])
        assert ei.value.code == -4                                            # EPPK_ERR_NO_SNAPSHOT
