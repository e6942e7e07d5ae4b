"""GPU: the metric predicates of the Filter phase (SEMANTICS.md §2c; include/eppk.h eppk_set_filters / eppk_filter_masks) against their
numpy restatement (tests/filter_ref.py) on the cases of tests/filter_cases.py: mask rows and verdict bytes bit for bit.

The module is not in the conftest's MODE_MODULES: it sets the library switches it needs itself, before it creates a context."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q = 1
CHAIN = [(Q, 1)]


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fc():
    return _load("filter_cases")


def _picker(pkg, c, max_batch=None):
    return pkg.BatchedPicker(CHAIN, max_pods=c["P"], max_blocks=c["B"], max_batch=max_batch or max(c["R"], 1))


def _same(got, want, what):
    gm, gv = got
    wm, wv = want
    bad = np.nonzero(np.any(gm != wm, axis=1) | (gv != wv))[0]
    assert bad.size == 0, (f"{what}: {bad.size} rows differ, first {bad[:4]}: gpu {[hex(int(x)) for x in gm[bad[0]]][:4]} verdict {gv[bad[0]]:#x}, "
                           f"restatement {[hex(int(x)) for x in wm[bad[0]]][:4]} verdict {wv[bad[0]]:#x}")


def _check_variants(pk, fc, c, what, pods=None, programs=None):
    """With and without mask_in, with and without cls."""
    pods = c["pods"] if pods is None else pods
    programs = c["programs"] if programs is None else programs
    for use_mask in (True, False):
        for use_cls in (True, False):
            cls = c["cls"] if use_cls else None
            mask = c["mask"] if use_mask else None
            got = pk.filter_masks(c["reqs"], cls=cls, mask=mask)
            want = fc.ref.filter_mask_words(pods, programs, c["adapter"], cls, mask)
            _same(got, want, f"{what} mask_in {use_mask} cls {use_cls}: {fc.info(c)}")


# J = ceil(P / 64) = 1, 1, 1, 2, 3, 64: a word seam, tail bits, idle lanes; R below, at and above a workgroup's four wavefronts
@pytest.mark.parametrize("R", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 130, 4096])
def test_masks_and_verdicts_match_the_restatement(pkg, fc, P, R):
    c = fc.make_case(fc.SEED0 + 100 + P % 97 + R, P=P, R=R)
    with _picker(pkg, c) as pk:
        pk.publish(c["pods"])
        pk.set_filters(c["programs"])
        _check_variants(pk, fc, c, "shape")


def test_a_wavefront_makes_dozens_of_loop_trips(pkg, fc, monkeypatch):
    monkeypatch.setenv("EPPK_MAX_CU", "1")           # the grid is capped from the context's CU count: 8 workgroups, 32 wavefronts, 65 trips
    c = fc.make_case(fc.SEED0 + 200, P=130, R=2049)
    with _picker(pkg, c) as pk:
        pk.publish(c["pods"])
        pk.set_filters(c["programs"])
        _check_variants(pk, fc, c, "narrow grid")


@pytest.mark.parametrize("n", range(24))
def test_generated_cases(pkg, fc, n):
    """The seeds the CPU test holds to their coverage: every (kind, policy) pair in every stage position, holes in a third."""
    c = fc.make_case(fc.SEED0 + n)
    with _picker(pkg, c) as pk:
        pk.publish(c["pods"])
        pk.set_filters(c["programs"])
        _check_variants(pk, fc, c, "generated")


@pytest.mark.parametrize("P", [65, 1000])
def test_snapshots_with_holes(pkg, fc, P):
    c = fc.make_case(fc.SEED0 + 300 + P, P=P, R=64, holes=True)
    assert (c["pods"]["flags"] & 1).any()
    with _picker(pkg, c) as pk:
        pk.publish(c["pods"])
        pk.set_filters(c["programs"])
        _check_variants(pk, fc, c, "holes")
        got = pk.filter_masks(c["reqs"], cls=c["cls"], mask=c["mask"])[0]
        assert not (fc.ref.unpack(got, P) & ((c["pods"]["flags"] & 1) != 0)).any()


def test_no_programs_returns_c0_with_verdict_zero(pkg, fc):
    c = fc.make_case(fc.SEED0 + 301, P=130, R=40, holes=True)
    with _picker(pkg, c) as pk:
        pk.publish(c["pods"])
        _check_variants(pk, fc, c, "no programs", programs=[])
        pk.set_filters(c["programs"])
        pk.set_filters([])                                                    # ... and after programs were taken away again
        _check_variants(pk, fc, c, "programs removed", programs=[])


def test_device_form_in_place_with_bad_classes(pkg, fc):
    """eppk_filter_masks_device with mask_out aliasing mask_in, verdicts and classes on the device; a class without a program gets no
    candidates and EPPK_VERDICT_BAD_CLASS (the host-buffer forms refuse such a batch: tests/test_gpu_filter_pick.py)."""
    import torch
    c = fc.make_case(fc.SEED0 + 302, P=130, R=300)
    cls = c["cls"].copy()
    cls[7::11] = 4
    cls[8::13] = 255
    dev = torch.device("cuda", 0)
    with _picker(pkg, c) as pk:
        pk.publish(c["pods"])
        pk.set_filters(c["programs"])
        d_reqs = torch.from_numpy(c["reqs"].view(np.int64)).to(dev)
        d_mask = torch.from_numpy(c["mask"].view(np.int64).copy()).to(dev)
        d_cls = torch.from_numpy(cls).to(dev)
        d_verdict = torch.full((c["R"],), 0x55, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        pk.filter_masks_device(d_reqs.data_ptr(), c["R"], d_cls.data_ptr(), d_mask.data_ptr(), d_mask.data_ptr(), d_verdict.data_ptr())
        torch.cuda.synchronize(dev)
        got = (d_mask.cpu().numpy().view(np.uint64), d_verdict.cpu().numpy())
        want = fc.ref.filter_mask_words(c["pods"], c["programs"], c["adapter"], cls, c["mask"])
        assert (want[1] & fc.ref.BAD_CLASS).sum() >= 20
        _same(got, want, "in place")
        # without a verdict array, into a second buffer
        d_out = torch.zeros_like(d_mask)
        d_in = torch.from_numpy(c["mask"].view(np.int64).copy()).to(dev)
        torch.cuda.synchronize(dev)
        pk.filter_masks_device(d_reqs.data_ptr(), c["R"], d_cls.data_ptr(), d_in.data_ptr(), d_out.data_ptr(), None)
        torch.cuda.synchronize(dev)
        assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want[0])
        assert np.array_equal(d_in.cpu().numpy().view(np.uint64), c["mask"])
        assert pk.launch_status() == 0


def test_assumed_load_bumps_reach_the_planes(pkg, orc, fc):
    """The stale-plane test.  assumed_bump_kernel edits the raw rows in place: a QUEUE_LE plane built before a batch must not serve the
    filter call behind it.  E = 1 and a chain of QUEUE alone: all R requests of the batch pick the pod t with the shortest queue, whose
    gauge grows to q' = queue[t] + R.  Class 0 asks for queue <= q' - 1, class 1 for queue <= q': before the batch t passes both, after
    it t passes class 1 alone -- with no publish and no eppk_set_filters in between."""
    c = fc.make_case(fc.SEED0 + 303, P=130, R=33, qmode="f", holes=False)
    pods = c["pods"].copy()
    pods["queue"] = np.arange(130, dtype=np.uint32)[::-1] * 100 + 7          # distinct; the shortest queue is pod 129's 7
    t, R = 129, c["R"]
    q_new = int(pods["queue"][t]) + R
    programs = [[(fc.ref.QUEUE_LE, fc.ref.REQUIRE, q_new - 1)], [(fc.ref.QUEUE_LE, fc.ref.REQUIRE, q_new)]]
    cls = (np.arange(R) % 2).astype(np.uint8)
    with _picker(pkg, c) as pk:
        pk.publish(pods)
        pk.set_filters(programs)
        pk.set_assumed_load(1)
        before = pk.filter_masks(c["reqs"], cls=cls)
        _same(before, fc.ref.filter_mask_words(pods, programs, c["adapter"], cls), "before the batch")
        assert np.all((before[0][:, t // 64] >> np.uint64(t % 64)) & np.uint64(1) == 1)
        picks, scores = pk.pick(c["reqs"])
        opods = pods.copy()
        opicks, oscores = orc.pick_batch_assumed(CHAIN, opods, None, c["reqs"], c["B"], 1)
        assert np.array_equal(picks, opicks) and np.array_equal(scores.view(np.uint64), oscores.view(np.uint64)) and np.all(picks == t)
        for p in picks:                                                       # the restatement's queues: queue[pick] += 1
            pods["queue"][p] += 1
        assert int(pods["queue"][t]) == q_new and np.array_equal(pods["queue"], opods["queue"])
        after = pk.filter_masks(c["reqs"], cls=cls)
        _same(after, fc.ref.filter_mask_words(pods, programs, c["adapter"], cls), "after the batch")
        has_t = ((after[0][:, t // 64] >> np.uint64(t % 64)) & np.uint64(1)).astype(np.uint8)
        assert np.array_equal(has_t, cls), "pod t passes `queue <= q'` and fails `queue <= q' - 1`"
        # a bump inside eppk_pick_filtered (the filter of the NEXT call sees it), thresholds at the new gauge again
        p2, s2, v2 = pk.pick_filtered(c["reqs"], 1, cls=cls)
        want_mask, want_v = fc.ref.filter_mask_words(pods, programs, c["adapter"], cls)
        op2, os2 = orc.pick_batch_assumed(CHAIN, pods, None, c["reqs"], c["B"], 1, mask=want_mask)    # (mutates pods: the bumps of this batch)
        assert np.array_equal(p2[:, 0], op2) and np.array_equal(s2[:, 0].view(np.uint64), os2.view(np.uint64)) and np.array_equal(v2, want_v)
        assert np.all(op2[cls == 0] == -1) and np.all(op2[cls == 1] == t) and np.all(v2[cls == 0] == (1 | fc.ref.SHED))
        _same(pk.filter_masks(c["reqs"], cls=cls), fc.ref.filter_mask_words(pods, programs, c["adapter"], cls), "after the filtered batch")


def test_a_publish_and_new_programs_each_take_effect(pkg, fc):
    c = fc.make_case(fc.SEED0 + 304, P=130, R=48)
    d = fc.make_case(fc.SEED0 + 305, P=130, R=48, holes=True)
    with _picker(pkg, c) as pk:
        pk.publish(c["pods"])
        pk.set_filters(c["programs"])
        _check_variants(pk, fc, c, "first snapshot")
        pk.publish(d["pods"])                                                 # new rows, the programs stay
        _check_variants(pk, fc, c, "second snapshot", pods=d["pods"])
        pk.set_filters(d["programs"])                                         # new programs, the rows stay
        _check_variants(pk, fc, c, "second programs", pods=d["pods"], programs=d["programs"])
        pk.publish(d["pods"][:65])                                            # fewer pods: J shrinks from 3 to 2
        c65 = dict(c, P=65, mask=np.ascontiguousarray(c["mask"][:, :2]))
        _check_variants(pk, fc, c65, "smaller snapshot", pods=d["pods"][:65], programs=d["programs"])
