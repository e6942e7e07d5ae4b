"""eppk_host_staging / eppk_pick_batch_staged: rows (and mask rows) built in the library's pinned buffers give the picks and scores of
eppk_pick_batch on the same rows; eppk_pick_batch itself uploads pageable rows in chunks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R,P,masked", [(1, 64, False), (700, 1000, False), (700, 1000, True), (40000, 4096, False), (33000, 4096, True)])
def test_staged_pick_equals_pick(pkg, orc, R, P, masked):
    wl = pkg.workload.make_workload(5, R=R, P=P, n_groups=32, masked=masked)
    with pkg.BatchedPicker(wl.chain, max_pods=4096, max_blocks=wl.B, max_batch=R + 5, index_slots=wl.index_slots) as pk:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        want_p, want_s = pk.pick(wl.reqs, wl.mask)                   # (40000 x 264 B = 10 MB: five chunks)
        st_reqs, st_mask = pk.staging(with_mask=masked)
        assert st_reqs.shape == (R + 5, 1 + wl.B)
        st_reqs[:R] = wl.reqs
        if masked:
            J = (P + 63) // 64
            st_mask[:R * J].reshape(R, J)[:] = wl.mask
        got_p, got_s = pk.pick_staged(R, use_mask=masked)
        assert np.array_equal(got_p, want_p) and np.array_equal(got_s.view(np.uint64), want_s.view(np.uint64))
        # and both equal the oracle
        oix = orc.OracleIndex()
        oix.insert(wl.index_hashes, wl.index_pods)
        op, os_, _ = orc.pick_batch(wl.chain, wl.pods, oix, wl.reqs, wl.B, wl.mask)
        assert np.array_equal(got_p, op) and np.array_equal(got_s.view(np.uint64), os_.view(np.uint64))
        # a bad row in the staging buffer is refused like anywhere else
        st_reqs[0, 0] = np.uint64(1000) << np.uint64(32)
        with pytest.raises(Exception):
            pk.pick_staged(R, use_mask=masked)


@pytest.mark.parametrize("zc_max", [None, "0", "1000000"])      # zero-copy picks of small batches: the library's default limit / never / every size
@pytest.mark.parametrize("R,learn,masked", [(3000, False, False), (3000, True, False), (1500, True, True), (20000, True, False)])
def test_pipelined_stage_sets_against_the_oracle(pkg, orc, monkeypatch, eppk_mode, R, learn, masked, zc_max):
    """eppk_pick_stage_begin / _end: two staging sets in flight, batch k + 1 uploaded while batch k is scored.  Eight batches, picks and
    scores of every one bit-exact against the oracle running the same sequence -- with EPPK_PICK_LEARN the post-route index update is
    chained on the device behind each pick and batch k + 1 must already see what batch k taught the index (the oracle inserts between
    batches), although its rows were uploaded before that update finished."""
    if zc_max is not None:
        monkeypatch.setenv("EPPK_ZERO_COPY_MAX", zc_max)
    wl = pkg.workload.make_workload(5, R=R, P=4096, n_groups=16, masked=masked)
    batches = [wl.reqs] + [pkg.workload.make_requests(wl, 31 + i) for i in range(3)]
    J = (wl.P + 63) // 64
    with pkg.BatchedPicker(wl.chain, max_pods=4096, max_blocks=wl.B, max_batch=R, index_slots=1 << 23) as pk:     # (4 batches x 16 new blocks x R keys stay below the load limit)
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        oix = orc.OracleIndex()
        oix.insert(wl.index_hashes, wl.index_pods)
        bufs = [pk.stage_buffers(0, with_mask=masked), pk.stage_buffers(1, with_mask=masked)]

        def fill(s, b):
            bufs[s][0][:R] = batches[b % len(batches)]
            if masked:
                bufs[s][1][:R * J].reshape(R, J)[:] = wl.mask

        def check(s, b):
            picks, scores = pk.stage_end(s)
            op, osc, _ = orc.pick_batch(wl.chain, wl.pods, oix, batches[b % len(batches)], wl.B, wl.mask if masked else None)
            assert np.array_equal(picks, op), f"batch {b}: {int((picks != op).sum())} picks differ"
            assert np.array_equal(scores.view(np.uint64), osc.view(np.uint64)), f"batch {b}"
            if learn:
                oix.insert_picks(batches[b % len(batches)], wl.B, op)

        n_batches = 8
        fill(0, 0)
        pk.stage_begin(0, R, use_mask=masked, learn=learn)
        for b in range(1, n_batches):
            s = b & 1
            fill(s, b)
            pk.stage_begin(s, R, use_mask=masked, learn=learn)      # batch b is on its way before batch b - 1 has been collected
            check(s ^ 1, b - 1)
        check((n_batches - 1) & 1, n_batches - 1)
        assert pk.launch_status() == 0 and pk.index_selfcheck() == 0 and pk.index_dropped() == 0
        if learn:
            assert pk.index_size() == oix.size()
        # protocol errors: end without begin, begin twice
        with pytest.raises(pkg.EppkError):
            pk.stage_end(0)
        pk.stage_begin(0, R, use_mask=masked)
        with pytest.raises(pkg.EppkError):
            pk.stage_begin(0, R, use_mask=masked)
        pk.stage_end(0)


@pytest.mark.parametrize("zc_max", ["0", None, "1000000"])
@pytest.mark.parametrize("R,masked", [(1, False), (37, True), (2048, False), (3072, True), (3073, False), (8200, False)])
def test_zero_copy_small_batches(pkg, orc, monkeypatch, eppk_mode, zc_max, R, masked):
    """Host-buffer picks of at most EPPK_ZERO_COPY_MAX requests run zero-copy (the kernel reads the pinned staging rows and writes the
    pinned result buffers: one launch, no upload / download): every entry point that takes the path -- eppk_pick_batch on pageable rows,
    eppk_pick_batch_staged, eppk_pick_stage_begin / _end -- against the oracle, with the path off, at its default and forced for every size."""
    if zc_max is None:
        monkeypatch.delenv("EPPK_ZERO_COPY_MAX", raising=False)           # the library's default (3072)
    else:
        monkeypatch.setenv("EPPK_ZERO_COPY_MAX", zc_max)
    wl = pkg.workload.make_workload(5, R=R, P=4096, n_groups=16, masked=masked)
    J = (wl.P + 63) // 64
    oix = orc.OracleIndex()
    oix.insert(wl.index_hashes, wl.index_pods)
    op, os_, _ = orc.pick_batch(wl.chain, wl.pods, oix, wl.reqs, wl.B, wl.mask)
    with pkg.BatchedPicker(wl.chain, max_pods=4096, max_blocks=wl.B, max_batch=R + 3, index_slots=wl.index_slots) as pk:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        for rep in range(2):                                           # (twice: the buffers are reused)
            p, s = pk.pick(wl.reqs, wl.mask)
            assert np.array_equal(p, op) and np.array_equal(s.view(np.uint64), os_.view(np.uint64)), "eppk_pick_batch"
            st_reqs, st_mask = pk.staging(with_mask=masked)
            st_reqs[:R] = wl.reqs
            if masked:
                st_mask[:R * J].reshape(R, J)[:] = wl.mask
            p, s = pk.pick_staged(R, use_mask=masked)
            assert np.array_equal(p, op) and np.array_equal(s.view(np.uint64), os_.view(np.uint64)), "eppk_pick_batch_staged"
            for which in (0, 1):
                b_reqs, b_mask = pk.stage_buffers(which, with_mask=masked)
                b_reqs[:R] = wl.reqs
                if masked:
                    b_mask[:R * J].reshape(R, J)[:] = wl.mask
                pk.stage_begin(which, R, use_mask=masked)
            for which in (0, 1):
                p, s = pk.stage_end(which)
                assert np.array_equal(p, op) and np.array_equal(s.view(np.uint64), os_.view(np.uint64)), f"stage set {which}"
        # ordered fallbacks and the random-top-k picker go through the same staging (eppk_pick_topk / eppk_pick_random_topk)
        rp, rs = pk.pick_random_topk(wl.reqs, 3, 7, wl.mask)
        orp, ors = orc.pick_random_topk(wl.chain, wl.pods, oix, wl.reqs, wl.B, 3, 7, wl.mask)
        assert np.array_equal(rp, orp) and np.array_equal(rs.view(np.uint64), ors.view(np.uint64)), "eppk_pick_random_topk"
        tp, ts = pk.pick_topk(wl.reqs, 3, wl.mask)
        assert np.array_equal(tp[:, 0], op) and np.array_equal(ts[:, 0].view(np.uint64), os_.view(np.uint64)), "eppk_pick_topk: head of the list"
        assert all(rp[r] in tp[r] for r in range(R))
        if R <= 64:                                                    # (the oracle's list builder is a Python loop)
            otp, ots = orc.pick_topk(wl.chain, wl.pods, oix, wl.reqs, 3, wl.mask)
            assert np.array_equal(tp, otp) and np.array_equal(ts.view(np.uint64), ots.view(np.uint64)), "eppk_pick_topk"
        # a row out of range is refused on this path too, and nothing is launched
        st_reqs, _ = pk.staging(with_mask=masked)
        st_reqs[R - 1, 0] = np.uint64(1000) << np.uint64(32)
        with pytest.raises(Exception):
            pk.pick_staged(R, use_mask=masked)
        assert pk.launch_status() == 0


@pytest.mark.parametrize("R", [300, 3000, 20000])          # host loop (<= 2048 rows) / device check beside a zero-copy pick / device check behind the upload
def test_rows_out_of_range_are_reported_by_every_host_path(pkg, orc, R):
    """Request rows in pinned memory are range-checked on the device (a thread per row header) instead of by a host loop in front of the
    launch: the call still fails and names the LOWEST bad row, delivers nothing, leaves no sticky launch-status flag behind and the
    index in order -- and the next, clean batch is bit-exact against the oracle."""
    wl = pkg.workload.make_workload(5, R=R, P=4096, n_groups=16)
    oix = orc.OracleIndex()
    oix.insert(wl.index_hashes, wl.index_pods)
    op, os_, _ = orc.pick_batch(wl.chain, wl.pods, oix, wl.reqs, wl.B)
    bad = wl.reqs.copy()
    lo, hi = R // 3, R - 1
    bad[hi, 0] = np.uint64(1000) << np.uint64(32)                 # n_blocks = 1000
    bad[lo, 0] = np.uint64(200)                                   # adapter 200
    with pkg.BatchedPicker(wl.chain, max_pods=4096, max_blocks=wl.B, max_batch=R, index_slots=1 << 21) as pk:      # (room for what the LEARN batch teaches it)
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        st_reqs, _ = pk.staging()
        st_reqs[:R] = bad
        with pytest.raises(pkg.EppkError, match=f"row {lo} "):
            pk.pick_staged(R)
        with pytest.raises(pkg.EppkError, match=f"row {lo} "):
            pk.pick(bad)
        for learn in (False, True):
            b_reqs, _ = pk.stage_buffers(0)
            b_reqs[:R] = bad
            try:
                pk.stage_begin(0, R, learn=learn)
                with pytest.raises(pkg.EppkError, match=f"row {lo} "):
                    pk.stage_end(0)
            except pkg.EppkError as e:                               # (the host loop of a small batch refuses it in _begin)
                assert f"row {lo} " in str(e) and R <= 2048
        assert pk.launch_status() == 0 and pk.index_selfcheck() == 0
        # a LEARN batch with bad rows taught the index its other rows; without LEARN nothing changed: clean batches still match the oracle
        st_reqs[:R] = wl.reqs
        p, s = pk.pick_staged(R)
        if R <= 2048:                                                # (refused in _begin: the index never saw the batch)
            assert np.array_equal(p, op) and np.array_equal(s.view(np.uint64), os_.view(np.uint64))
        else:
            good = np.ones(R, dtype=bool); good[[lo, hi]] = False
            picks_learned = op.copy(); picks_learned[~good] = -1
            oix.insert_picks(bad, wl.B, picks_learned)               # what the device learned: every row but the two bad ones
            op2, os2, _ = orc.pick_batch(wl.chain, wl.pods, oix, wl.reqs, wl.B)
            assert np.array_equal(p, op2) and np.array_equal(s.view(np.uint64), os2.view(np.uint64))
            assert pk.index_size() == oix.size()
