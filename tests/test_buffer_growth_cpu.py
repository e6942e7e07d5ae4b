"""CPU twin of tests/test_gpu_buffer_growth.py: the capacities its sequences must cross, recomputed from the sizing rules of
csrc/eppk.hip (tests/buffer_growth_cases.py restates them), and the generator's answers held to the reference models at these shapes."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


bg = _load("buffer_growth_cases")
sc = bg.sc


def test_shapes_are_the_ones_the_sequences_are_sized_for():
    assert (bg.CFG["max_pods"], bg.CFG["max_blocks"], bg.CFG["max_batch"], bg.CFG["index_slots"]) == (130, 8, 64, 32768)
    assert bg.ENV == {"EPPK_QUAD_MIN": "4", "EPPK_BOUND_CHUNK": "64"} and bg.ROWS == (48, 700, 64, 1500)
    assert bg.ALL_ROWS[:4] == bg.ROWS and bg.PODS[:4] == (130, 130, 60, 60) and len(bg.PODS) == len(bg.ALL_ROWS) == len(bg.ALL_TOPK) == 6
    assert sorted(set(bg.PODS)) == [60, 130] and (130 + 63) // 64 == 3 and (60 + 63) // 64 == 1
    assert [r * e for r, e in bg.SUBSET_ROWS_ENTRIES] == [600, 1100, 300, 2100] and all(r <= bg.CFG["max_batch"] for r, _ in bg.SUBSET_ROWS_ENTRIES)
    assert bg.INSERT_PAIRS == (3000, 5000, 1000, 9000) and 3000 + bg.CFG["groups"] * 4 < bg.CFG["index_slots"] // 4


@pytest.mark.parametrize("buffer", bg.BUFFERS)
def test_every_sequence_replaces_twice_and_reuses_in_between(buffer):
    seen = bg.growth(buffer)
    assert seen
    for name, hist in seen.items():
        assert len(hist) == bg.steps_of(buffer)
        if name == "so_offsets":                               # max_batch + 1 offsets whatever the batch: made once
            assert hist == ["first", "reuse", "reuse", "reuse"]
            continue
        asked = [h for h in hist if h != "none"]
        assert asked[0] == "first" and asked.count("replace") >= 2, (buffer, name, hist)
        first, last = asked.index("replace"), len(asked) - 1 - asked[::-1].index("replace")
        assert "reuse" in asked[first:last], (buffer, name, hist)        # a smaller batch between two replacements reuses
        if buffer != "resolves":
            assert hist == ["first", "replace", "reuse", "replace"], (buffer, name, hist)


def test_the_resolves_need_their_two_extra_steps():
    """A batch of at most one chunk (64 rows) takes the single-launch kernel: over the four steps every case shares, the chunk histogram,
    the band order and the band histogram are made at 700 rows and replaced once, at 1500 (the histogram by 10 words: 11 chunks x 130
    pods against 24 x 60).  The steps of 200 and 3100 rows reuse and replace them again."""
    seen = bg.growth("resolves")
    for name in ("bd_hist_words", "bn_perm_rows", "bn_bh_words"):
        assert seen[name] == ["none", "first", "none", "replace", "reuse", "replace"], (name, seen[name])
    for name in ("bd_state_rows", "bd_list_rows"):
        assert seen[name] == ["first", "replace", "reuse", "replace", "reuse", "replace"], (name, seen[name])
    assert [bg.need_of("resolves", i).get("bd_hist_words") for i in range(6)] == [None, 11 * 130, None, 24 * 60, 4 * 60, 49 * 60]
    assert all(n > bg.CHUNK for n in bg.EXTRA_ROWS)


def test_capacities_at_the_thresholds_the_issue_names():
    assert [bg.need_of("subset_keys", i)["sk_entries"] for i in range(4)] == [1024, 2048, 1024, 4096]                  # doubling from 1024
    assert [bg.need_of("index_insert", i)["sortwl_words"] - 4 for i in range(4)] == [4096, 5000, 4096, 9000]         # the floor of 4096 slots
    assert [bg.need_of("learn_words", i)["learn_rows"] for i in range(4)] == [64, 700, 64, 1500]                      # the floor of max_batch rows
    assert bg.work_list_words(48, True) == 32 + 16 + 16 * 4 * 34 and bg.work_list_words(1500, False) == 32 + 376 + 376 * 4
    assert -(-1500 // 4) // 8 + 1 == 47                        # the largest grid of the sequence: not clipped on a device of 47 CUs and more


def test_the_three_resolves_take_both_forms():
    forms = [f for i in range(4) for f in bg.resolve_forms(i)]
    for kind in ("bounded", "banded", "costed"):
        assert f"pick_{kind}_device" in forms and f"resolve_{kind}_device" in forms
    assert all(len(bg.resolve_step(f, i, j)["bands"]) == 3 for i in range(4) for j, f in enumerate(bg.resolve_forms(i)) if "banded" in f)


def test_generator_answers_against_the_reference_models(orc):
    """The picks the GPU module compares with are the oracle's own, row by row (score_row), at both pod counts; the random picker's
    answer is an entry of the request's ordered list; every request a resolve places from its list gets the entry its rank names at that
    entry's score, and the load handed back is the load handed in plus what the placed requests weigh."""
    import __graft_entry__ as g
    pkg = g.load_package()
    m = bg.make_model(orc, pkg.workload)
    for i, P in ((0, 130), (2, 60)):
        m.apply(bg.publish_step(P))
        if i == 0:
            m.apply(bg.seed_step())
        assert m.P == P and m.pool.ipods == 60
        s = bg.step("pick_masked", i)
        inp, want = m.apply(s)
        for r in range(0, bg.ROWS[i], 7):
            T = orc.score_row(sc.CHAIN, m.pods, m.oix, inp["reqs"][r], inp["mask"][r])
            if want["picks"][r] >= 0:                          # the pick is a best-scoring candidate of the row, at the oracle's own total
                assert T[want["picks"][r]] == want["scores"][r] == np.max(T[np.isfinite(T)]), (i, r)
        s = bg.step("random_topk", i)
        inp, want = m.apply(s)
        lists = m._topk(inp["reqs"], s["k"])
        assert all(want["picks"][r] in lists[0][r] for r in range(bg.ROWS[i]))
        for j, form in enumerate(bg.resolve_forms(i)):
            rs = bg.resolve_step(form, i, j)
            if form.startswith("resolve_"):
                m.lists = m._topk(m.rows(rs, R=bg.ROWS[i]), rs["k"])
            inp, want = m.resolve(rs)
            lists = (inp["lists"], inp["list_scores"]) if "lists" in inp else m._topk(inp["reqs"], rs["k"], inp["mask"])
            picks, ranks, R, k = want["picks"], want["ranks"].astype(np.int64), bg.ROWS[i], inp["k"]
            assert picks.shape[0] == R and ranks.shape[0] == R
            placed = np.nonzero(picks >= 0)[0]
            listed = placed[ranks[placed] < k]                  # (a rank beyond the list: a request a spilling band placed elsewhere)
            assert listed.size, (i, form)
            # every request placed from its list got the entry its rank names, at that entry's score
            assert np.array_equal(picks[listed], lists[0][listed, ranks[listed]]), (i, form)
            assert np.array_equal(want["scores"][listed].view(np.uint64), lists[1][listed, ranks[listed]].view(np.uint64)), (i, form)
            if inp["load"] is not None and not (inp["per_entry"] and listed.size != placed.size):                        # the load handed back = the load handed in + what the placed requests weigh
                if inp["cost"] is None:
                    w = np.ones(R, dtype=np.int64)
                elif inp["per_entry"]:
                    w = inp["cost"][np.arange(R), np.minimum(ranks, k - 1)].astype(np.int64)
                else:
                    w = inp["cost"].astype(np.int64)
                took = np.bincount(picks[placed], weights=w[placed], minlength=P).astype(np.int64)
                assert np.array_equal(inp["load"].astype(np.int64) + took, want["load"].astype(np.int64)), (i, form)
    h, p = bg.insert_pairs(m, 3)
    assert h.size == 9000 and np.unique(h).size == 3000 and p.max() < 60 and np.all(np.diff(p.astype(np.int64)) >= 0)
