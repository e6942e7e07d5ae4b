"""CPU: the many-chunk cases of the three load resolves (tests/resolve_chunk_cases.py) before they meet the device
(tests/test_gpu_resolve_chunks.py).

  * scan_cut / offsets_cut, the generator's model of how the scan kernels and banded_offsets_kernel cut the chunk axis, against a
    transcription of the kernels' index arithmetic;
  * the conditions a case has to meet so that it tests what it says (rc.violations): a random bounded case at >= 17 chunks has a pod's
    room end in >= 5 distinct scan segments in round 0 and >= 4 in round 1, places rows in >= 3 rounds and leaves 10 .. 40 % to the
    finish; every band of more than one row of a banded or costed case places rows in >= 2 rounds and leaves some to the finish, and a
    SPILL band spills; a saturation case takes exactly the rows the exact sums allow, and a prefix modulo 2^32 would take others;
  * every tag of REQUIRED, and SCAN_TAGS in every family;
  * the three restatements against each other where they must agree, and against the naive per-row loop of
    tests/test_bounded_ref_cpu.py on the constructed cases at 17 and 129 chunks.

The generator is the same code for every chunk size: all chunk counts at 64 rows, a few at 128 and 512 to keep this file within
seconds.  The GPU module asserts the same conditions of every case it runs."""
import importlib.util
import math
import os

import numpy as np
import pytest


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rc = _load("resolve_chunk_cases")
SHAPES = {64: rc.COUNTS + (rc.BIG,), 128: (17, 129), 512: (17, 33)}
FAMILIES = ("bounded", "banded", "costed")
U32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def cases():
    """{(chunk, n_chunks): [(family, case, the restatement's answer)]}: computed once, shared, left unchanged."""
    return {(chunk, n): [(f, c, rc.WANT[f](c)) for f, cs in rc.make_cases(chunk, n).items() for c in cs] for chunk, counts in SHAPES.items() for n in counts}


def kernel_cut(n_chunks, n_segs):
    """bounded_scan_kernel / banded_offsets_kernel, thread by thread, in 32-bit arithmetic: seg_len and per segment (c0, c1, the trips of
    `for (c = c0; c < c1; c += 8u)`)."""
    seg_len = ((n_chunks + n_segs - 1) & U32) // n_segs
    out = []
    for seg in range(n_segs):
        c0 = (seg * seg_len) & U32 if (seg * seg_len) & U32 < n_chunks else n_chunks
        c1 = (c0 + seg_len) & U32 if (c0 + seg_len) & U32 < n_chunks else n_chunks
        trips, c = 0, c0
        while c < c1:
            trips, c = trips + 1, c + 8
        out.append((c0, c1, trips))
    return seg_len, out


@pytest.mark.parametrize("cut,n_segs", [(rc.scan_cut, 16), (rc.offsets_cut, 32)])
def test_the_model_of_the_cuts_equals_the_kernels_index_arithmetic(cut, n_segs):
    for n in list(range(1, 301)) + [1024, 1025, 4096]:
        m = cut(n)
        seg_len, segs = kernel_cut(n, n_segs)
        assert m["seg_len"] == seg_len and m["segs"] == [(c0, c1) for c0, c1, _ in segs] and m["trips"] == [t for _, _, t in segs], n
        # the segments partition [0, n) in order; behind the first short one every segment is empty
        assert segs[0][0] == 0 and segs[-1][1] == n and all(a[1] == b[0] for a, b in zip(segs, segs[1:])), n
        sizes = [c1 - c0 for c0, c1, _ in segs]
        assert all(s == seg_len for s in sizes[: n // seg_len]) and sum(sizes) == n and all(s == 0 for s in sizes[n // seg_len + 1:]), n
    assert rc.scan_cut(16)["seg_len"] == 1 and rc.scan_cut(17)["seg_len"] == 2 and rc.scan_cut(128)["seg_len"] == 8 and rc.scan_cut(129)["seg_len"] == 9
    assert rc.scan_cut(257)["seg_len"] == 17 and max(rc.scan_cut(257)["trips"]) == 3 and max(rc.scan_cut(129)["trips"]) == 2
    assert rc.scan_cut(17)["segs"][8] == (16, 17) and rc.scan_cut(17)["segs"][9] == (17, 17), "a clipped segment, then empty ones"
    assert rc.offsets_cut(32)["seg_len"] == 1 and rc.offsets_cut(33)["seg_len"] == 2 and rc.offsets_cut(rc.BIG)["seg_len"] == 33


def test_every_case_meets_its_conditions(cases):
    bad = [v for (chunk, _), todo in cases.items() for f, c, want in todo for v in rc.violations(f, c, chunk, want)]
    assert not bad, bad[:8]
    for (chunk, n), todo in cases.items():
        names = [(f, c["name"]) for f, c, _ in todo]
        assert len(set(names)) == len(names), "case names are unique"
        assert any(-(-c["lists"].shape[0] // chunk) == n for _, c, _ in todo)
        assert all(c["n_pods"] <= 64 for _, c, _ in todo if n >= 128), "the scratch is n_chunks * P words"
        randoms = [c for f, c, _ in todo if f == "bounded" and "random" in c["tags"]]
        assert randoms and all(c["n_pods"] == 24 and c["lists"].shape[1] == 4 for c in randoms)
        assert all(0.08 < np.mean(c["lists"] == rc.NO) < 0.12 for c in randoms)


def test_every_required_branch_is_reached(cases):
    for chunk in SHAPES:
        tags = {f: set() for f in FAMILIES}
        for (ch, n), todo in cases.items():
            if ch == chunk:
                for f, c, _ in todo:
                    tags[f] |= c["tags"]
        have = set().union(*tags.values())
        if chunk == 64:
            assert not set(rc.REQUIRED) - have, sorted(set(rc.REQUIRED) - have)
            for f in FAMILIES:
                assert not set(rc.SCAN_TAGS) - tags[f], (f, sorted(set(rc.SCAN_TAGS) - tags[f]))
        if chunk == 512:
            assert not set(rc.REQUIRED_17_33) - have, sorted(set(rc.REQUIRED_17_33) - have)
    assert set(rc.REQUIRED_17_33) - {"seg_len=3"} <= set(rc.REQUIRED)


def test_the_tags_say_what_the_cut_does():
    assert rc.scan_tags(16) == {"seg_len=1"} and rc.scan_tags(17) == {"seg_len=2", "empty-trailing-segment", "clipped-last-segment"}
    assert rc.scan_tags(128) == {"seg_len=8"} and rc.scan_tags(129) == {"seg_len=9", "second-trip", "empty-trailing-segment", "clipped-last-segment"}
    assert rc.scan_tags(257) == {"seg_len=17", "second-trip", "third-trip", "clipped-last-segment"}
    assert rc.offsets_tags(32) == {"offsets-seg_len=1"} and rc.offsets_tags(33) == {"offsets-seg_len=2"} and rc.offsets_tags(129) == {"offsets-seg_len>2"}


def test_the_constructed_rooms_end_where_the_cut_says(cases):
    for (chunk, n), todo in cases.items():
        if n == rc.BIG:
            continue
        cut = rc.scan_cut(n)
        caps = rc.constructed_caps(chunk, n)
        assert bool(caps) == (cut["seg_len"] >= 2)
        rows = rc.n_rows(chunk, n)
        built = {f: {c["cap_all"] // (3 if f == "costed" else 1): (c, w) for f2, c, w in todo if f2 == f and "constructed" in c["tags"]} for f in ("bounded", "costed")}
        assert set(built["bounded"]) == set(caps) and (n == 16 or set(built["costed"]) == set(caps))
        for f in built:
            for T, (c, want) in built[f].items():
                assert np.all(want[0][:T] == 0) and (T == rows or want[0][T] == 1), f"{c['name']}: pod 0's room ends behind row {T - 1}"
        if not caps:
            continue
        ends = lambda tag: {T - 1 for T, tags in caps.items() if tag in tags}   # noqa: E731  (the last row pod 0 takes)
        seg_ends = [c1 * chunk for c0, c1 in cut["segs"][:-1] if c1 > c0 and c1 < n]
        some = ends("room-ends-at-segment-end")
        # the last row of a segment's last chunk, the first row of the next segment's first chunk, one row earlier, one row later
        assert sum(1 for e in seg_ends if {e - 2, e - 1, e, e + 1} <= some) >= 2
        c0 = cut["segs"][1][0]
        if cut["seg_len"] >= 9:
            e = (c0 + 8) * chunk
            assert {e - 2, e - 1, e, e + 1} <= ends("room-ends-at-trip-8"), "the 8th and the 9th chunk of segment 1"
        if cut["seg_len"] >= 17:
            e = (c0 + 16) * chunk
            assert {e - 2, e - 1, e, e + 1} <= ends("room-ends-at-trip-16"), "the 16th and the 17th chunk of segment 1"
        assert {rows - 3, rows - 2, rows - 1} <= ends("room-ends-in-last-chunk") and (rows - 2) // chunk >= n - 2


def test_the_bands_have_the_sizes_the_cases_are_for(cases):
    for (chunk, n), todo in cases.items():
        by = {c["name"]: c for f, c, _ in todo if f == "banded"}
        batch = by[f"batch-{n}x{chunk}"]
        R = batch["lists"].shape[0]
        assert R == rc.n_rows(chunk, n) and -(-R // chunk) == n
        sizes = [r.size for r in rc.band_places(batch)]
        assert sizes[2] == 0 and sizes[4] == 0 and all(sizes[b] % chunk for b in (0, 1, 3)), "no band starts on a chunk boundary"
        if chunk == 64 and n in rc.BAND_CHUNKS:
            # a band is a binomial draw of R rows at p = 1/7 .. 3/7: three standard deviations, and one chunk for the rounding up
            tol = math.ceil(3.0 * math.sqrt(R * (3 / 7) * (4 / 7)) / chunk) + 1
            assert all(abs(-(-s // chunk) - w) <= tol for s, w in zip(sizes, rc.BAND_CHUNKS[n])), (n, [-(-s // chunk) for s in sizes])
        if n == rc.BIG:
            assert {"band-mid-chunk>16", "band-mid-chunk>128", "offsets-seg_len>2"} <= batch["tags"]
            continue
        own = by[f"band1-{n}x{chunk}"]
        sizes = [r.size for r in rc.band_places(own)]
        assert sizes[1] == rc.n_rows(chunk, n) and sizes[0] % chunk and sizes[2] == 0 and sizes[4] == 0, "band 1 alone has n_chunks band-chunks"
        assert rc.scan_tags(n) <= own["tags"] and ("band-mid-chunk>16" in own["tags"]) == (n > 16)
        if n in rc.EXACT_BAND:
            a, extra = rc.EXACT_BAND[n]
            exact = by[f"band1-exactly-{a}chunk+{extra}-x{chunk}"]
            assert [r.size for r in rc.band_places(exact)][:2] == [1, a * chunk + extra] and "band-of-one-row" in exact["tags"]
        if n == 129:
            bad = by[f"bad-band-{n}x{chunk}"]
            at = np.nonzero(bad["band"] >= len(bad["bands"]))[0]
            assert at.size == 5 and len(set((at // chunk).tolist())) == 5 and at.max() // chunk == n - 1 and not rc.nc.host_ok(bad)
            assert next(w for f, c, w in todo if c is bad)[4] == rc.nc.ref.LAUNCH_BAD_REQUEST_ROW
        if n == 257:
            assert by[f"null-band-{n}x{chunk}"]["band"] is None
        if n in (17, 33):
            for f, c, _ in todo:
                if f"pods=4096-{n}" in c["tags"]:
                    L, P = c["lists"], 4096
                    seg = np.nonzero((L == P - 1).any(axis=1))[0] // chunk // rc.scan_cut(n)["seg_len"]
                    assert c["n_pods"] == P and seg.min() == 0 and (f != "bounded" or seg.max() == (n - 1) // rc.scan_cut(n)["seg_len"])


def test_the_saturation_cases_pass_2_32_where_they_say(cases):
    for chunk in (64, 128):
        todo = [(c, w) for f, c, w in cases[(chunk, 129)] if "saturation" in c["tags"]]
        assert len(todo) == 5
        cut = rc.scan_cut(129)
        span = cut["seg_len"] * chunk
        assert span * rc.MAX_COST > 1 << 32, "a segment of nine chunks totals more than 2^32"
        for c, want in todo:
            taken = np.nonzero((want[0] == 0) & (want[2] == 0))[0]
            mark = int(taken[-1]) + 1                                     # the first bidder the exact sum refuses
            assert want[0][mark] == 1 and np.all(c["cost"][c["lead"]:] == rc.MAX_COST) and np.all(want[2][(want[0] < 0) & (c["lists"][:, 0] == 0)] == rc.OVERFLOW)
            extra = np.count_nonzero(rc.modulo_takers(c)) - taken.size
            assert extra > 1000, "a prefix modulo 2^32 accepts thousands of further rows"
            if "2^32-in-segment-0" in c["tags"]:
                assert mark == 256 and mark // span == 0 and c["lead"] == 0
            if "2^32-in-later-segment" in c["tags"]:
                assert mark // span >= 3 and mark % chunk
            if "2^32-at-segment-boundary" in c["tags"]:
                assert mark % span == 0 and mark > 0
            if "2^32-at-trip-boundary" in c["tags"]:
                assert mark % chunk == 0 and (mark // chunk) % cut["seg_len"] == rc.TRIP
            if "clamped-totals-summed" in c["tags"]:
                assert c["small"] and np.all(c["cost"][: c["lead"]] == 1) and taken.size == c["lead"] + 255 and c["lead"] // span >= 3


def _same(a, b, what):
    for x, y, name in zip(a[:4], b[:4], ("picks", "scores", "ranks", "loads")):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), f"{what}: {name}"
    fa, fb = (rc.bc.ref.LAUNCH_BAD_PICK if f is True else int(f) for f in (a[4], b[4]))
    assert fa == fb, what


def test_the_three_restatements_agree_where_they_must(cases):
    """One band with reserve 0 is the bounded resolve; every cost 1 is the banded resolve (per request and per entry)."""
    for key in ((64, 17), (64, 129), (128, 17), (512, 17)):
        for i, (f, c, want) in enumerate(cases[key]):
            if f == "bounded":
                _same(rc.nc.want(rc.as_banded(c)), want, c["name"])
                if i % 4 == 0:
                    _same(rc.cc.want(rc.as_costed(rc.as_banded(c))), want, c["name"])
            if f == "banded":
                _same(rc.cc.want(rc.as_costed(c, per_entry=bool(i & 1))), want, c["name"])


def test_the_restatement_equals_the_naive_loop_on_the_constructed_cases(cases):
    naive = _load("test_bounded_ref_cpu").naive
    ran = 0
    for key in ((64, 17), (64, 129)):
        for f, c, want in cases[key]:
            if f == "bounded" and "constructed" in c["tags"]:
                _same(naive(c["lists"], c["scores"], c["n_pods"], c["cap"], c["cap_all"], c["policy"], c["load"]), want, c["name"])
                ran += 1
    assert ran >= 30


def test_locate_names_chunk_and_segment(cases):
    c = next(c for f, c, _ in cases[(64, 129)] if f == "bounded")
    assert rc.locate(c, 64, [0, 9 * 64]) == "row 0: chunk 0 segment 0, row 576: chunk 9 segment 1"
    c = next(c for f, c, _ in cases[(64, 129)] if f == "banded" and "band-of-n" in c["tags"])
    rows = rc.band_places(c)[1]
    text = rc.locate(c, 64, [rows[9 * 64]])
    assert f"row {rows[9 * 64]}: band 1 place 576 band-chunk 9 segment 1; batch chunk {rows[9 * 64] // 64}" in text
