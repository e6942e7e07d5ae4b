"""Inputs for the three load resolves (SEMANTICS.md §3d-§3f) over MANY chunks: batches of 16 .. 257 (and once 1025) chunks, where
bounded_scan_kernel / banded_scan_kernel / costed_scan_kernel put several chunks into one of their kBoundScanSegs = 16 segments and walk
a segment in trips of eight chunks, and banded_offsets_kernel puts several chunks into one of its kBandScanSegs = 32 segments.

Pure numpy, loaded by file name like tests/bounded_cases.py.  A case has the shape the generator of its family uses, so that
bounded_cases.want / banded_cases.want / costed_cases.want answer it:
    bounded   name, tags, lists, scores, n_pods, cap, cap_all, policy, load, no_score, no_rank
    banded    ... without policy, with bands [(policy, reserve)] and band (u8 [R] or None)
    costed    ... and cost (u32 [R], or [R, k] with per_entry), per_entry
scan_cut / offsets_cut are a model of the two cuts: they say which branches a case reaches (tags), and where a differing row lies
(locate).  tests/test_resolve_chunks_cpu.py holds the model to a transcription of the kernels' index arithmetic and the generator to
REQUIRED and to the conditions its doc-string lists."""
import importlib.util
import os

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


bc = _load("bounded_cases")
nc = _load("banded_cases")
cc = _load("costed_cases")
NO, SHED, SPILL = bc.NO, bc.ref.SHED, bc.ref.SPILL
OVERFLOW = bc.ref.RANK_OVERFLOW
MAX_COST, FULL = cc.MAX_COST, cc.FULL
SEED0 = 0xC4A2

SCAN_SEGS, OFFSETS_SEGS, TRIP = 16, 32, 8        # kBoundScanSegs, kBandScanSegs, the chunks of one trip of the scan kernels' prefix loop
COUNTS = (16, 17, 31, 32, 33, 128, 129, 257)     # chunks per batch: both sides of seg_len 1/2 (scan), 1/2 (offsets), 8/9; 257: seg_len 17
BIG = 1025                                       # the production batch under a chunk of 64 rows
RAG = {16: 0, 17: 1, 31: 7, 32: -1, 33: 0, 128: 7, 129: 1, 257: -1, BIG: 9}      # rows of the last chunk: 0 = full, -1 = chunk - 1
TABLE = [(SHED, 0), (SPILL, 2), (SHED, 5), (SPILL, 9), (SHED, 9), (SPILL, 20)]
BAND_DRAW = [0, 1, 1, 1, 3, 3, 5]                # bands 2 and 4 stay empty: no band starts on a chunk boundary
BAND_CHUNKS = {129: (19, 56, 0, 36, 0, 19), 257: (38, 110, 0, 73, 0, 38), BIG: (147, 441, 0, 290, 0, 148)}    # under a chunk of 64 rows, +-2
EXACT_BAND = {16: (16, 0), 17: (16, 1), 128: (128, 0), 129: (128, 1)}            # a band of exactly a * chunk + b rows beside a band of one row
P_RANDOM, K_RANDOM = 24, 4
TAKE = (1.4, 2.8, 5.0)                          # see _band_caps

SCAN_TAGS = ["seg_len=1", "seg_len=2", "seg_len=8", "seg_len=9", "seg_len=17", "empty-trailing-segment", "clipped-last-segment", "second-trip",
             "third-trip"]
# every family (bounded, banded, costed) reaches SCAN_TAGS over COUNTS; all of them together reach REQUIRED
REQUIRED = (SCAN_TAGS + ["offsets-seg_len=1", "offsets-seg_len=2", "offsets-seg_len>2", "band-mid-chunk>16", "band-mid-chunk>128", "band-of-one-row",
                         "empty-band-between", "bad-band", "null-band", "segment-total>=2^32", "2^32-in-segment-0", "2^32-in-later-segment",
                         "2^32-at-segment-boundary", "2^32-at-trip-boundary", "clamped-totals-summed", "pods=4096-17", "pods=4096-33",
                         "room-ends-at-segment-end", "room-ends-at-trip-8", "room-ends-at-trip-16", "room-ends-in-last-chunk", "per-entry", "random",
                         "null-load", "null-score", "null-rank", "null-list-scores"])
# ... and what 17 and 33 chunks alone reach (the default chunk of 512 rows runs no more than these)
REQUIRED_17_33 = ["seg_len=2", "seg_len=3", "empty-trailing-segment", "clipped-last-segment", "offsets-seg_len=1", "offsets-seg_len=2",
                  "band-mid-chunk>16", "band-of-one-row", "empty-band-between", "pods=4096-17", "pods=4096-33", "room-ends-at-segment-end",
                  "room-ends-in-last-chunk", "per-entry", "random"]


# ---- the two cuts ----------------------------------------------------------------------------------------------------------

def _cut(n_chunks, n_segs):
    seg_len = -(-n_chunks // n_segs)
    segs = []
    for s in range(n_segs):
        c0 = min(s * seg_len, n_chunks)
        segs.append((c0, min(c0 + seg_len, n_chunks)))
    return dict(n_chunks=n_chunks, seg_len=seg_len, segs=segs, trips=[-(-(c1 - c0) // TRIP) for c0, c1 in segs])


def scan_cut(n_chunks):
    """The cut of the three scan kernels: seg_len, the [c0, c1) of the 16 segments, and the eight-wide trips each takes."""
    return _cut(n_chunks, SCAN_SEGS)


def offsets_cut(n_chunks):
    """The cut of banded_offsets_kernel: 32 segments (its write-back loop takes a chunk per trip: trips counts eights all the same)."""
    return _cut(n_chunks, OFFSETS_SEGS)


def scan_tags(n_chunks):
    cut = scan_cut(n_chunks)
    tags = {f"seg_len={cut['seg_len']}"}
    if any(c0 == c1 for c0, c1 in cut["segs"]):
        tags.add("empty-trailing-segment")
    if any(0 < c1 - c0 < cut["seg_len"] for c0, c1 in cut["segs"]):
        tags.add("clipped-last-segment")
    if max(cut["trips"]) >= 2:
        tags.add("second-trip")
    if max(cut["trips"]) >= 3:
        tags.add("third-trip")
    return tags


def offsets_tags(n_chunks):
    L = offsets_cut(n_chunks)["seg_len"]
    return {f"offsets-seg_len={L}" if L <= 2 else "offsets-seg_len>2"}


def n_rows(chunk, n_chunks, rag=None):
    rag = RAG.get(n_chunks, 0) if rag is None else rag
    return (n_chunks - 1) * chunk + (chunk if rag == 0 else chunk - 1 if rag < 0 else rag)


def band_places(c):
    """Per band b: the rows of the band in batch order -- place i of the band's segment holds rows[i]."""
    R = c["lists"].shape[0]
    bb = np.zeros(R, dtype=np.uint8) if c.get("band") is None else c["band"]
    return [np.nonzero(bb == b)[0] for b in range(len(c["bands"]))]


def band_tags(c, chunk):
    """What the batch and the bands of a banded / costed case reach."""
    R = c["lists"].shape[0]
    tags = offsets_tags(-(-R // chunk))
    sizes = [r.size for r in band_places(c)]
    start = 0
    for b, n in enumerate(sizes):
        if n:
            tags |= scan_tags(-(-n // chunk))
            if start % chunk and n > 16 * chunk:
                tags.add("band-mid-chunk>16")
            if start % chunk and n > 128 * chunk:
                tags.add("band-mid-chunk>128")
            if n == 1:
                tags.add("band-of-one-row")
        elif 0 < b < len(sizes) - 1 and sizes[b - 1] > chunk and sizes[b + 1] > chunk:
            tags.add("empty-band-between")
        start += n
    return tags


def locate(c, chunk, rows):
    """Where rows lie, as text: chunk and scan segment of the batch (bounded), or band, band-chunk and scan segment of the band's own
    segment plus the chunk and offsets segment of the batch (banded, costed)."""
    R = c["lists"].shape[0]
    out = []
    if "bands" not in c:
        L = max(1, scan_cut(-(-R // chunk))["seg_len"])
        return ", ".join(f"row {r}: chunk {r // chunk} segment {r // chunk // L}" for r in map(int, rows))
    Lo = max(1, offsets_cut(-(-R // chunk))["seg_len"])
    places = band_places(c)
    bb = np.zeros(R, dtype=np.uint8) if c["band"] is None else c["band"]
    for r in map(int, rows):
        b = int(bb[r])
        if b >= len(places):
            out.append(f"row {r}: in no band, batch chunk {r // chunk}")
            continue
        i = int(np.searchsorted(places[b], r))
        L = max(1, scan_cut(-(-places[b].size // chunk))["seg_len"])
        out.append(f"row {r}: band {b} place {i} band-chunk {i // chunk} segment {i // chunk // L}; batch chunk {r // chunk} offsets segment {r // chunk // Lo}")
    return ", ".join(out)


# ---- what happens in a case (from the restatement's ranks) -------------------------------------------------------------------

def bounded_trace(c, chunk, want):
    """Per round: the scan segments in which a pod's room ends -- the segment of the chunk of the first refused bidder of a pod that
    also has a taker in the round; the rows each round places; the share of rows left to the finish."""
    L, P = c["lists"], c["n_pods"]
    R, k = L.shape
    rank = want[2]
    valid = (L >= 0) & (L < P)
    placed = np.where(rank < k, rank, k).astype(np.int64)
    seg_len = max(1, scan_cut(-(-R // chunk))["seg_len"])
    segments = []
    for j in range(k):
        bid = valid[:, j] & (placed >= j)
        take = bid & (placed == j)
        refused = bid & ~take
        hit = set()
        for p in np.unique(L[take, j]):
            r = np.nonzero(refused & (L[:, j] == p))[0]
            if r.size:
                hit.add(int(r[0]) // chunk // seg_len)
        segments.append(hit)
    return dict(segments=segments, placed=[int(np.count_nonzero(placed == j)) for j in range(k)],
                finish=float(np.count_nonzero(rank & OVERFLOW)) / max(1, R))


def band_trace(c, want):
    """Per non-empty band: (rounds that place rows, rows left to the finish, rows spilled)."""
    k = c["lists"].shape[1]
    pick, rank = want[0], want[2]
    out = {}
    for b, rows in enumerate(band_places(c)):
        if rows.size:
            rk = rank[rows]
            left = (rk & OVERFLOW) != 0
            out[b] = (len(set(rk[rk < k].tolist())), int(np.count_nonzero(left)), int(np.count_nonzero(left & (pick[rows] != NO))))
    return out


def saturated_takers(c):
    """Round 0 of a saturation case in exact arithmetic: pod 0's bidders while their running cost stays within 2^32 - 1."""
    bids = c["lists"][:, 0] == 0
    cost = np.where(bids, c["cost"].astype(np.int64), 0)
    return bids & (np.cumsum(cost) <= FULL)


def modulo_takers(c):
    """... and with every prefix reduced modulo 2^32: the rows a device without the 64-bit sums would give pod 0."""
    bids = c["lists"][:, 0] == 0
    cost = np.where(bids, c["cost"].astype(np.int64), 0)
    S = (np.cumsum(cost) - cost) & FULL
    return bids & (S + cost <= FULL)


def violations(family, c, chunk, want):
    """The conditions a case has to meet so that it tests what its tags say (tests/test_resolve_chunks_cpu.py asserts them of every
    case, tests/test_gpu_resolve_chunks.py of the cases it runs): a list of texts, empty when all hold."""
    R = c["lists"].shape[0]
    bad = []
    if family == "bounded" and "random" in c["tags"] and -(-R // chunk) >= 17:
        t = bounded_trace(c, chunk, want)
        if len(t["segments"][0]) < 5 or len(t["segments"][1]) < 4:
            bad.append(f"the room ends in {[len(s) for s in t['segments']]} scan segments per round, want >= 5 and >= 4")
        if sum(1 for n in t["placed"] if n) < 3:
            bad.append(f"rows placed per round {t['placed']}, want three rounds")
        if not 0.10 <= t["finish"] <= 0.40:
            bad.append(f"{t['finish']:.3f} of the rows reach the finish, want 0.10 .. 0.40")
    if family != "bounded" and c["tags"] & {"random", "exact-band", "null-band"}:
        t = band_trace(c, want)
        for b, (rounds, left, spilled) in t.items():
            if band_places(c)[b].size > 1 and (rounds < 2 or left == 0):
                bad.append(f"band {b} places rows in {rounds} rounds and leaves {left} to the finish, want >= 2 and > 0")
        if not any(spilled for b, (_, _, spilled) in t.items() if c["bands"][b][0] == SPILL):
            bad.append("no SPILL band spills")
    if "saturation" in c["tags"]:
        pick, rank, load = want[0], want[2], want[3]
        exact = saturated_takers(c)
        if not np.array_equal((pick == 0) & (rank == 0), exact) or np.array_equal(modulo_takers(c), exact):
            bad.append("round 0 does not take the exact prefix, or a prefix modulo 2^32 takes the same rows")
        if np.count_nonzero((pick == 1) & (rank == 1)) != 256 or np.count_nonzero(pick >= 0) != np.count_nonzero(exact) + 256:
            bad.append("round 1 does not place 256 rows on pod 1 and leave everything else to the finish")
        if not c["small"] and (np.count_nonzero(exact) != 256 or load.tolist() != [256 * MAX_COST] * 2):
            bad.append(f"loads {load.tolist()}, want 256 rows of EPPK_MAX_COST on either pod")
    return [f"{INFO[family](c)}: {text}" for text in bad]


# ---- bounded ---------------------------------------------------------------------------------------------------------------

def _lists(rng, n, P=P_RANDOM, k=K_RANDOM):
    lists = rng.integers(0, P, size=(n, k)).astype(np.int32)
    lists[rng.random((n, k)) < 0.1] = NO
    return lists


def _caps(rng, lists, P):
    """Even pods fill in round 0 (a fraction f of their round-0 bidders), odd pods in a later round."""
    first = lists[:, 0]
    bid0 = np.bincount(first[first >= 0], minlength=P).astype(np.float64)
    f = rng.permutation((np.arange(P) + 0.5) / P)
    return np.where(np.arange(P) % 2 == 0, np.round(f * bid0), bid0 + np.round(0.45 * f * bid0)).astype(np.uint32)


def constructed_caps(chunk, n_chunks):
    """{cap: tags}: every row lists pod 0 first, so cap_all = T ends pod 0's room behind row T - 1.  The positions come from scan_cut."""
    cut = scan_cut(n_chunks)
    n = n_rows(chunk, n_chunks)
    if cut["seg_len"] < 2:
        return {}
    out = {}

    def aim(t, tag):                                                    # the room ends in row t, one row earlier, one row later
        for d in (-1, 0, 1):
            if 1 <= t + d + 1 <= n:
                out.setdefault(t + d + 1, set()).add(tag)

    full = [s for s in range(SCAN_SEGS - 1) if cut["segs"][s + 1][1] > cut["segs"][s + 1][0]]       # segments with a non-empty successor
    for s in sorted({full[0], full[len(full) // 2], full[-1]}):
        c1 = cut["segs"][s][1]
        aim(c1 * chunk - 1, "room-ends-at-segment-end")                 # the last row of the last chunk of segment s ...
        aim(c1 * chunk, "room-ends-at-segment-end")                     # ... and the first row of the first chunk of segment s + 1
    c0 = cut["segs"][1][0]
    for at, tag in ((8, "room-ends-at-trip-8"), (16, "room-ends-at-trip-16")):
        if cut["seg_len"] > at:
            aim((c0 + at) * chunk - 1, tag)                             # the last row of chunk `at` of segment 1 and the first of the next:
            aim((c0 + at) * chunk, tag)                                 # both sides of a trip of eight
    last = max(s for s in range(SCAN_SEGS) if cut["segs"][s][1] > cut["segs"][s][0])
    aim(n - 2, "room-ends-in-last-chunk")
    aim(cut["segs"][last][0] * chunk, "room-ends-in-last-chunk")        # the first chunk of the last non-empty segment
    return out


def bounded_cases(chunk, n_chunks, seeds=(1, 2), constructed=True):
    tags0 = scan_tags(n_chunks)
    n = n_rows(chunk, n_chunks)
    out = []
    for i, (T, tags) in enumerate(sorted(constructed_caps(chunk, n_chunks).items()) if constructed else ()):
        row = [[0, 1], [0, 1, 2]][i & 1]
        out.append(bc._case(f"room-{n_chunks}x{chunk}-cap{T}", tags0 | tags | {"constructed"}, np.tile(np.array([row], dtype=np.int32), (n, 1)), 3,
                            cap_all=T, policy=i & 1, load=np.zeros(3), seed=T))
    for seed in seeds:
        rng = np.random.default_rng(SEED0 + 7919 * n_chunks + chunk + seed)
        lists = _lists(rng, n)
        out.append(bc._case(f"random-{n_chunks}x{chunk}-s{seed}", tags0 | {"random"}, lists, P_RANDOM, cap=_caps(rng, lists, P_RANDOM), policy=seed & 1,
                            load=np.zeros(P_RANDOM), seed=seed))
    # outputs and loads the caller does not ask for, each at one many-chunk size
    base = out[-1]
    null = {129: ("null-load", dict(load=None)), 33: ("null-score", dict(no_score=True)), 257: ("null-rank", dict(no_rank=True)),
            17: ("null-list-scores", dict(scores=None))}
    if n_chunks in null:
        tag, change = null[n_chunks]
        out.append(dict(base, name=f"{tag}-{n_chunks}x{chunk}", tags=tags0 | {tag}, **change))
    if n_chunks in (17, 33):
        out.append(_pods_4096(chunk, n_chunks))
    return out


def _pods_4096(chunk, n_chunks):
    """The largest snapshot: 256 pod groups of the scan; the last pod takes bids in the first and in the last scan segment."""
    P = 4096
    n = n_rows(chunk, n_chunks)
    rng = np.random.default_rng(SEED0 + n_chunks + chunk + P)
    lists = bc._random_lists(rng, n, 2, P, hot=P - 1)
    lists[0], lists[n - 1] = [P - 1, 0], [P - 1, 1]
    return bc._case(f"pods-4096-{n_chunks}x{chunk}", scan_tags(n_chunks) | {f"pods=4096-{n_chunks}"}, lists, P, cap_all=5, policy=SPILL, load=np.zeros(P),
                    seed=P)


# ---- banded ----------------------------------------------------------------------------------------------------------------

def _band_caps(rng, lists, band, P, bands):
    """Ten pods that band 0 fills, five each for bands 1 and 3, four for band 5: the band's own reserve, what the bands in front are
    expected to take -- their round-0 bidders times TAKE: the more pods are full, the more refused rows come round again -- and a
    fraction of the band's own round-0 bidders: below 1 the room ends in round 0, above in a later round."""
    live = [b for b in range(len(bands)) if np.any(band == b)]
    groups = np.repeat(np.arange(4), [10, 5, 5, 4])[: P]
    groups = rng.permutation(np.concatenate([groups, np.full(max(0, P - groups.size), 3)]))
    first = lists[:, 0]
    bid = np.stack([np.bincount(first[(band == b) & (first >= 0)], minlength=P) for b in range(len(bands))]).astype(np.float64)
    caps = np.zeros(P, dtype=np.uint32)
    seen = [0, 0, 0, 0]
    for p in range(P):
        g = min(int(groups[p]), len(live) - 1)
        b = live[g]
        at = (seen[g] + 0.5) / max(1, np.count_nonzero(groups == g))    # evenly over the group's pods
        seen[g] += 1
        f = 0.25 + 0.65 * at if g == 0 else 0.4 + 1.6 * at
        caps[p] = bands[b][1] + int(round(sum(TAKE[i] * bid[x][p] for i, x in enumerate(live[:g])) + f * bid[b][p]))
    return caps


def _banded(name, tags, chunk, lists, band, cap, bands=TABLE, **kw):
    c = nc._case(name, tags, lists, P_RANDOM, bands, band, cap=cap, load=kw.pop("load", np.zeros(P_RANDOM)), **kw)
    c["tags"] |= band_tags(c, chunk)
    return c


def _band_n(rng, chunk, n_chunks):
    """Band bytes with band 1 of exactly n_chunks band-chunks (ragged as RAG says), the others a sixth, a third and a sixth of it, no
    band a multiple of the chunk."""
    n1 = n_rows(chunk, n_chunks)
    sizes = {0: n1 // 6 + 1, 1: n1, 3: n1 // 3 + 1, 5: n1 // 6 + 2}
    for b in (0, 3, 5):
        if sizes[b] % chunk == 0:
            sizes[b] += 3
    return rng.permutation(np.concatenate([np.full(s, b, dtype=np.uint8) for b, s in sizes.items()]))


def banded_cases(chunk, n_chunks):
    out = []
    rng = np.random.default_rng(SEED0 + 104729 * n_chunks + chunk)
    n = n_rows(chunk, n_chunks)
    # the batch has n_chunks chunks (what banded_offsets_kernel sees) ...
    lists = _lists(rng, n)
    band = rng.choice(BAND_DRAW, size=n).astype(np.uint8)
    caps = _band_caps(rng, lists, band, P_RANDOM, TABLE)
    out.append(_banded(f"batch-{n_chunks}x{chunk}", {"random", "batch-of-n"}, chunk, lists, band, caps, seed=n_chunks))
    null = {129: ("null-load", dict(load=None)), 33: ("null-score", dict(no_score=True)), 257: ("null-rank", dict(no_rank=True)),
            17: ("null-list-scores", dict(scores=None))}
    if n_chunks in null:
        tag, change = null[n_chunks]
        out.append(dict(out[0], name=f"{tag}-{n_chunks}x{chunk}", tags=out[0]["tags"] - {"random", "batch-of-n"} | {tag}, **change))
    if n_chunks == BIG:
        return out
    # ... and band 1 alone has n_chunks band-chunks (what the scan kernels see)
    band = _band_n(rng, chunk, n_chunks)
    lists = _lists(rng, band.size)
    out.append(_banded(f"band1-{n_chunks}x{chunk}", {"random", "band-of-n"}, chunk, lists, band, _band_caps(rng, lists, band, P_RANDOM, TABLE), seed=n_chunks + 1))
    if n_chunks in EXACT_BAND:
        a, extra = EXACT_BAND[n_chunks]
        band = np.ones(a * chunk + extra + 1, dtype=np.uint8)
        band[int(rng.integers(1, band.size - 1))] = 0                  # band 0: one row, so band 1 starts at place 1
        lists = _lists(rng, band.size)
        out.append(_banded(f"band1-exactly-{a}chunk+{extra}-x{chunk}", {"exact-band"}, chunk, lists, band, _caps(rng, lists, P_RANDOM) + 2, seed=a + extra))
    if n_chunks == 129:
        bad = out[0]["band"].copy()
        for c_at in (0, 5, 64, 127, 128):                              # in the first, the last and three distant chunks
            bad[min(n - 1, c_at * chunk + 3)] = (6, 7, 200, 255, 9)[c_at % 5]
        out.append(_banded(f"bad-band-{n_chunks}x{chunk}", {"bad-band"}, chunk, out[0]["lists"], bad, out[0]["cap"], seed=n_chunks + 2))
    if n_chunks == 257:
        lists = out[0]["lists"]
        out.append(_banded(f"null-band-{n_chunks}x{chunk}", {"null-band"}, chunk, lists, None, _caps(rng, lists, P_RANDOM) + 2, bands=[(SPILL, 2), (SHED, 3)],
                           seed=n_chunks + 3))
    if n_chunks in (17, 33):
        b = _pods_4096(chunk, n_chunks)
        c = nc._case(b["name"], b["tags"], b["lists"], 4096, [(SPILL, 0), (SHED, 2)], rng.integers(0, 2, size=n), cap_all=5, load=np.zeros(4096), seed=4096)
        c["tags"] |= band_tags(c, chunk)
        out.append(c)
    return out


# ---- costed ----------------------------------------------------------------------------------------------------------------

def _costed(b, cost, per_entry=False, **change):
    c = dict(b, cost=np.ascontiguousarray(cost, dtype=np.uint32), per_entry=per_entry, **change)
    c["tags"] = set(c["tags"])
    return c


def saturation_cases(chunk, n_chunks=129):
    """Every row lists [0, 1] at cost EPPK_MAX_COST = 2^24 - 1 under a cap of 2^32 - 1: 256 rows fit a pod, and a scan segment of nine
    chunks totals more than 2^32.  `lead` rows in front do not bid (or bid at cost 1: `small`), so that the 2^32 mark -- bidder 256 --
    falls where the name says."""
    cut = scan_cut(n_chunks)
    n = n_rows(chunk, n_chunks, 0)
    where = (("2^32-in-segment-0", 0, False), ("2^32-in-later-segment", cut["segs"][3][0] * chunk + 10, False),
             ("2^32-at-segment-boundary", cut["segs"][2][1] * chunk - 256, False),
             ("2^32-at-trip-boundary", (cut["segs"][2][0] + TRIP) * chunk - 256, False),
             ("clamped-totals-summed", cut["segs"][2][1] * chunk + 17, True))
    out = []
    for tag, lead, small in where:
        lists = np.tile(np.array([[0, 1]], dtype=np.int32), (n, 1))
        cost = np.full(n, MAX_COST, dtype=np.uint32)
        if small:
            cost[:lead] = 1
        else:
            lists[:lead] = NO
        c = cc._case(f"saturated-{tag}-{n_chunks}x{chunk}", {tag, "segment-total>=2^32", "saturation"} | scan_tags(n_chunks), lists, 2, cost,
                     [(SHED, 0)], None, cap_all=FULL, load=np.zeros(2), seed=lead)
        c["lead"], c["small"] = lead, small
        out.append(c)
    return out


def costed_cases(chunk, n_chunks):
    out = []
    rng = np.random.default_rng(SEED0 + 1299709 * n_chunks + chunk)
    for b in banded_cases(chunk, n_chunks):
        R, k = b["lists"].shape
        scale = dict(cap=None if b["cap"] is None else b["cap"] * 4, cap_all=b["cap_all"] * 4, bands=[(p, r * 4) for p, r in b["bands"]])
        out.append(_costed(b, rng.integers(1, 9, size=R), **scale))
        if "batch-of-n" in b["tags"]:
            out.append(_costed(b, rng.integers(1, 9, size=(R, k)), per_entry=True, name=b["name"] + "-per-entry", tags=b["tags"] | {"per-entry"}, **scale))
    if n_chunks not in (BIG, 16):
        # the constructed room ends, at cost 3: cap 3 T + 1 holds T rows and not T + 1
        for i, (T, tags) in enumerate(sorted(constructed_caps(chunk, n_chunks).items())):
            n = n_rows(chunk, n_chunks)
            out.append(cc._case(f"room-{n_chunks}x{chunk}-cap{T}", scan_tags(n_chunks) | tags | {"constructed"}, np.tile(np.array([[0, 1]], dtype=np.int32), (n, 1)),
                                3, np.full(n, 3), [(i & 1, 0)], None, cap_all=3 * T + 1, load=np.zeros(3), seed=T))
    if n_chunks == 129:
        out += saturation_cases(chunk, n_chunks)
    return out


# ---- the families side by side ------------------------------------------------------------------------------------------------

def as_banded(c):
    """A bounded case as a banded one: one band with reserve 0 and the case's policy."""
    b = {key: v for key, v in c.items() if key != "policy"}
    return dict(b, bands=[(c["policy"], 0)], band=None)


def as_costed(c, per_entry=False):
    """A banded case at cost 1."""
    R, k = c["lists"].shape
    return dict(c, cost=np.ones((R, k) if per_entry else R, dtype=np.uint32), per_entry=per_entry)


def make_cases(chunk, n_chunks):
    """{"bounded": [...], "banded": [...], "costed": [...]} for batches (and bands) of n_chunks chunks of `chunk` rows."""
    return dict(bounded=bounded_cases(chunk, n_chunks) if n_chunks != BIG else bounded_cases(chunk, n_chunks, seeds=(1,), constructed=False),
                banded=banded_cases(chunk, n_chunks), costed=costed_cases(chunk, n_chunks))


WANT = dict(bounded=bc.want, banded=nc.want, costed=cc.want)
INFO = dict(bounded=bc.info, banded=nc.info, costed=cc.info)
