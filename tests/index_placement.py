"""Test-side planner for the prefix index (protocol v5): builds keys that land EXACTLY where a test wants them -- in their home bucket, one
or two buckets further on, wrapped from the last bucket to the front of the table, or nowhere (absent, behind an overflowed or a plain home
bucket) -- so that the pick kernels' code for displaced keys is reached on purpose instead of by the accident of a crowded table.

Pure numpy, no GPU.  Loaded by file name (as tests/wrand_ref.py is); tests/test_index_placement_cpu.py holds the planner to its word with
`Table`, a restatement of where csrc/eppk_kernels.hip.h index_insert_one puts a new key.

The table: index_slots / 4 buckets of 64 bytes, five key words each.  A key goes into the first free word of its home bucket; a full bucket
gets its "overflowed" flag set and the key moves on to the next bucket, modulo the bucket count.
"""
from dataclasses import dataclass, field
from typing import Dict, List, Sequence, Tuple

import numpy as np

KEYS_PER_BUCKET = 5
HOME_MUL = 0x9E3779B1
TOMB = 0xFFFFFFFFFFFFFFFF

# placements of one key of a chain
HOME = "h"            # in its home bucket
D1 = "d1"             # home bucket full: one bucket further on
D2 = "d2"             # home bucket and the one behind it full: two buckets further on
WRAP = "w"            # home = the LAST bucket, full: lives at the front of the table (bucket 0, or further on once that is full too)
TOMB_D1 = "t"         # as D1, but the fillers of the home bucket are to be tombstoned afterwards (Plan.tomb_fillers: insert them on a pod of
                      # their own, remove that pod when the chains are in): five tombstones, the flag still set, the key one bucket on
ABSENT_OVF = "ao"     # never inserted; its home bucket is full and overflowed (a look-up has to walk, and finds nothing)
ABSENT = "a"          # never inserted; its home bucket is empty
PLACEMENTS = (HOME, D1, D2, WRAP, TOMB_D1, ABSENT_OVF, ABSENT)


def n_buckets(index_slots: int) -> int:
    nb = int(index_slots) // 4
    if nb < 2 or nb & (nb - 1):
        raise ValueError(f"index_slots = {index_slots}: the bucket count must be a power of two >= 2")
    return nb


def home_bucket(h, index_slots: int):
    """Home bucket of a block hash as libeppk computes it (eppk_kernels.hip.h home_bucket): the top log2(buckets) bits of
    (lo ^ hi) * 0x9E3779B1 mod 2^32."""
    lg = n_buckets(index_slots).bit_length() - 1
    h = np.asarray(h, dtype=np.uint64)
    f = (h & np.uint64(0xFFFFFFFF)) ^ (h >> np.uint64(32))
    return (((f * np.uint64(HOME_MUL)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - lg)).astype(np.int64)


def keys_for_buckets(buckets: Sequence[int], counts: Sequence[int], index_slots: int, seed: int, max_draws: int = 1 << 26) -> List[np.ndarray]:
    """counts[i] distinct 64-bit keys (never 0 / ~0) whose home bucket is buckets[i], by rejection from a generator seeded with `seed`.
    Raises if `max_draws` candidates do not yield them."""
    nb = n_buckets(index_slots)
    buckets = np.asarray(buckets, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    if buckets.size != np.unique(buckets).size or (buckets < 0).any() or (buckets >= nb).any():
        raise ValueError("keys_for_buckets: buckets must be distinct and inside the table")
    need = np.zeros(nb, dtype=np.int64)
    need[buckets] = counts
    rng = np.random.default_rng(seed)
    got_b, got_k = [], []
    drawn = 0
    chunk = 1 << 20
    while need.sum() > 0:
        if drawn >= max_draws:
            raise RuntimeError(f"keys_for_buckets: {int(need.sum())} keys still missing after {drawn} candidates")
        cand = rng.integers(1, 0xFFFFFFFFFFFFFFFF, chunk, dtype=np.uint64)       # [1, ~0): neither reserved hash
        drawn += chunk
        hb = home_bucket(cand, index_slots)
        sel = np.nonzero(need[hb] > 0)[0]
        if sel.size == 0:
            continue
        order = sel[np.argsort(hb[sel], kind="stable")]
        b_sorted = hb[order]
        first = np.searchsorted(b_sorted, b_sorted, side="left")               # rank of a candidate among those of its bucket
        keep = (np.arange(order.size) - first) < need[b_sorted]
        got_b.append(b_sorted[keep])
        got_k.append(cand[order[keep]])
        need -= np.bincount(b_sorted[keep], minlength=nb)
    if not got_b:
        return [np.zeros(0, dtype=np.uint64) for _ in buckets]
    allb = np.concatenate(got_b)
    allk = np.concatenate(got_k)
    if np.unique(allk).size != allk.size:
        raise RuntimeError("keys_for_buckets: the generator repeated a key")
    order = np.argsort(allb, kind="stable")
    allb, allk = allb[order], allk[order]
    lo = np.searchsorted(allb, buckets, side="left")
    return [allk[l:l + c] for l, c in zip(lo.tolist(), counts.tolist())]


class Table:
    """Where index_insert_one puts NEW keys (model_insert below): words[bucket][0..4] (0 = empty, TOMB = tombstone), flags[bucket]."""

    def __init__(self, index_slots: int) -> None:
        self.index_slots = int(index_slots)
        self.nb = n_buckets(index_slots)
        self.words: Dict[int, List[int]] = {}
        self.flags: set = set()
        self.at: Dict[int, Tuple[int, int]] = {}             # live key -> (bucket, word)

    def insert(self, h: int) -> Tuple[int, int]:
        h = int(h)
        if h in self.at:
            return self.at[h]
        b = int(home_bucket(np.uint64(h), self.index_slots))
        for _ in range(self.nb):
            w = self.words.setdefault(b, [0] * KEYS_PER_BUCKET)
            free = [i for i, k in enumerate(w) if k in (0, TOMB)]
            # (the device searches the whole chain for the key first and takes the first free word it passed: the same word as long as no
            #  tombstone sits in an EARLIER bucket of the chain than the first free word of this one -- the planner never builds that)
            if free:
                w[free[0]] = h
                self.at[h] = (b, free[0])
                return self.at[h]
            self.flags.add(b)                                # full: flag the bucket, go on to the next one
            b = (b + 1) % self.nb
        raise RuntimeError("table full")

    def tombstone(self, h: int) -> None:
        b, i = self.at.pop(int(h))
        self.words[b][i] = TOMB

    def live(self) -> int:
        return len(self.at)

    def non_empty_words(self) -> int:
        return sum(1 for w in self.words.values() for k in w if k != 0)

    def distance(self, h: int) -> int:
        """Buckets between a live key and its home bucket (modulo the bucket count)."""
        return (self.at[int(h)][0] - int(home_bucket(np.uint64(int(h)), self.index_slots))) % self.nb


def model_insert(calls: Sequence[Tuple[str, np.ndarray]], index_slots: int) -> Table:
    """The table after the plan's insert calls, in order (keys of one call in array order: the plan makes the order irrelevant)."""
    t = Table(index_slots)
    for _, keys in calls:
        for h in keys.tolist():
            t.insert(h)
    return t


@dataclass
class Plan:
    index_slots: int
    spec: List[List[str]]
    chains: List[np.ndarray]                                   # per row: its keys, absent ones included
    calls: List[Tuple[str, np.ndarray]]                        # ordered insert calls: ("filler" | "tomb" | "chain" | "spill" | "wrap", keys)
    want: Dict[int, Tuple[int, bool]]                          # inserted chain key -> (bucket distance from home, wrapped past the last bucket)
    absent: Dict[int, bool] = field(default_factory=dict)     # absent chain key -> home bucket overflowed

    @property
    def fillers(self) -> np.ndarray:
        return np.concatenate([k for kind, k in self.calls if kind in ("filler", "spill")] + [np.zeros(0, dtype=np.uint64)])

    @property
    def tomb_fillers(self) -> np.ndarray:
        return np.concatenate([k for kind, k in self.calls if kind == "tomb"] + [np.zeros(0, dtype=np.uint64)])

    def n_keys(self) -> int:
        return sum(k.size for _, k in self.calls)


def plan(rows: Sequence[Sequence[str]], index_slots: int, seed: int) -> Plan:
    """rows[r][i] = the wanted placement of key i of row r's chain (PLACEMENTS).  Every planned key gets home and spill buckets of its own
    (nothing else of the plan hashes there), so where a key lands does not depend on the order in which one insert launch handles its
    pairs.  The exception is WRAP, of which a table has only one home -- its last bucket: all wrapped keys share it, and go in five per
    call, so that call n fills bucket n of the front of the table (distance n + 1 from the last bucket).

    Order of the calls: fillers (five per bucket to be filled) and the fillers to be tombstoned; the chains' keys together with the
    sixth key that overflows the home bucket of an ABSENT_OVF key; the wrapped keys, five per call."""
    nb = n_buckets(index_slots)
    rows = [list(r) for r in rows]
    for r in rows:
        for p in r:
            if p not in PLACEMENTS:
                raise ValueError(f"unknown placement {p!r}")
    n_wrap = sum(r.count(WRAP) for r in rows)
    wrap_buckets = (n_wrap + KEYS_PER_BUCKET - 1) // KEYS_PER_BUCKET
    cursor = wrap_buckets + 1 if n_wrap else 0                 # (one empty bucket behind the wrapped keys ends their chain)
    need: Dict[int, int] = {}
    slots: List[List[Tuple[str, int]]] = []                    # per row, per key: (placement, home bucket)
    for r in rows:
        out = []
        for p in r:
            if p == WRAP:
                out.append((p, nb - 1))
                continue
            b = cursor
            if p == HOME or p == ABSENT:
                need[b] = 1; cursor += 1
            elif p in (D1, TOMB_D1):
                need[b] = 6; cursor += 2
            elif p == D2:
                need[b] = 6; need[b + 1] = 5; cursor += 3
            else:                                              # ABSENT_OVF: five fillers, the sixth that overflows, the key itself
                need[b] = 7; cursor += 2
            out.append((p, b))
        slots.append(out)
    if n_wrap:
        need[nb - 1] = KEYS_PER_BUCKET + n_wrap
    if cursor >= nb - 1:
        raise RuntimeError(f"plan: {cursor} buckets wanted, the table has {nb}")
    bs = sorted(need)
    got = dict(zip(bs, keys_for_buckets(bs, [need[b] for b in bs], index_slots, seed)))
    taken = {b: 0 for b in bs}

    def take(b: int, n: int) -> np.ndarray:
        k = got[b][taken[b]:taken[b] + n]
        taken[b] += n
        assert k.size == n
        return k

    fill, tomb, chain_keys, spill, wrapped = [], [], [], [], []
    want: Dict[int, Tuple[int, bool]] = {}
    absent: Dict[int, bool] = {}
    chains = []
    if n_wrap:
        fill.append(take(nb - 1, KEYS_PER_BUCKET))
    for out in slots:
        ch = []
        for p, b in out:
            if p in (D1, D2):
                fill.append(take(b, KEYS_PER_BUCKET))
                if p == D2:
                    fill.append(take(b + 1, KEYS_PER_BUCKET))
            elif p == TOMB_D1:
                tomb.append(take(b, KEYS_PER_BUCKET))
            elif p == ABSENT_OVF:
                fill.append(take(b, KEYS_PER_BUCKET))
                spill.append(take(b, 1))
            h = int(take(b, 1)[0])
            ch.append(h)
            if p == WRAP:
                want[h] = (len(wrapped) // KEYS_PER_BUCKET + 1, True)
                wrapped.append(h)
            elif p in (ABSENT, ABSENT_OVF):
                absent[h] = p == ABSENT_OVF
            else:
                want[h] = ({HOME: 0, D1: 1, TOMB_D1: 1, D2: 2}[p], False)
                chain_keys.append(h)
        chains.append(np.array(ch, dtype=np.uint64))
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint64)
    calls = [("filler", cat(fill)), ("tomb", cat(tomb)), ("chain", np.array(chain_keys, dtype=np.uint64)), ("spill", cat(spill))]
    for i in range(0, len(wrapped), KEYS_PER_BUCKET):
        calls.append(("wrap", np.array(wrapped[i:i + KEYS_PER_BUCKET], dtype=np.uint64)))
    calls = [(kind, k) for kind, k in calls if k.size]
    return Plan(int(index_slots), rows, chains, calls, want, absent)


def verify(p: Plan) -> Table:
    """Table (the restatement of the device's insert) applied to the plan's calls puts every key where the plan says; raises otherwise.
    The GPU module calls this too, so that it never runs on a plan that places nothing.  Returns the table BEFORE any tombstoning."""
    t = model_insert(p.calls, p.index_slots)
    for h, (d, wrapped) in p.want.items():
        home = int(home_bucket(np.uint64(h), p.index_slots))
        if t.distance(h) != d or (home + d >= t.nb) != wrapped:
            raise AssertionError(f"key {h:#x}: planned {d} buckets from home {home}, the model puts it {t.distance(h)} away")
        for n in range(d):                                     # every bucket on the way is full and flagged
            b = (home + n) % t.nb
            if b not in t.flags or 0 in t.words[b]:
                raise AssertionError(f"key {h:#x}: bucket {b} on its way is not full and flagged")
    for h, ovf in p.absent.items():
        home = int(home_bucket(np.uint64(h), p.index_slots))
        if h in t.at or (home in t.flags) != ovf:
            raise AssertionError(f"absent key {h:#x}: home bucket {home} overflowed = {home in t.flags}, planned {ovf}")
    if t.live() >= p.index_slots // 2 or t.non_empty_words() >= 3 * (KEYS_PER_BUCKET * t.nb) // 4:
        raise AssertionError(f"the plan overloads the table: {t.live()} live keys in {p.index_slots} slots")
    return t
