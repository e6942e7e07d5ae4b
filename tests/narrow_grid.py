"""Test-side helpers for tests/test_gpu_narrow_grid.py: the narrow launch geometries, the grid the launch code computes for them, and the
generator that puts chosen kinds of blocks next to each other IN TIME inside one wavefront.

Pure numpy, no GPU.  Loaded by file name (as tests/index_placement.py is); tests/test_narrow_grid_cpu.py holds the generator to its word.

Every pick kernel is a persistent loop: wavefront w of `nwaves` takes block w, then w + nwaves, and so on -- a block is four request rows
in pick_quad_kernel, one row in pick_fast_kernel and the generic kernel.  Block b is therefore trip b // nwaves of wavefront b % nwaves.
The loops are unrolled twice (the landing registers `qa` / `qb` swap roles), so a trip has a PARITY, and the quad kernel loads rows two
blocks ahead, so what a block can inherit comes from the one or two blocks in front of it in the same wavefront.
"""
from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

# ---- geometries -------------------------------------------------------------------------------------------------------------------------
# EPPK_MAX_CU clamps the CU count the persistent grids are sized from, EPPK_MAX_WG_PER_CU the workgroups per CU; with both at 1 a launch
# is ONE workgroup.  max_cu / quad / fast / generic: the CU clamp and the threads per workgroup of the three kernels (library defaults
# 512 / 1024 / 512; the generic kernel has no knob).
GEOMETRIES = {
    "g1w8": ({"EPPK_MAX_CU": "1", "EPPK_MAX_WG_PER_CU": "1"}, dict(max_cu=1, quad=512, fast=1024, generic=512)),
    "g3w8": ({"EPPK_MAX_CU": "3", "EPPK_MAX_WG_PER_CU": "1"}, dict(max_cu=3, quad=512, fast=1024, generic=512)),
    "g1w1": ({"EPPK_MAX_CU": "1", "EPPK_MAX_WG_PER_CU": "1", "EPPK_QUAD_THREADS": "64", "EPPK_FAST_THREADS": "64"},
             dict(max_cu=1, quad=64, fast=64, generic=512)),
}
GEOMETRY_KNOBS = ("EPPK_MAX_CU", "EPPK_MAX_WG_PER_CU", "EPPK_QUAD_THREADS", "EPPK_FAST_THREADS")
ROWS_PER_BLOCK = {"quad": 4, "fast": 1, "generic": 1}


def ceil_div(a: int, b: int) -> int:
    return -(-int(a) // int(b))


def expected_grid(kernel: str, n_reqs: int, geometry: str) -> Tuple[int, int]:
    """(workgroups, threads) of a launch of `kernel` ("quad" | "fast" | "generic") over n_reqs rows under a geometry whose
    EPPK_MAX_WG_PER_CU is 1: one workgroup per wavefront-load of blocks, at most max_cu of them (csrc/eppk.hip launch_pick)."""
    g = GEOMETRIES[geometry][1]
    threads = g[kernel]
    blocks = ceil_div(n_reqs, ROWS_PER_BLOCK[kernel])
    return max(1, min(ceil_div(blocks, threads // 64), g["max_cu"])), threads


def trips(kernel: str, n_reqs: int, grid: int, threads: int) -> int:
    """Loop trips of the busiest wavefront: ceil(blocks / (grid * threads / 64))."""
    return ceil_div(ceil_div(n_reqs, ROWS_PER_BLOCK[kernel]), grid * (threads // 64))


# ---- ordered neighbours -------------------------------------------------------------------------------------------------------------------
# The kinds of block the generator arranges.  What a kind IS -- which rows of which corpus -- is the GPU module's business
# (test_gpu_narrow_grid.py block_rows); here a kind is a name.
KINDS = ("short",        # plain short rows: every walk stops below 16 hits
         "none",         # nothing cached
         "m17",          # exactly 17 hits: the wavefront refetches keys 17..31 into the probe registers
         "home32",       # 32 hits, every key in its home bucket
         "d16_17",       # keys 16 and 17 displaced: the two sides of the refetch
         "d16_31",       # keys 16..31 displaced
         "miss_ovf",     # a walk that ends in a miss behind an overflowed bucket
         "twosets",      # two pod sets: the group's list, then one pod
         "tomb",         # a home bucket of tombstones, the keys one bucket on
         "reserved",     # a reserved hash among the blocks: the row is deferred
         "parked",       # masked: candidates that miss the QUEUE extremes: the row is parked
         "nocand")       # masked: no candidate at all
FILL = "short"


@dataclass
class Schedule:
    nwaves: int
    kinds: List[str]                                        # kind of block b, in batch order
    placed: Dict[Tuple[str, ...], List[Tuple[int, int]]]    # strip (a, b) or (a, b, c) -> [(wavefront, first trip)] where it was put

    @property
    def n_trips(self) -> int:
        return len(self.kinds) // self.nwaves

    def kind_at(self, wave: int, trip: int) -> str:
        return self.kinds[trip * self.nwaves + wave]


def triples_of(kinds: Sequence[str]) -> List[Tuple[str, str, str]]:
    """A few triples: every kind once in the middle, between its two cyclic neighbours in reversed order, and once three times in a row
    where that says something (state that accumulates: deferred, parked, refetched)."""
    n = len(kinds)
    out = [(kinds[(i + 1) % n], kinds[i], kinds[(i - 1) % n]) for i in range(n)]
    out += [(k, k, k) for k in kinds if k in ("m17", "reserved", "parked", "d16_31")]
    return out


def neighbour_schedule(nwaves: int, kinds: Sequence[str] = KINDS) -> Schedule:
    """Every ordered pair (a, b) of `kinds` -- a == b included -- on consecutive trips of one wavefront, once with a on an even trip and once
    on an odd one; the triples of triples_of() the same way.  Strips go to the wavefront that has the fewest blocks so far, behind one
    FILL block where the parity asks for it; all wavefronts are then filled up to the same number of trips, so that the batch is a full
    rectangle of nwaves x trips blocks."""
    strips = [((a, b), p) for a in kinds for b in kinds for p in (0, 1)] + [(t, p) for t in triples_of(kinds) for p in (0, 1)]
    cols: List[List[str]] = [[] for _ in range(nwaves)]
    placed: Dict[Tuple[str, ...], List[Tuple[int, int]]] = {}
    for strip, parity in strips:
        w = min(range(nwaves), key=lambda c: (len(cols[c]), c))
        if len(cols[w]) % 2 != parity:
            cols[w].append(FILL)
        placed.setdefault(tuple(strip), []).append((w, len(cols[w])))
        cols[w].extend(strip)
    T = max(len(c) for c in cols)
    T += T % 2                                              # an even trip count: the last strip of a column is never the loop's early exit
    for c in cols:
        c.extend([FILL] * (T - len(c)))
    return Schedule(nwaves, [cols[w][t] for t in range(T) for w in range(nwaves)], placed)


def runs_in(kinds: Sequence[str], nwaves: int, length: int) -> Dict[Tuple[str, ...], set]:
    """What a batch really contains, from the block order alone: every run of `length` consecutive trips of one wavefront -> the parities
    (first trip modulo 2) at which it occurs.  Block b is trip b // nwaves of wavefront b % nwaves."""
    out: Dict[Tuple[str, ...], set] = {}
    n = len(kinds)
    for b in range(n):
        idx = [b + i * nwaves for i in range(length)]
        if idx[-1] >= n:
            break
        out.setdefault(tuple(kinds[i] for i in idx), set()).add((b // nwaves) % 2)
    return out
