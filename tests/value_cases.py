"""Test-side generator of SNAPSHOT values at the edges of their types: the cases on which tests/test_gpu_values.py holds the pick kernels
to the oracle.  tests/test_value_cases_cpu.py holds this generator to the coverage that module relies on, and the oracle to the numpy
restatement on the same cases.

Pure numpy, no GPU, no library.  Loaded by file name (as tests/index_placement.py and tests/wrand_ref.py are).

Every other GPU module takes its pods from workload.make_pods: queue in 0..63, kv_util a multiple of 1/1024, max_lora 4 or 8, weights
-3..5 -- values at which `1.0 - kv`, its product with the weight and most partial sums are EXACT, every queue difference fits 6 bits,
and no LoRA comparison is near its seam.  A case here is one choice of each of:

queue    "a" uniform over all of u32; "b" drawn from {0, 1, 2^31-1, 2^31, 2^31+1, 2^32-2, 2^32-1}; "c" all within 2 of 2^32-1;
         "d" all equal to 2^32-1; "e" one pod at 0, one at 2^32-1, the rest strictly between; "f" the old 0..63 (control)
kv_util  "a" uniform in [0, 1) with a full mantissa; "b" drawn from KV_SPECIALS (NaN, +-inf, -0.0, the smallest subnormal, the
         neighbours of 1.0, +-1e300, 0.1, 1/3); "c" normal(0.5, 0.5): a third outside [0, 1]; "d" the old multiples of 1/1024 (control)
LoRA     max_lora per pod from MAX_LORAS; active / waiting of a pod: all 128 bits, none, or a few bits that include the word seam
         (adapters 0, 63, 64, 127); request adapters forced to include -1, 0, 63, 64, 127
chain    0..8 scorers with weights from WEIGHTS; one of CHAIN_PLANS (empty, all-zero, all-negative, fused with 7 and 8 entries,
         interpreted tails, the shapes the library does NOT fuse, random) -- `fused_kind` restates the library's chain analysis
shape    P from PODS (every lane word, ragged last mask word), B from BLOCKS (both counter-plane widths, no index), R <= 200, a small
         prefix index, masks in half of the cases (an empty row, a single-candidate row, rows that lose every pod at the snapshot-wide
         queue minimum / maximum / both, a row that is sure to keep both), holes in a quarter

The mode letters, the chain plan and the shape of a case follow from its seed's NUMBER (seed - SEED0) by fixed strides, so that the
coverage is by construction; what is left to the seeded generator is inside the modes.
"""
from typing import Dict, List, Optional, Tuple

import numpy as np

Q, KV, L, PF = 1, 2, 3, 4
POD_DTYPE = np.dtype([("queue", "<u4"), ("running", "<u4"), ("kv_util", "<f8"), ("max_lora", "<u4"), ("flags", "<u4"),
                      ("active", "<u8", (2,)), ("waiting", "<u8", (2,)), ("reserved", "<u8")])
U32 = (1 << 32) - 1

QUEUE_MODES = ("a", "b", "c", "d", "e", "f")
KV_MODES = ("a", "b", "c", "d")
QUEUE_SPECIALS = (0, 1, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, U32 - 1, U32)
KV_SPECIALS = (float("nan"), float("inf"), float("-inf"), -0.0, 5e-324, 1.0, 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, -1e300, 1e300, 0.1, 1.0 / 3.0)
MAX_LORAS = (0, 1, 4, 8, 255, 256, 257, U32)
WEIGHTS = (-((1 << 31) - 1), (1 << 31) - 1, -65537, -1, 0, 1, 3, 7, 1000003)
SEAM_ADAPTERS = (-1, 0, 63, 64, 127)
PODS = (1, 3, 64, 65, 1000, 1500, 2500)
BLOCKS = (0, 5, 33, 70)
CHAIN_PLANS = ("empty", "zero", "negative", "fused7", "fused8", "tail7", "tail8", "short", "prefix_twice", "lora_twice", "three_trailing",
               "between", "random")

SEED0 = 31000
N_SEEDS = 104                   # 8 x 13: every chain plan eight times; 104 = 4 * 24 + 8: every (queue, kv_util) pair at least four times
# the value modes the once-per-mode tests run: every queue mode and every kv_util mode
VALUE_MODES = (("a", "a"), ("b", "b"), ("c", "c"), ("d", "a"), ("e", "b"), ("f", "d"))


def fused_kind(chain) -> int:
    """What eppk_chain_is_fused answers for `chain` (csrc/eppk.hip, the chain analysis of eppk_create), restated: behind the leading
    QUEUE / KV scorers at most four entries, among them at most one LORA, one PREFIX and two pod-only scorers.  1 = fused, 2 = fused
    with an interpreted tail (a pod-only scorer behind the leading run), 0 = the generic kernel."""
    kinds = [int(k) for k, _ in chain]
    lead = 0
    while lead < len(kinds) and kinds[lead] in (Q, KV):
        lead += 1
    nl = npf = post = 0
    for n_tail, kind in enumerate(kinds[lead:]):
        if kind == L:
            nl += 1
        elif kind == PF:
            npf += 1
        else:
            if post >= 2:
                return 0
            post += 1
        if n_tail >= 4:
            return 0
    if nl > 1 or npf > 1:
        return 0
    return 2 if post else 1


def make_req_rows(adapter, n_blocks, hashes, max_blocks: int) -> np.ndarray:
    """[R, 1 + max_blocks] u64 request rows (include/eppk.h): word 0 = adapter (i32, low half) | n_blocks << 32."""
    adapter = np.asarray(adapter, dtype=np.int32)
    rows = np.zeros((adapter.shape[0], 1 + max_blocks), dtype=np.uint64)
    rows[:, 0] = adapter.view(np.uint32).astype(np.uint64) | (np.asarray(n_blocks, dtype=np.uint64) << np.uint64(32))
    if hashes is not None and max_blocks:
        rows[:, 1:] = np.asarray(hashes, dtype=np.uint64)[:, :max_blocks]
    return rows


def mask_words(bits: np.ndarray) -> np.ndarray:
    """[R, P] bool -> [R, ceil(P / 64)] u64 mask words (bit p % 64 of word p / 64 = pod p)."""
    R, P = bits.shape
    W = (P + 63) // 64
    full = np.zeros((R, W * 64), dtype=bool)
    full[:, :P] = bits
    return np.packbits(full.reshape(R, W, 64), axis=2, bitorder="little").view(np.uint64).reshape(R, W)


def mask_bits(mask: np.ndarray, P: int) -> np.ndarray:
    """[R, W] u64 mask words -> [R, P] bool."""
    return np.unpackbits(np.ascontiguousarray(mask).view(np.uint8).reshape(mask.shape[0], -1), axis=1, bitorder="little")[:, :P].astype(bool)


# ---- values ---------------------------------------------------------------------------------------------------------------------------

def queue_values(rng, mode: str, P: int) -> np.ndarray:
    if mode == "a":
        q = rng.integers(0, 1 << 32, P, dtype=np.uint64)
    elif mode == "b":
        q = rng.choice(np.array(QUEUE_SPECIALS, dtype=np.uint64), P)
    elif mode == "c":
        q = np.uint64(U32) - rng.integers(0, 3, P, dtype=np.uint64)
    elif mode == "d":
        q = np.full(P, U32, dtype=np.uint64)
    elif mode == "e":
        q = rng.integers(1, U32, P, dtype=np.uint64)                         # strictly between the extremes
        if P >= 2:
            lo, hi = rng.choice(P, 2, replace=False)
            q[lo], q[hi] = 0, U32
        else:
            q[0] = U32
    elif mode == "f":
        q = rng.integers(0, 64, P, dtype=np.uint64)
    else:
        raise ValueError(mode)
    return q.astype(np.uint32)


def kv_values(rng, mode: str, P: int) -> np.ndarray:
    if mode == "a":
        return rng.random(P)                                                  # 53 random bits: a full mantissa
    if mode == "b":
        return rng.choice(np.array(KV_SPECIALS, dtype=np.float64), P)
    if mode == "c":
        return rng.normal(0.5, 0.5, P)
    if mode == "d":
        return rng.integers(0, 1025, P) / 1024.0
    raise ValueError(mode)


def lora_values(rng, pods: np.ndarray) -> None:
    P = pods.shape[0]
    pods["max_lora"] = rng.choice(np.array(MAX_LORAS, dtype=np.uint64), P).astype(np.uint32)
    ones = np.uint64(0xFFFFFFFFFFFFFFFF)
    for name in ("active", "waiting"):
        how = rng.integers(0, 4, P)                                           # 0: all 128 bits, 1: none, 2 / 3: a few bits, the seam among them
        words = np.zeros((P, 2), dtype=np.uint64)
        words[how == 0] = ones
        for p in np.nonzero(how >= 2)[0]:
            some = list(rng.integers(0, 128, int(rng.integers(0, 5)))) + [a for a in (0, 63, 64, 127) if rng.random() < 0.4]
            for a in some:
                words[p, int(a) >> 6] |= np.uint64(1) << np.uint64(int(a) & 63)
        pods[name] = words


def make_pods(rng, P: int, qmode: str, kvmode: str) -> np.ndarray:
    pods = np.zeros(P, dtype=POD_DTYPE)
    pods["queue"] = queue_values(rng, qmode, P)
    pods["running"] = rng.integers(0, 256, P)
    pods["kv_util"] = kv_values(rng, kvmode, P)
    lora_values(rng, pods)
    return pods


# ---- chains ---------------------------------------------------------------------------------------------------------------------------

def _w(rng, n, pool=WEIGHTS) -> List[int]:
    return [int(x) for x in rng.choice(np.array(pool, dtype=np.int64), n)]


def _pod_only(rng, n) -> List[int]:
    return [int(x) for x in rng.choice([Q, KV], n)]


def make_chain(rng, plan: str) -> Tuple[List[Tuple[int, int]], int]:
    """(chain, the kind eppk_chain_is_fused must report for it)."""
    tails = ([], [L], [PF], [L, PF], [PF, L])
    if plan == "empty":
        kinds, want = [], 1
    elif plan in ("zero", "negative", "random"):
        kinds = [int(x) for x in rng.choice([Q, KV, L, PF], int(rng.integers(1 if plan != "random" else 0, 9)))]
        want = None
    elif plan in ("fused7", "fused8"):                                        # leading run + P / LP / PL: no interpreted tail, the quad route
        n = 7 if plan == "fused7" else 8
        tail = tails[int(rng.integers(2, 5))]
        kinds, want = _pod_only(rng, n - len(tail)) + tail, 1
        kinds[0] = Q                                                          # (a QUEUE term in base[]: the snapshot-wide normalisers)
    elif plan in ("tail7", "tail8"):                                          # ... + one or two trailing pod-only scorers
        n = 7 if plan == "tail7" else 8
        tail = tails[int(rng.integers(1, 5))]
        post = int(rng.integers(1, 3))
        kinds, want = _pod_only(rng, n - len(tail) - post) + tail + _pod_only(rng, post), 2
        kinds[-1] = Q                                                         # (a QUEUE term behind the tail: post[] embeds the normalisers)
    elif plan == "short":
        tail = tails[int(rng.integers(0, 5))]
        post = int(rng.integers(0, 3)) if tail else 0
        kinds = _pod_only(rng, int(rng.integers(0, 4))) + tail + _pod_only(rng, post)
        want = 2 if post else 1
    elif plan == "prefix_twice":
        kinds, want = _pod_only(rng, int(rng.integers(0, 3))) + [PF] + [int(x) for x in rng.choice([Q, KV, L], int(rng.integers(0, 3)))] + [PF], 0
    elif plan == "lora_twice":
        kinds, want = _pod_only(rng, int(rng.integers(0, 3))) + [L] + [int(x) for x in rng.choice([Q, KV, PF], int(rng.integers(0, 3)))] + [L], 0
    elif plan == "three_trailing":
        kinds, want = _pod_only(rng, int(rng.integers(0, 3))) + tails[int(rng.integers(1, 5))] + _pod_only(rng, 3), 0
    elif plan == "between":                                                   # a pod-only scorer between L and P: an interpreted tail
        pair = [L, PF] if rng.random() < 0.5 else [PF, L]
        kinds, want = _pod_only(rng, int(rng.integers(0, 3))) + [pair[0]] + _pod_only(rng, 1) + [pair[1]], 2
    else:
        raise ValueError(plan)
    n = len(kinds)
    if plan == "zero":
        weights = [0] * n
    elif plan == "negative":
        weights = _w(rng, n, [w for w in WEIGHTS if w < 0])
    else:
        weights = _w(rng, n)
    chain = list(zip(kinds, weights))
    return chain, fused_kind(chain) if want is None else want


# ---- a case ---------------------------------------------------------------------------------------------------------------------------

def make_case(seed: int, qmode: Optional[str] = None, kvmode: Optional[str] = None, plan: Optional[str] = None, P: Optional[int] = None,
              B: Optional[int] = None, R: Optional[int] = None, masked: Optional[bool] = None, holes: Optional[bool] = None,
              chain: Optional[List[Tuple[int, int]]] = None) -> Dict:
    """Case `seed`; the keyword arguments pin what the seed's number would choose."""
    n = seed - SEED0
    rng = np.random.default_rng(seed)
    qmode = QUEUE_MODES[n % 6] if qmode is None else qmode
    kvmode = KV_MODES[(n // 6) % 4] if kvmode is None else kvmode
    plan = CHAIN_PLANS[n % 13] if plan is None else plan
    P = PODS[(n + n // 7) % 7] if P is None else P
    if B is None:                                                             # (fused7 / fused8: an index and six counter planes -- what the quad route needs)
        B = (5, 33)[(n // 13) % 2] if plan in ("fused7", "fused8") else BLOCKS[(n + n // 13) % 4]
    r_draw = int(rng.integers(8, 201))
    if R is None:
        R = (1, 2, 3)[(n // 19) % 3] if n % 19 == 18 else r_draw
    masked = bool((n // 2 + n // 26) % 2) if masked is None else masked
    holes = bool(n % 4 == 3) if holes is None else holes
    if chain is None:
        chain, kind = make_chain(rng, plan)
    else:
        chain, kind, plan = [(int(k), int(w)) for k, w in chain], fused_kind(chain), "given"
    pods = make_pods(rng, P, qmode, kvmode)
    if holes and P > 1:
        pods["flags"] = (rng.random(P) < rng.choice([0.05, 0.5])).astype(np.uint32)
        pods["flags"][int(rng.integers(0, P))] = 0                            # (never all of them)
    live = (pods["flags"] & 1) == 0

    # index: a few chains of random hashes (sometimes the reserved values), each block cached on a few pods (test_gpu_fuzz._case)
    n_chains = int(rng.integers(1, 6))
    chains = rng.integers(1, 2 ** 63, (n_chains, max(B, 1)), dtype=np.uint64)
    if rng.random() < 0.3:
        chains[0, 0] = 0
    if rng.random() < 0.3 and B > 1:
        chains[-1, 1] = np.uint64(0xFFFFFFFFFFFFFFFF)
    ih, ip = [], []
    for ci in range(n_chains):
        depth = int(rng.integers(0, B + 1))
        for b in range(depth):
            for pod in rng.integers(0, P, int(rng.integers(1, 6))):
                ih.append(chains[ci, b]); ip.append(pod)
    ih = np.asarray(ih, dtype=np.uint64); ip = np.asarray(ip, dtype=np.uint32)
    n_keys = max(len(set(ih.tolist())), 1)
    slots = 64
    while slots < (2 if rng.random() < 0.3 else 4) * n_keys:
        slots *= 2
    hs = chains[rng.integers(0, n_chains, R)].copy()
    for r in range(R):                                                        # break chains at random depths
        if B and rng.random() < 0.7:
            cut = int(rng.integers(0, B))
            hs[r, cut:] = rng.integers(1, 2 ** 63, B - cut, dtype=np.uint64)
    nblk = rng.integers(0, B + 1, R) if B else np.zeros(R, dtype=np.int64)
    adapter = rng.integers(-1, 128, R)
    at = np.arange(len(SEAM_ADAPTERS)) + (6 if R >= 11 else 0)                # behind the mask's constructed rows where there is room
    adapter[at[at < R]] = np.array(SEAM_ADAPTERS)[: int((at < R).sum())]
    reqs = make_req_rows(adapter, nblk, hs[:, :B] if B else None, B)

    mask = None
    if masked:
        bits = rng.random((R, P)) < rng.choice([0.1, 0.5, 0.9])
        q = pods["queue"]
        qlo, qhi = (q[live].min(), q[live].max()) if live.any() else (0, 0)
        bits[0] = False                                                       # no candidate
        if R > 1:
            bits[1] = False; bits[1, int(rng.integers(0, P))] = True          # one (a hole now and then: none then)
        for r, drop in ((2, q == qlo), (3, q == qhi), (4, (q == qlo) | (q == qhi))):
            if r < R:                                                         # every pod at a snapshot-wide QUEUE extreme is gone ...
                bits[r] = (rng.random(P) < 0.8) & ~drop
        if R > 5:                                                             # ... and a row that keeps one pod of either
            bits[5, int(np.nonzero(live & (q == qlo))[0][0])] = True
            bits[5, int(np.nonzero(live & (q == qhi))[0][0])] = True
        mask = mask_words(bits)
    return dict(seed=seed, qmode=qmode, kvmode=kvmode, plan=plan, chain=chain, kind=kind, pods=pods, ih=ih, ip=ip, slots=slots, reqs=reqs,
                mask=mask, P=P, B=B, R=R, k=1 + n % 5)


def quad_route_exists(c: Dict) -> bool:
    """Whether a batch of the case takes pick_quad_kernel under EPPK_QUAD_MIN=4 (csrc/eppk.hip launch_pick): a fused chain without an
    interpreted tail, a PREFIX scorer, an index, six counter planes, four requests."""
    return c["kind"] == 1 and any(k == PF for k, _ in c["chain"]) and 1 <= c["B"] <= 63 and c["R"] >= 4


def pods_of(seed: int) -> int:
    """P of case `seed` without building it."""
    n = seed - SEED0
    return PODS[(n + n // 7) % 7]


def info(c: Dict) -> str:
    return (f"seed {c['seed']}: chain {c['chain']} ({c['plan']}, kind {c['kind']}) queue mode {c['qmode']} kv_util mode {c['kvmode']} "
            f"P {c['P']} B {c['B']} R {c['R']} masked {c['mask'] is not None} holes {int((c['pods']['flags'] & 1).sum())} slots {c['slots']}")


def index_dict(c: Dict) -> Dict[int, set]:
    """The case's prefix index as {hash: set(pod)} for tests/golden/gen_golden.py (pairs that name a hole are ignored, as on the device)."""
    hole = (c["pods"]["flags"] & 1).astype(bool)
    out: Dict[int, set] = {}
    for h, p in zip(c["ih"].tolist(), c["ip"].tolist()):
        if not hole[p]:
            out.setdefault(h, set()).add(p)
    return out


def request_fields(c: Dict):
    """(adapter i32 [R], n_blocks u32 [R], hashes u64 [R, max(B, 1)]) of the case's request rows."""
    w0 = c["reqs"][:, 0]
    adapter = (w0 & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    hashes = c["reqs"][:, 1:] if c["B"] else np.zeros((c["R"], 1), dtype=np.uint64)
    return adapter, (w0 >> np.uint64(32)).astype(np.uint32), hashes
