"""The metric predicates of the Filter phase (SEMANTICS.md §2c) restated in numpy: the reference of the filter tests.

Written from §2c alone, in plain loops over requests and stages and boolean arrays over the pods.  No GPU, no library; loaded by file
name (as tests/wrand_ref.py is).  A program is a list of stages (kind, on_empty, threshold): the threshold is `u` for the integer kinds,
`f` for KV_LE, and ignored by the LoRA kinds."""
import numpy as np

QUEUE_LE, RUNNING_LE, KV_LE, LORA_LOADED, LORA_SERVABLE, QUEUE_WITHIN = 1, 2, 3, 4, 5, 6
REQUIRE, PREFER = 0, 1
SHED, BAD_CLASS = 0x40, 0x80
KINDS = (QUEUE_LE, RUNNING_LE, KV_LE, LORA_LOADED, LORA_SERVABLE, QUEUE_WITHIN)
POLICIES = (REQUIRE, PREFER)


def unpack(mask: np.ndarray, P: int) -> np.ndarray:
    """[R, W] u64 mask words -> [R, P] bool (bits >= P are dropped: they name no pod)."""
    mask = np.ascontiguousarray(mask, dtype=np.uint64)
    return np.unpackbits(mask.view(np.uint8).reshape(mask.shape[0], -1), axis=1, bitorder="little")[:, :P].astype(bool)


def pack(bits: np.ndarray) -> np.ndarray:
    """[R, P] bool -> [R, ceil(P / 64)] u64 mask words (bit p % 64 of word p / 64 = pod p)."""
    R, P = bits.shape
    W = (P + 63) // 64
    full = np.zeros((R, W * 64), dtype=bool)
    full[:, :P] = bits
    return np.packbits(full.reshape(R, W, 64), axis=2, bitorder="little").view(np.uint64).reshape(R, W)


def _popcount128(words: np.ndarray) -> np.ndarray:
    """[P, 2] u64 -> [P] number of set bits."""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(words.shape[0], 16), axis=1).sum(axis=1).astype(np.int64)


def _holds(pods: np.ndarray, a: int) -> np.ndarray:
    """[P] bool: adapter a (0..127) is in active[p] or waiting[p]."""
    w, b = a >> 6, np.uint64(a & 63)
    return (((pods["active"][:, w] | pods["waiting"][:, w]) >> b) & np.uint64(1)).astype(bool)


def predicate(pods: np.ndarray, kind: int, thr, adapter: int, C: np.ndarray) -> np.ndarray:
    """[P] bool: pred_s(r, p) for every pod; C = the candidate set as the stage finds it (QUEUE_WITHIN's minimum ranges over it)."""
    P = pods.shape[0]
    if kind == QUEUE_LE:
        return pods["queue"].astype(np.int64) <= int(thr)
    if kind == RUNNING_LE:
        return pods["running"].astype(np.int64) <= int(thr)
    if kind == KV_LE:
        with np.errstate(invalid="ignore"):
            return pods["kv_util"] <= np.float64(thr)                        # raw IEEE: NaN on either side is False
    if kind in (LORA_LOADED, LORA_SERVABLE):
        if adapter < 0:
            return np.ones(P, dtype=bool)                                    # the base model needs no slot
        held = _holds(pods, adapter)
        if kind == LORA_LOADED:
            return held
        loaded = _popcount128(pods["active"]) + _popcount128(pods["waiting"])
        return held | (loaded < pods["max_lora"].astype(np.int64))
    if kind == QUEUE_WITHIN:
        if not C.any():
            return np.zeros(P, dtype=bool)
        q = pods["queue"].astype(np.int64)
        return (q - int(q[C].min())) <= int(thr)                             # (over C the difference is >= 0; outside C the answer is not used)
    raise ValueError(kind)


def filter_masks(pods: np.ndarray, programs, adapter, cls=None, mask=None):
    """§2c for a batch.  pods: the snapshot rows (as they stand now: assumed-load bumps included); programs: list of programs; adapter
    [R] int; cls [R] or None (program 0); mask [R, W] u64 words or None.  Returns ([R, P] bool C_n, [R] u8 verdict)."""
    P = pods.shape[0]
    adapter = np.asarray(adapter, dtype=np.int64)
    R = adapter.shape[0]
    live = (pods["flags"] & 1) == 0
    cand = np.zeros((R, P), dtype=bool)
    verdict = np.zeros(R, dtype=np.uint8)
    bits = None if mask is None else unpack(mask, P)
    for r in range(R):
        C = live.copy() if bits is None else (bits[r] & live)               # C_0: the mask, minus holes, minus bits >= n_pods
        v = 0
        if len(programs):
            g = 0 if cls is None else int(cls[r])
            if g >= len(programs):
                C = np.zeros(P, dtype=bool)
                v = BAD_CLASS
            else:
                for s, (kind, on_empty, thr) in enumerate(programs[g]):
                    if not C.any():
                        break                                                # nothing happens, no bit
                    K = C & predicate(pods, int(kind), thr, int(adapter[r]), C)
                    if K.any():
                        C = K
                    else:
                        v |= 1 << s
                        if int(on_empty) == REQUIRE:
                            C = np.zeros(P, dtype=bool)
                            v |= SHED
        cand[r] = C
        verdict[r] = v
    return cand, verdict


def filter_mask_words(pods, programs, adapter, cls=None, mask=None):
    """filter_masks with the candidate rows as u64 words: what the library returns."""
    cand, verdict = filter_masks(pods, programs, adapter, cls, mask)
    return pack(cand), verdict
