"""The picker "rendezvous" (SEMANTICS.md §3j) in plain numpy: unsigned wrapping arithmetic, a stable sort on (-h, p)."""
import numpy as np

U64, U32 = np.uint64, np.uint32


def splitmix64(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def fold(m):
    return (m ^ (m >> U64(32))).astype(U32)


def fmix32(h):
    with np.errstate(over="ignore"):
        h = (h ^ (h >> U32(16))) * U32(0x85EBCA6B)
        h = (h ^ (h >> U32(13))) * U32(0xC2B2AE35)
    return h ^ (h >> U32(16))


def prefix_keys(reqs, depth):
    """key[r] = hash[min(depth, n_blocks) - 1] of row r (word 0 = adapter | n_blocks << 32, then the hashes), 0 without blocks."""
    at = np.minimum((reqs[:, 0] >> U64(32)).astype(np.int64), depth)
    return np.where(at > 0, reqs[np.arange(len(reqs)), at], U64(0)).astype(U64)


def candidates(n_reqs, n_pods, flags=None, mask=None):
    """[R, P] bool: the mask (bit b of word j = pod 64j + b) AND not a hole."""
    ok = np.ones((n_reqs, n_pods), dtype=bool)
    if mask is not None:
        ok = (((mask[:, :, None] >> np.arange(64, dtype=U64)) & U64(1)) != 0).reshape(n_reqs, -1)[:, :n_pods]
    return ok if flags is None else ok & ((flags & 1) == 0)


def rendezvous(key, k, seed, cand, pod_key=None):
    """([R, k] int32 picks, [R, k] float64 scores) of the u64 keys [R] over the candidate matrix [R, P]."""
    R, P = cand.shape
    with np.errstate(over="ignore"):
        a = fold(splitmix64(key + U64(seed) * U64(0x9E3779B97F4A7C15)))
    c = fold(splitmix64(np.arange(P, dtype=U64) if pod_key is None else pod_key))
    picks, scores = np.full((R, k), -1, dtype=np.int32), np.zeros((R, k))
    for r in range(R):
        pods = np.nonzero(cand[r])[0]
        h = fmix32(a[r] ^ c[pods])
        o = np.argsort(-h.astype(np.int64), kind="stable")[:k]         # pods ascend: a stable sort breaks ties by p
        picks[r, :o.size], scores[r, :o.size] = pods[o], h[o] * 2.0 ** -32
    return picks, scores
