"""The picker "weighted-random" (SEMANTICS.md §3c) restated in numpy: the reference of the weighted-random tests.

Totals come from elsewhere (the oracle's score_row: NaN = not a candidate); this module only restates the sampling rule."""
import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
LEVELS = 12                                  # 2^12 = 4096 leaves


def splitmix64(z) -> np.ndarray:
    """The mixer of random-top-k (SEMANTICS.md §3b), on uint64 arrays (wrapping arithmetic)."""
    z = np.asarray(z, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def words(seed: int, r, i: int) -> np.ndarray:
    """u = splitmix64(seed + (r+1) * 0x9E3779B97F4A7C15 + i) mod 2^64 for batch indices r, round i."""
    r = np.asarray(r, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + (r + np.uint64(1)) * GOLDEN + np.uint64(i)
    return splitmix64(z)


def leaf_order(P: int) -> np.ndarray:
    """lambda(p) = 64 * (p mod 64) + p // 64: the leaf of pod p."""
    p = np.arange(P, dtype=np.int64)
    return 64 * (p % 64) + p // 64


def leaves(w: np.ndarray) -> np.ndarray:
    """[R, P] weights -> [R, 4096] leaves (pod p at leaf lambda(p), +0.0 where there is no pod)."""
    w = np.atleast_2d(np.asarray(w, dtype=np.float64))
    R, P = w.shape
    x = np.zeros((R, 4096), dtype=np.float64)
    x[:, :P] = w
    return x.reshape(R, 64, 64).transpose(0, 2, 1).reshape(R, 4096)


def tree(w: np.ndarray) -> list:
    """Levels N_0 .. N_12 of the weights' tree: N_{m+1}[q] = N_m[2q] + N_m[2q+1], one binary64 add each."""
    lv = [leaves(w)]
    for _ in range(LEVELS):
        x = lv[-1]
        lv.append(x[:, 0::2] + x[:, 1::2])
    return lv


def descend(lv: list, x: np.ndarray) -> np.ndarray:
    """From the root: at children A, B go to A if B == 0 or x < A, else x -= A and go to B.  Returns the pods reached."""
    R = lv[0].shape[0]
    rows = np.arange(R)
    x = np.array(x, dtype=np.float64, copy=True).reshape(R)
    q = np.zeros(R, dtype=np.int64)
    for m in range(LEVELS - 1, -1, -1):
        a = lv[m][rows, 2 * q]
        b = lv[m][rows, 2 * q + 1]
        left = (b == 0.0) | (x < a)
        x = np.where(left, x, x - a)
        q = 2 * q + (~left).astype(np.int64)
    return 64 * (q % 64) + q // 64              # lambda is its own inverse


def choose(t: np.ndarray, cand: np.ndarray, u: np.ndarray) -> np.ndarray:
    """One round (step 6) for every row: t [R, P] totals, cand [R, P] bool (C_i), u [R] uint64 words.  -1 where C_i is empty."""
    t = np.atleast_2d(t)
    cand = np.atleast_2d(cand)
    R = t.shape[0]
    u = np.asarray(u, dtype=np.uint64).reshape(R)
    pos = cand & (np.where(cand, t, 0.0) > 0.0)
    w = np.where(pos, t, 0.0)
    lv = tree(w)
    S = lv[LEVELS][:, 0]
    x = ((u >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) * S
    pick = descend(lv, x)
    n = cand.sum(axis=1)
    for r in np.nonzero((S == 0.0) & (n > 0))[0]:       # uniform over C_i, ascending pod order
        idx = np.nonzero(cand[r])[0]
        pick[r] = idx[int(u[r] % np.uint64(idx.size))]
    pick[n == 0] = -1
    return pick


def weighted_random(T: np.ndarray, k: int, seed: int, r_index, cand: np.ndarray = None):
    """The whole rule: T [R, P] totals (NaN = not a candidate unless `cand` is given), rows at batch indices r_index.
    Returns ([R, k] int32 picks, [R, k] float64 scores), padded with -1 / 0.0."""
    T = np.atleast_2d(np.asarray(T, dtype=np.float64))
    R = T.shape[0]
    cand = (~np.isnan(T)) if cand is None else np.array(cand, dtype=bool, copy=True)
    r_index = np.asarray(r_index, dtype=np.uint64).reshape(R)
    picks = np.full((R, k), -1, dtype=np.int32)
    scores = np.zeros((R, k), dtype=np.float64)
    rows = np.arange(R)
    for i in range(k):
        p = choose(T, cand, words(seed, r_index, i))
        ok = p >= 0
        picks[ok, i] = p[ok]
        scores[ok, i] = T[rows[ok], p[ok]]
        cand[rows[ok], p[ok]] = False
    return picks, scores
