"""CPU: the picker "weighted-random" (SEMANTICS.md §3c) -- its C ABI is declared and exported by name, and the numpy restatement
that the GPU tests compare against gets hand-worked cases right."""
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["eppk_pick_weighted_random", "eppk_pick_weighted_random_device", "eppk_group_pick_weighted_random"]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ref():
    return _load("wrand_ref", os.path.join(ROOT, "tests", "wrand_ref.py"))


def test_header_declares_and_lib_lists_the_entry_points():
    with open(os.path.join(ROOT, "include", "eppk.h")) as f:
        hdr = f.read()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", hdr), n
    with open(os.path.join(ROOT, "gateway-api-inference-extension_amd", "_lib.py")) as f:
        src = f.read()
    syms = re.search(r"SYMBOLS = \[(.*?)\]", src, re.S).group(1)
    for n in NAMES:
        assert f'"{n}"' in syms, n


def _word_for(x_frac):
    """A word u whose (u >> 11) * 2^-53 is x_frac (a multiple of 2^-53 in [0, 1))."""
    return np.uint64(int(round(x_frac * 2 ** 53)) << 11)


def test_three_pods_weights_1_2_1_intervals(ref):
    t = np.array([[1.0, 2.0, 1.0]])
    cand = np.ones((1, 3), dtype=bool)
    # S = 4: x in [0, 1) -> pod 0, [1, 3) -> pod 1, [3, 4) -> pod 2
    for frac, want in [(0.0, 0), (0.2, 0), (0.25, 1), (0.5, 1), (0.7, 1), (0.75, 2), (0.99, 2)]:
        assert ref.choose(t, cand, [_word_for(frac)])[0] == want, frac
    u = np.uint64(0xFFFFFFFFFFFFFFFF)           # the largest word: x = (1 - 2^-53) * S
    assert ref.choose(t, cand, [u])[0] == 2


def test_x_equal_to_S_takes_the_left_branch_at_an_empty_right_subtree(ref):
    w = np.array([[1.0, 2.0, 1.0]])
    lv = ref.tree(w)
    S = lv[12][0, 0]
    assert S == 4.0
    # x == S: every empty right subtree (B == 0) sends the descent left, so it ends on the last positive leaf, not on a hole
    assert ref.descend(lv, np.array([S]))[0] == 2
    # leaf order, not pod order: pod 130 sits at leaf 130, pod 7 at leaf 448
    w2 = np.zeros((1, 200))
    w2[0, 130] = 0.5
    w2[0, 7] = 0.25
    lv2 = ref.tree(w2)
    assert ref.descend(lv2, np.array([lv2[12][0, 0]]))[0] == 7
    assert ref.descend(lv2, np.array([0.0]))[0] == 130
    assert ref.descend(lv2, np.array([0.5]))[0] == 7


def test_all_totals_non_positive_take_the_uniform_fallback(ref):
    t = np.array([[-1.0, 0.0, -3.0, np.nan, -2.0]])
    cand = ~np.isnan(t)
    idx = np.array([0, 1, 2, 4])
    for u in [0, 1, 2, 3, 7, 0xFFFFFFFFFFFFFFFF]:
        assert ref.choose(t, cand, [np.uint64(u)])[0] == idx[u % 4]
    p, s = ref.weighted_random(t, 4, 5, [0])
    assert sorted(p[0].tolist()) == [0, 1, 2, 4]
    assert np.array_equal(s[0], t[0, p[0]])


def test_k_above_the_candidate_count_pads(ref):
    t = np.full((2, 10), np.nan)
    t[0, 3] = 1.5
    t[0, 8] = -0.5
    p, s = ref.weighted_random(t, 4, 11, [0, 1])
    assert p[0, 0] == 3 and p[0, 1] == 8          # the positive one first (S > 0), then the fallback among what is left
    assert s[0, 0] == 1.5 and s[0, 1] == -0.5
    assert list(p[0, 2:]) == [-1, -1] and list(s[0, 2:]) == [0.0, 0.0]
    assert list(p[1]) == [-1] * 4 and list(s[1]) == [0.0] * 4


@pytest.mark.parametrize("P", [100, 4096])
def test_leaf_order(ref, P):
    lam = ref.leaf_order(P)
    p = np.arange(P)
    assert np.array_equal(lam, 64 * (p % 64) + p // 64)
    assert np.unique(lam).size == P
    w = np.arange(1, P + 1, dtype=np.float64)[None, :]
    L = ref.leaves(w)
    assert np.array_equal(L[0, lam], w[0])
    assert np.count_nonzero(L) == P
    if P == 4096:
        assert np.array_equal(np.sort(lam), p)
    else:                                          # pod 64j + l sits in column l at position j
        assert lam[65] == 65 and lam[64] == 1 and lam[99] == 64 * 35 + 1


def test_tree_is_the_pairwise_sum(ref):
    rng = np.random.default_rng(3)
    w = rng.random((3, 300))
    lv = ref.tree(w)
    assert len(lv) == 13 and lv[12].shape == (3, 1)
    L = ref.leaves(w)

    def pairwise(x):
        return x[0] if x.size == 1 else pairwise(x[0::2] + x[1::2])
    for r in range(3):
        assert lv[12][r, 0] == pairwise(L[r])


def test_words_round_zero_is_the_random_top_k_word(ref):
    seed, r = 0xDEADBEEFCAFEF00D, 17
    z = (seed + (r + 1) * 0x9E3779B97F4A7C15) % 2 ** 64
    z ^= z >> 30; z = z * 0xBF58476D1CE4E5B9 % 2 ** 64
    z ^= z >> 27; z = z * 0x94D049BB133111EB % 2 ** 64
    z ^= z >> 31
    assert int(ref.words(seed, [r], 0)[0]) == z
    assert int(ref.words(seed, [r], 1)[0]) != z


def test_sampling_follows_the_weights(ref):
    # 300 pods, 40 000 draws of one row: counts against R*w/S (chi-square, bins with expectation >= 5), no w == 0 pod picked
    rng = np.random.default_rng(7)
    t = rng.normal(0.5, 1.0, 300)
    R = 40000
    p, _ = ref.weighted_random(np.broadcast_to(t, (R, 300)), 1, 12345, np.arange(R))
    w = np.where(t > 0, t, 0.0)
    assert np.all(w[p[:, 0]] > 0)
    cnt = np.bincount(p[:, 0], minlength=300).astype(np.float64)
    exp = R * w / w.sum()
    keep = exp >= 5
    chi2 = float(((cnt[keep] - exp[keep]) ** 2 / exp[keep]).sum())
    df = int(keep.sum()) - 1
    assert (chi2 - df) / np.sqrt(2 * df) < 6
