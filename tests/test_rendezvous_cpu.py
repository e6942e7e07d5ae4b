"""CPU: what the rendezvous rule (SEMANTICS.md §3j) promises, on its numpy restatement (tests/rendezvous_ref.py)."""
import numpy as np
import rendezvous_ref as ref


def test_first_and_second_choice_spread_evenly():
    """65 536 sequential keys over 64 pods: a pod's share is binomial(65536, 1/64), mean 1024, sigma 31.7; six sigma = [832, 1216]."""
    picks, scores = ref.rendezvous(np.arange(65536, dtype=np.uint64), 2, 1, np.ones((65536, 64), dtype=bool))
    for col in (0, 1):
        n = np.bincount(picks[:, col], minlength=64)
        assert n.min() >= 832 and n.max() <= 1216, (col, n.min(), n.max())
    assert np.all(picks[:, 0] != picks[:, 1]) and np.all(scores[:, 0] >= scores[:, 1]) and np.all(scores < 1.0)


def test_a_pod_that_leaves_moves_only_its_own_requests():
    R, P, k, gone = 500, 40, 3, 17
    key = np.random.default_rng(1).integers(0, 2 ** 64, R, dtype=np.uint64)
    cand = np.ones((R, P), dtype=bool)
    full = ref.rendezvous(key, k + 1, 9, cand)[0]
    cand[:, gone] = False
    after = ref.rendezvous(key, k, 9, cand)[0]
    assert np.any(full[:, :k] == gone)
    assert all(list(new) == [p for p in old if p != gone][:k] for old, new in zip(full, after))
