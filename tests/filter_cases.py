"""Test-side generator of FILTER cases (SEMANTICS.md §2c): snapshots with values at the edges of their types (tests/value_cases.py's
make_pods), four filter programs, class bytes, candidate masks and request rows, on which the GPU tests hold the library to the numpy
restatement (tests/filter_ref.py).  tests/test_filter_ref_cpu.py holds this generator to the coverage those tests rely on.

Pure numpy, no GPU, no library.  Loaded by file name.

A case has four programs:
  0  the FUZZ program: four stages whose (kind, policy) pairs follow from the seed's NUMBER -- stage s of case n has pair
     (n + 5 s) mod 12 of PAIRS, so twelve consecutive seeds put every pair into every stage position -- and whose thresholds are drawn
     from the snapshot's own gauges, +-1 (integers) or +-1 ulp (kv_util): the values at which a compare flips
  1  [RUNNING_LE rmin PREFER]      rmin = the smallest `running` of a live pod (the generator makes sure not all live pods share it)
  2  [QUEUE_LE 2^32-1 REQUIRE, QUEUE_WITHIN 2^32-1 PREFER, RUNNING_LE 2^32-1 REQUIRE]     passes every candidate
  3  [RUNNING_LE rmin REQUIRE]
and its first rows are CONSTRUCTED so that every outcome class occurs whatever the seed draws:
  row 0  class 2, every pod         -> untouched        row 3  class 3, every live pod but those at rmin -> shed
  row 1  class 1, every pod         -> narrowed         row 4  class 3, no pod at all                    -> C_0 empty, verdict 0
  row 2  class 1, every live pod but those at rmin -> waived
  row 5  a random row whose last mask word carries bits >= n_pods (when P is no multiple of 64)
The other rows draw class, adapter (SEAM_ADAPTERS) and mask density at random."""
import importlib.util
import os
from typing import Dict, Optional

import numpy as np


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


vc = _load("value_cases")
ref = _load("filter_ref")

U32 = (1 << 32) - 1
PAIRS = tuple((k, pol) for k in ref.KINDS for pol in ref.POLICIES)          # 12 (kind, policy) pairs
PODS = (2, 63, 64, 65, 130, 1000, 4096)
SEED0 = 47000
N_SEEDS = 24                                                                 # two rounds of the twelve pairs: every queue / kv_util mode, holes on and off
MIN_ROWS = 8


def fuzz_pairs(n: int):
    return [PAIRS[(n + 5 * s) % 12] for s in range(4)]


def _threshold(rng, pods, kind):
    P = pods.shape[0]
    p, p2 = int(rng.integers(0, P)), int(rng.integers(0, P))
    d = int(rng.integers(-1, 2))
    if kind == ref.QUEUE_LE:
        return min(max(int(pods["queue"][p]) + d, 0), U32)
    if kind == ref.RUNNING_LE:
        return min(max(int(pods["running"][p]) + d, 0), U32)
    if kind == ref.KV_LE:
        x = np.float64(pods["kv_util"][p])
        return float(x if d == 0 else np.nextafter(x, np.float64(np.inf if d > 0 else -np.inf)))
    if kind == ref.QUEUE_WITHIN:
        return min(max(abs(int(pods["queue"][p]) - int(pods["queue"][p2])) + d, 0), U32)
    return 0


def make_case(seed: int, P: Optional[int] = None, R: Optional[int] = None, holes: Optional[bool] = None, qmode: Optional[str] = None,
              kvmode: Optional[str] = None, B: int = 0) -> Dict:
    """Case `seed`; the keyword arguments pin what the seed's number would choose.  B = hash slots of a request row (all zero here)."""
    n = seed - SEED0
    rng = np.random.default_rng(seed)
    P = PODS[(n + n // 7) % 7] if P is None else P
    assert P >= 1                                                            # (P = 1: no request can be narrowed; the GPU tests' smallest shape)
    qmode = vc.QUEUE_MODES[n % 6] if qmode is None else qmode
    kvmode = vc.KV_MODES[(n // 6) % 4] if kvmode is None else kvmode
    holes = bool(n % 3 == 1) if holes is None else holes
    R = int(rng.integers(MIN_ROWS, 97)) if R is None else R
    pods = vc.make_pods(rng, P, qmode, kvmode)
    if holes:
        pods["flags"] = (rng.random(P) < rng.choice([0.05, 0.5])).astype(np.uint32)
        keep = rng.choice(P, min(2, P), replace=False)
        pods["flags"][keep] = 0                                              # (at least two live pods)
    live = (pods["flags"] & 1) == 0
    lp = np.nonzero(live)[0]
    if np.all(pods["running"][lp] == pods["running"][lp[0]]):                # not every live pod at the minimum
        r0 = int(pods["running"][lp[-1]])
        pods["running"][lp[-1]] = r0 + 1 if r0 < U32 else r0 - 1            # (a different value whatever the draw: no wrap at 2^32 - 1)
    rmin = int(pods["running"][lp].min())
    at_min = live & (pods["running"] == rmin)

    programs = [
        [(k, pol, _threshold(rng, pods, k)) for k, pol in fuzz_pairs(n)],
        [(ref.RUNNING_LE, ref.PREFER, rmin)],
        [(ref.QUEUE_LE, ref.REQUIRE, U32), (ref.QUEUE_WITHIN, ref.PREFER, U32), (ref.RUNNING_LE, ref.REQUIRE, U32)],
        [(ref.RUNNING_LE, ref.REQUIRE, rmin)],
    ]
    cls = rng.choice(np.array([0, 0, 0, 1, 2, 3], dtype=np.uint8), R)
    adapter = rng.choice(np.array(vc.SEAM_ADAPTERS, dtype=np.int32), R)
    dens = rng.choice([0.02, 0.5, 0.95, 1.0], R)
    bits = rng.random((R, P)) < dens[:, None]
    W = (P + 63) // 64
    cls[:5] = (2, 1, 1, 3, 3)[: min(R, 5)]
    for r, row in enumerate((np.ones(P, bool), np.ones(P, bool), live & ~at_min, live & ~at_min, np.zeros(P, bool))):
        if r < R:
            bits[r] = row
    mask = ref.pack(bits)
    if R > 5 and P % 64:
        mask[5, W - 1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(P % 64)  # bits that name no pod
    reqs = vc.make_req_rows(adapter, np.zeros(R, dtype=np.uint64), None, B)
    return dict(seed=seed, P=P, R=R, B=B, pods=pods, programs=programs, cls=cls, adapter=adapter, mask=mask, reqs=reqs, qmode=qmode, kvmode=kvmode,
                holes=holes, pairs=fuzz_pairs(n))


def outcomes(c: Dict, cand: np.ndarray, verdict: np.ndarray) -> Dict[str, np.ndarray]:
    """The four outcome classes of a case's rows, given the restatement's answer: name -> [R] bool."""
    live = (c["pods"]["flags"] & 1) == 0
    c0 = ref.unpack(c["mask"], c["P"]) & live
    n0, nn = c0.sum(axis=1), cand.sum(axis=1)
    prefer = np.zeros(c["R"], dtype=np.uint8)
    for r in range(c["R"]):
        prog = c["programs"][int(c["cls"][r])]
        for s, (_, pol, _) in enumerate(prog):
            if pol == ref.PREFER:
                prefer[r] |= 1 << s
    return dict(untouched=(verdict == 0) & np.all(cand == c0, axis=1),
                narrowed=(nn > 0) & (nn < n0),
                waived=(verdict & prefer) != 0,
                shed=(verdict & ref.SHED) != 0)


def info(c: Dict) -> str:
    return f"seed {c['seed']}: P {c['P']} R {c['R']} queue mode {c['qmode']} kv_util mode {c['kvmode']} holes {c['holes']} fuzz pairs {c['pairs']}"
