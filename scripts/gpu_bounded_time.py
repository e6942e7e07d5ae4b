"""Picker "best-score under per-pod caps" (SEMANTICS.md §3d) at full size: C5 (64k requests x 4096 pods, full chain + prefix index), k = 4.

Times eppk_pick_bounded_device under both policies with cap_all at 1x, 2x and 4x ceil(R / P), the resolve alone over the same lists
(eppk_bounded_resolve_device), and -- in the same process, alternating with them -- eppk_pick_topk_device(k = 4), the part the picker cannot
avoid, and eppk_pick_weighted_random_device(k = 1), the alternative it competes with; HIP events on the launch stream after a warm-up,
`--rounds` rounds of `--reps` calls each, median / min / max over the rounds.  Per setting: the busiest pod's request count and the share
of requests at each rank and in overflow.  The last batch of every setting is checked against tests/bounded_ref.py over the lists
eppk_pick_topk_device delivered: a timing of wrong picks is worth nothing.  One JSON line.

`--topk-only` times eppk_pick_topk_device(k = 4) alone and touches nothing newer: what to run from a checkout of the PARENT commit in the
same session, for the figure the bounded picker is held against."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def _ref():
    spec = importlib.util.spec_from_file_location("bounded_ref", os.path.join(ROOT, "tests", "bounded_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="timed calls per leg and round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds of the alternating legs")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--topk-only", action="store_true")
    args = ap.parse_args()
    import torch
    pkg = g.load_package()
    wl = pkg.workload.make_workload(5)
    R, P, k = wl.reqs.shape[0], wl.pods.shape[0], args.k
    fair = -(-R // P)
    with pkg.BatchedPicker(wl.chain, max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots) as pk:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        lib = pk._lib
        st = torch.cuda.Stream()
        torch.cuda.set_stream(st)
        s = st.cuda_stream
        d_reqs = torch.from_numpy(wl.reqs.view(np.int64)).cuda()
        d_lists = torch.empty((R, k), dtype=torch.int32, device="cuda")
        d_ls = torch.empty((R, k), dtype=torch.float64, device="cuda")
        d_pick = torch.empty(R, dtype=torch.int32, device="cuda")
        d_score = torch.empty(R, dtype=torch.float64, device="cuda")
        d_rank = torch.empty(R, dtype=torch.uint8, device="cuda")
        d_load = torch.zeros(P, dtype=torch.int32, device="cuda")

        def topk():
            rc = lib.eppk_pick_topk_device(pk._ctx, d_reqs.data_ptr(), R, None, k, d_lists.data_ptr(), d_ls.data_ptr(), s)
            assert rc == 0, rc
        legs = {f"topk{k}": topk}
        settings = []
        if not args.topk_only:
            legs["wrand_k1"] = lambda: pk.pick_weighted_random_device(d_reqs.data_ptr(), R, None, 1, 7, d_pick.data_ptr(), d_score.data_ptr(), s)
            for policy, pname in ((0, "shed"), (1, "spill")):
                for mult in (1, 2, 4):
                    settings.append((f"{pname}_cap{mult}x", policy, mult * fair))
            for name, policy, cap in settings:
                # (no load array: the picker starts every batch from zeros, as the timed loop must)
                legs["bounded_" + name] = (lambda policy=policy, cap=cap: pk.pick_bounded_device(
                    d_reqs.data_ptr(), R, None, k, None, cap, policy, None, d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr(), s))
                legs["resolve_" + name] = (lambda policy=policy, cap=cap: pk.bounded_resolve_device(
                    d_lists.data_ptr(), d_ls.data_ptr(), R, k, None, cap, policy, None, d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr(), s))
        for f in legs.values():                 # warm-up: code objects, occupancy queries, scratch
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {n: [] for n in legs}
        for _ in range(args.rounds):
            for n, f in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(args.reps):
                    f()
                e1.record(st)
                e1.synchronize()
                times[n].append(e0.elapsed_time(e1) * 1e3 / args.reps)
        out = {n: {"us_median": float(np.median(v)), "us_min": float(np.min(v)), "us_max": float(np.max(v))} for n, v in times.items()}
        out["shape"], out["k"], out["reps"], out["rounds"] = f"{R} x {P}", k, args.reps, args.rounds
        if not args.topk_only:
            ref = _ref()
            out["geometry"] = dict(zip(("chunk", "one_launch_max"), pk.bounded_geometry()))
            topk()
            torch.cuda.synchronize()
            lists, totals = d_lists.cpu().numpy(), d_ls.cpu().numpy()
            bp, _ = pk.pick(wl.reqs)
            wp, _ = pk.pick_weighted_random(wl.reqs, 7, 1)
            assert np.array_equal(lists[:, 0], bp)
            out["busiest_pod"] = {"best_score": int(np.bincount(bp[bp >= 0], minlength=P).max()),
                                  "weighted_random": int(np.bincount(wp[:, 0][wp[:, 0] >= 0], minlength=P).max())}
            out["settings"] = {}
            for name, policy, cap in settings:
                d_load.zero_()
                pk.pick_bounded_device(d_reqs.data_ptr(), R, None, k, None, cap, policy, d_load.data_ptr(), d_pick.data_ptr(), d_score.data_ptr(),
                                       d_rank.data_ptr(), s)
                assert pk.launch_status() == 0
                got = (d_pick.cpu().numpy(), d_score.cpu().numpy(), d_rank.cpu().numpy(), d_load.cpu().numpy().view(np.uint32))
                want = ref.resolve(lists, totals, P, None, cap, policy, np.zeros(P, dtype=np.uint32))
                for a, b, what in zip(got, want[:4], ("picks", "scores", "ranks", "loads")):
                    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name}: {what} differ from tests/bounded_ref.py"
                rank = got[2]
                out["settings"][name] = {
                    "cap_all": cap, "busiest_pod": int(got[3].max()), "checked_against_bounded_ref": True,
                    "share_by_rank": [round(float(np.mean(rank == j)), 5) for j in range(k)],
                    "share_overflow": round(float(np.mean((rank & ref.RANK_OVERFLOW) != 0)), 5),
                    "share_no_candidate": round(float(np.mean(rank == ref.RANK_NONE)), 5),
                    "bounded_over_topk": round(out["bounded_" + name]["us_median"] / out[f"topk{k}"]["us_median"], 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
