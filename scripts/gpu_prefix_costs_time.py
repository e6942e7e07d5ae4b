"""Costs per list entry from the prefix index (SEMANTICS.md §3k) at full size: C5's 64k requests x 4096 pods and its index.

Times, in one process and alternating, with HIP events after a warm-up: eppk_pick_topk_device (k = 4, 8: the call the kernel follows),
eppk_prefix_costs_device alone over those lists (k = 4, 8), and eppk_pick_costed_device against eppk_pick_cost_cached_device (k = 4,
one SHED band).  Then one figure of what the call is for: base = prompt blocks + a heavy-tailed decode reserve (DESIGN.md §3.13's
distribution), caps in blocks; how many requests each form places, and the heaviest pod's load in TRUE (uncached) blocks under each.
Prints one JSON line.  Kernel times: run it once more under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def timed(torch, st, legs, reps, rounds):
    for f in legs.values():                 # warm-up: code objects, occupancy queries, buffers
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {n: [] for n in legs}
    for _ in range(rounds):
        for n, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(reps):
                f()
            e1.record(st)
            e1.synchronize()
            times[n].append(e0.elapsed_time(e1) * 1e3 / reps)
    return {n: {"us_median": float(np.median(v)), "us_min": float(np.min(v)), "us_max": float(np.max(v))} for n, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed calls per leg and round")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of the alternating legs")
    ap.add_argument("--config", type=int, default=5, help="workload configuration (5 = the headline batch)")
    args = ap.parse_args()
    import torch
    pkg = g.load_package()
    wl = pkg.workload.make_workload(args.config)
    R, P = wl.reqs.shape[0], wl.pods.shape[0]
    rng = np.random.default_rng(13)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    s = st.cuda_stream
    nb = (wl.reqs[:, 0] >> np.uint64(32)).astype(np.int64)
    base = np.clip(nb + np.clip(np.floor((rng.pareto(1.1, R) + 1.0) * 4.0), 1, 8192).astype(np.int64), 1, 0x00FFFFFF).astype(np.uint32)
    cap = 64 * int(round(float(base.mean())))
    shed = ((0, 0),)                        # one band, EPPK_BOUNDED_SHED
    d_reqs = torch.from_numpy(wl.reqs.view(np.int64)).cuda()
    d_base = torch.from_numpy(base.view(np.int32)).cuda()
    d_lists = {k: torch.empty(R * k, dtype=torch.int32, device="cuda") for k in (4, 8)}
    d_ls = torch.empty(R * 8, dtype=torch.float64, device="cuda")
    d_cost = torch.empty(R * 8, dtype=torch.int32, device="cuda")
    d_matched = torch.empty(R * 8, dtype=torch.int32, device="cuda")
    d_pick = torch.empty(R, dtype=torch.int32, device="cuda")
    d_score = torch.empty(R, dtype=torch.float64, device="cuda")
    d_rank = {n: torch.empty(R, dtype=torch.uint8, device="cuda") for n in ("whole", "cached")}
    with pkg.BatchedPicker(wl.chain, max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots) as pk:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)

        def topk(k):
            def f():
                rc = pk._lib.eppk_pick_topk_device(pk._ctx, d_reqs.data_ptr(), R, None, k, d_lists[k].data_ptr(), d_ls.data_ptr(), s)
                assert rc == 0, rc
            return f

        def costs(k):
            return lambda: pk.prefix_costs_device(d_reqs.data_ptr(), R, d_lists[k].data_ptr(), k, d_base.data_ptr(), 1, d_cost.data_ptr(),
                                                  d_matched.data_ptr(), s)

        def whole():
            pk.pick_bounded_costed_device(d_reqs.data_ptr(), R, None, 4, d_base.data_ptr(), None, shed, None, cap, None, d_pick.data_ptr(),
                                          d_score.data_ptr(), d_rank["whole"].data_ptr(), s)

        def cached():
            pk.pick_costed_cached_device(d_reqs.data_ptr(), R, None, 4, d_base.data_ptr(), 1, None, shed, None, cap, None, d_pick.data_ptr(),
                                         d_score.data_ptr(), d_rank["cached"].data_ptr(), s)

        legs = {"topk4": topk(4), "prefix_costs_k4": costs(4), "topk8": topk(8), "prefix_costs_k8": costs(8),
                "pick_costed_k4": whole, "pick_costed_cached_k4": cached}
        out = timed(torch, st, legs, args.reps, args.rounds)
        legs["prefix_costs_k4"]()
        out["geometry"] = list(pk.launch_geometry())
        # what it is for: the same lists under both forms; a request placed at rank j truly brings cost[r][j] = base - matched blocks
        legs["topk4"](), legs["prefix_costs_k4"](), whole(), cached()
        st.synchronize()
        assert pk.launch_status() == 0
    lists = d_lists[4].cpu().numpy().reshape(R, 4)
    cost = d_cost.cpu().numpy().view(np.uint32)[:R * 4].reshape(R, 4).astype(np.int64)
    matched = d_matched.cpu().numpy().view(np.uint32)[:R * 4].reshape(R, 4)
    fig = {"cap_all": cap, "base_mean": float(base.mean()), "prompt_blocks_mean": float(nb.mean()),
           "matched_mean_entry0": float(matched[:, 0].mean()), "matched_over_prompt_entry0": float(matched[:, 0].sum() / max(1, nb.sum()))}
    for n, t in d_rank.items():
        rank = t.cpu().numpy()
        placed = rank < 4
        rows = np.nonzero(placed)[0]
        true_load = np.bincount(lists[rows, rank[rows]], weights=cost[rows, rank[rows]], minlength=P)
        fig[n] = {"placed": int(placed.sum()), "shed": int(R - placed.sum()), "heaviest_pod_true_blocks": int(true_load.max()),
                  "true_blocks_placed": int(true_load.sum())}
    out["figure"] = fig
    out["prefix_costs_k4_over_topk4"] = out["prefix_costs_k4"]["us_median"] / out["topk4"]["us_median"]
    out["cached_minus_whole_us"] = out["pick_costed_cached_k4"]["us_median"] - out["pick_costed_k4"]["us_median"]
    print(json.dumps({f"{R} x {P}": out}))


if __name__ == "__main__":
    main()
