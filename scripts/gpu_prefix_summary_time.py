"""The prefix-hit summary and the hybrid pick (SEMANTICS.md §3m) at full size: C5's 64k requests x 4096 pods x 32 blocks and its index.

Times, in one process and alternating, with HIP events after a warm-up: eppk_prefix_summary_device unmasked and under 50 % masks;
eppk_pick_hybrid_device at k = 4 with about 0 %, 50 % and 100 % cold rows (min_hit 1 on the workload's rows; the same on rows of which every
second one misses its first block; min_hit above every row's best); next to them the yardsticks eppk_pick_topk_device (k = 4),
eppk_prefix_costs_device (k = 8) and eppk_pick_rendezvous_scored_device (k = 4).  Then how walk, best, holders and the warm share
distribute on the headline index and on a cold one (--cold-groups uniform prefix groups).  Prints one JSON line.  Kernel times: run it once
more under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402
from gpu_prefix_costs_time import timed  # noqa: E402


def distribution(s, n_blocks):
    """Of an [R, 4] summary: value -> share of the rows, for walk, best and holders (the eight most common), and the hit ratio."""
    out = {}
    for col, name in enumerate(("walk", "best", "holders")):
        v, c = np.unique(s[:, col], return_counts=True)
        top = np.argsort(-c)[:8]
        out[name] = {int(v[i]): round(float(c[i]) / len(s), 4) for i in top}
    out["warm_share_min_hit_1"] = float(np.mean(s[:, 1] >= 1))
    out["prefix_hit_ratio"] = float(s[:, 1].sum() / max(1, int(n_blocks.sum())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed calls per leg and round")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of the alternating legs")
    ap.add_argument("--config", type=int, default=5, help="workload configuration (5 = the headline batch)")
    ap.add_argument("--cold-groups", type=int, default=65536, help="uniform prefix groups of the cold-index workload (0: skip it)")
    args = ap.parse_args()
    import torch
    pkg = g.load_package()
    wl = pkg.workload.make_workload(args.config)
    R, P = wl.reqs.shape[0], wl.pods.shape[0]
    J, k = (P + 63) // 64, 4
    rng = np.random.default_rng(23)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    s = st.cuda_stream
    half_cold = wl.reqs.copy()
    half_cold[1::2, 1] ^= np.uint64(1)                                         # every second row misses its first block: best = 0
    d_reqs = torch.from_numpy(wl.reqs.view(np.int64)).cuda()
    d_reqs_half = torch.from_numpy(half_cold.view(np.int64)).cuda()
    d_half = torch.from_numpy(rng.integers(0, 2 ** 64, (R, J), dtype=np.uint64).view(np.int64)).cuda()      # 50 % masks
    d_sum = torch.empty(R * 4, dtype=torch.int32, device="cuda")
    d_lists, d_ls = torch.empty(R * 8, dtype=torch.int32, device="cuda"), torch.empty(R * 8, dtype=torch.float64, device="cuda")
    d_l8 = torch.empty(R * 8, dtype=torch.int32, device="cuda")
    d_u32 = [torch.empty(R * 8, dtype=torch.int32, device="cuda") for _ in range(2)]
    d_route = torch.empty(R, dtype=torch.uint8, device="cuda")
    out = {}
    with pkg.BatchedPicker(wl.chain, max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots) as pk:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)

        def topk(kk, dst):
            def f():
                rc = pk._lib.eppk_pick_topk_device(pk._ctx, d_reqs.data_ptr(), R, None, kk, dst.data_ptr(), d_ls.data_ptr(), s)
                assert rc == 0, rc
            return f

        topk(8, d_l8)()                                                        # the lists eppk_prefix_costs_device answers for

        def hybrid(rows, min_hit):
            return lambda: pk.pick_hybrid_device(rows.data_ptr(), R, k, 3, min_hit, d_lists.data_ptr(), d_ls.data_ptr(), d_route.data_ptr(), depth=2, stream=s)

        legs = {"summary": lambda: pk.prefix_summary_device(d_reqs.data_ptr(), R, d_sum.data_ptr(), None, s),
                "summary_masked50": lambda: pk.prefix_summary_device(d_reqs.data_ptr(), R, d_sum.data_ptr(), d_half.data_ptr(), s),
                "summary_half_miss": lambda: pk.prefix_summary_device(d_reqs_half.data_ptr(), R, d_sum.data_ptr(), None, s),
                "topk4": topk(k, d_lists),
                "prefix_costs_k8": lambda: pk.prefix_costs_device(d_reqs.data_ptr(), R, d_l8.data_ptr(), 8, None, 1, d_u32[0].data_ptr(), d_u32[1].data_ptr(), s),
                "rendezvous_scored_k4": lambda: pk.pick_rendezvous_scored_device(d_reqs.data_ptr(), R, k, 3, 0, d_lists.data_ptr(), d_ls.data_ptr(), depth=2, stream=s),
                "hybrid_k4_cold0": hybrid(d_reqs, 1), "hybrid_k4_cold50": hybrid(d_reqs_half, 1), "hybrid_k4_cold100": hybrid(d_reqs, wl.B + 1)}
        out = timed(torch, st, legs, args.reps, args.rounds)
        out["hybrid_parts_sum_us"] = out["summary"]["us_median"] + out["topk4"]["us_median"] + out["rendezvous_scored_k4"]["us_median"]
        for name, cold in (("hybrid_k4_cold0", 0.0), ("hybrid_k4_cold50", 0.5), ("hybrid_k4_cold100", 1.0)):
            legs[name]()
            st.synchronize()
            assert abs(1.0 - float(d_route.float().mean()) - cold) < 0.01, name
        legs["summary"]()
        out["geometry"] = list(pk.launch_geometry())
        st.synchronize()
        nb = (wl.reqs[:, 0] >> np.uint64(32)).astype(np.int64)
        out["headline_index"] = distribution(d_sum.cpu().numpy().view(np.uint32).reshape(R, 4), nb)
        assert pk.launch_status() == 0
    if args.cold_groups:
        cw = pkg.workload.make_workload(args.config, n_groups=args.cold_groups, zipf_s=0.0)
        d_creqs = torch.from_numpy(cw.reqs.view(np.int64)).cuda()
        with pkg.BatchedPicker(cw.chain, max_pods=P, max_blocks=cw.B, max_batch=R, index_slots=cw.index_slots) as pk:
            pk.publish(cw.pods)
            pk.index_insert(cw.index_hashes, cw.index_pods)
            cold = timed(torch, st, {"summary_cold_index": lambda: pk.prefix_summary_device(d_creqs.data_ptr(), R, d_sum.data_ptr(), None, s)}, args.reps, args.rounds)
            st.synchronize()
            out.update(cold)
            out["cold_index"] = distribution(d_sum.cpu().numpy().view(np.uint32).reshape(R, 4), (cw.reqs[:, 0] >> np.uint64(32)).astype(np.int64))
            assert pk.launch_status() == 0
    print(json.dumps({f"{R} x {P}": out}))


if __name__ == "__main__":
    main()
