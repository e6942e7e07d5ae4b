"""Chain totals of listed pods (SEMANTICS.md §3l) at full size: C5's 64k requests x 4096 pods x 32 blocks and its index.

Times, in one process and alternating, with HIP events after a warm-up: eppk_score_lists_device (EPPK_SCORE_SORT) for k = 4 / 8, with the
workload's chain and with its PREFIX scorer taken out, unmasked and under 50 % masks, default and EPPK_SCORE_WITHIN_LIST; next to them
eppk_prefix_costs_device at the same k, the top-4 pick, eppk_pick_rendezvous_device, and the detour the call replaces: masked
eppk_pick_topk_device over mask rows that hold exactly the eight listed pods.  Then the pick form with the SPILL resolve behind it
against rendezvous + SPILL resolve alone.  Prints one JSON line.  Kernel times: run it once more under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402
from gpu_prefix_costs_time import timed  # noqa: E402

SORT, WITHIN, SPILL = 1, 2, 1


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
    J = (P + 63) // 64
    rng = np.random.default_rng(17)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    s = st.cuda_stream
    half = rng.integers(0, 2 ** 64, (R, J), dtype=np.uint64)                  # 50 % masks
    d_reqs = torch.from_numpy(wl.reqs.view(np.int64)).cuda()
    d_half = torch.from_numpy(half.view(np.int64)).cuda()
    d_key = torch.from_numpy(rng.integers(0, 2 ** 64, R, dtype=np.uint64).view(np.int64)).cuda()
    d_lists = {(k, m): torch.empty(R * k, dtype=torch.int32, device="cuda") for k in (4, 8) for m in (False, True)}
    d_out = torch.empty(R * 8, dtype=torch.int32, device="cuda")
    d_ls = torch.empty(R * 8, dtype=torch.float64, device="cuda")
    d_u32 = [torch.empty(R * 8, dtype=torch.int32, device="cuda") for _ in range(2)]
    d_pick, d_score = torch.empty(R, dtype=torch.int32, device="cuda"), torch.empty(R, dtype=torch.float64, device="cuda")
    d_rank, d_load = torch.empty(R, dtype=torch.uint8, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")
    cap = int(1.25 * R / P) + 1
    no_prefix = [(kind, w) for kind, w in wl.chain if int(kind) != 4]
    mk = lambda chain: pkg.BatchedPicker(chain, max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots)      # noqa: E731
    with mk(wl.chain) as pk, mk(no_prefix) as pk0:
        for p in (pk, pk0):
            p.publish(wl.pods)
            p.index_insert(wl.index_hashes, wl.index_pods)

        def topk(k, mask=None, out=None):
            def f():
                rc = pk._lib.eppk_pick_topk_device(pk._ctx, d_reqs.data_ptr(), R, mask, k, (d_out if out is None else out).data_ptr(), d_ls.data_ptr(), s)
                assert rc == 0, rc
            return f

        for (k, m), t in d_lists.items():                                      # the lists to score: the ordered fallbacks, unmasked and masked
            topk(k, d_half.data_ptr() if m else None, t)()
        st.synchronize()
        listed = np.zeros((R, J), dtype=np.uint64)                             # the detour's mask rows: exactly the eight listed pods
        l8 = d_lists[8, False].cpu().numpy().reshape(R, 8).astype(np.int64)
        rows = np.repeat(np.arange(R), 8)[l8.ravel() >= 0]
        pods = l8.ravel()[l8.ravel() >= 0]
        np.bitwise_or.at(listed, (rows, pods >> 6), np.uint64(1) << (pods & 63).astype(np.uint64))
        d_listed = torch.from_numpy(listed.view(np.int64)).cuda()

        def score(p, k, flags, m):
            return lambda: p.score_lists_device(d_reqs.data_ptr(), R, d_lists[k, m].data_ptr(), k, flags | SORT, d_out.data_ptr(), d_ls.data_ptr(),
                                                d_half.data_ptr() if m else None, s)

        def costs(k):
            return lambda: pk.prefix_costs_device(d_reqs.data_ptr(), R, d_lists[k, False].data_ptr(), k, None, 1, d_u32[0].data_ptr(), d_u32[1].data_ptr(), s)

        def rendezvous(k):
            return lambda: pk.pick_rendezvous_device(None, R, k, 3, d_out.data_ptr(), d_ls.data_ptr(), d_key=d_key.data_ptr(), stream=s)

        def resolve():
            d_load.zero_()
            pk.bounded_resolve_device(d_out.data_ptr(), d_ls.data_ptr(), R, 8, None, cap, SPILL, d_load.data_ptr(), d_pick.data_ptr(), d_score.data_ptr(),
                                      d_rank.data_ptr(), s)

        def plain_spill():
            rendezvous(8)()
            resolve()

        def scored_spill():
            pk.pick_rendezvous_scored_device(d_reqs.data_ptr(), R, 8, 3, 0, d_out.data_ptr(), d_ls.data_ptr(), d_key=d_key.data_ptr(), stream=s)
            resolve()

        legs = {"topk4": topk(4), "rendezvous_k4": rendezvous(4), "rendezvous_k8": rendezvous(8),
                "detour_masked_topk4_of_8_listed": topk(4, d_listed.data_ptr())}
        for k in (4, 8):
            legs[f"prefix_costs_k{k}"] = costs(k)
            for name, p in (("prefix", pk), ("no_prefix", pk0)):
                for m in (False, True):
                    for fl in (0, WITHIN):
                        legs[f"score_lists_k{k}_{name}{'_masked50' if m else ''}{'_within' if fl else ''}"] = score(p, k, fl, m)
        legs["rendezvous_k8_spill"], legs["rendezvous_scored_k8_spill"] = plain_spill, scored_spill
        out = timed(torch, st, legs, args.reps, args.rounds)
        legs["score_lists_k8_prefix"]()
        out["geometry_prefix"] = list(pk.launch_geometry())
        legs["score_lists_k8_no_prefix"]()
        out["geometry_no_prefix"] = list(pk0.launch_geometry())
        st.synchronize()
        assert pk.launch_status() == 0 and pk0.launch_status() == 0
    print(json.dumps({f"{R} x {P}": out}))


if __name__ == "__main__":
    main()
