"""Picker "weighted-random" (SEMANTICS.md §3c) at full size: C5 (64k requests x 4096 pods, full chain + prefix index).

Times eppk_pick_weighted_random_device (unmasked k = 1 and k = 4, 50 % masks with k = 1) and, in the same process and alternating
with them, eppk_pick_topk_device(k = 4) on the same rows, with HIP events after a warm-up; prints the herding figure (the most
requests any one pod receives under best-score and under weighted-random) and one JSON line.  Kernel times: run it once more under
`rocprofv3 --kernel-trace --stats` (pick_wrand_kernel against the top-4 route's kernels)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed calls per leg and round")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of the alternating legs")
    args = ap.parse_args()
    import torch
    pkg = g.load_package()
    wl = pkg.workload.make_workload(5)
    R, P = wl.reqs.shape[0], wl.pods.shape[0]
    J = (P + 63) // 64
    rng = np.random.default_rng(5)
    bits = rng.random((R, J * 64)) < 0.5
    mask = np.packbits(bits.reshape(R, J, 64)[:, :, ::-1], axis=2).view(">u8").reshape(R, J).astype(np.uint64)
    with pkg.BatchedPicker(wl.chain, max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots) as pk:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        lib = pk._lib
        st = torch.cuda.Stream()
        torch.cuda.set_stream(st)
        s = st.cuda_stream
        d_reqs = torch.from_numpy(wl.reqs.view(np.int64)).cuda()
        d_mask = torch.from_numpy(mask.view(np.int64)).cuda()
        d_pick = torch.empty(R * 8, dtype=torch.int32, device="cuda")
        d_score = torch.empty(R * 8, dtype=torch.float64, device="cuda")

        def wrand(k, m):
            return lambda: pk.pick_weighted_random_device(d_reqs.data_ptr(), R, d_mask.data_ptr() if m else None, k, 7, d_pick.data_ptr(),
                                                          d_score.data_ptr(), s)

        def topk4():
            rc = lib.eppk_pick_topk_device(pk._ctx, d_reqs.data_ptr(), R, None, 4, d_pick.data_ptr(), d_score.data_ptr(), s)
            assert rc == 0, rc
        legs = {"wrand_k1": wrand(1, False), "wrand_k4": wrand(4, False), "wrand_masked50_k1": wrand(1, True), "topk4": topk4}
        for f in legs.values():                 # warm-up: code objects, occupancy queries, buffers
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
        bp, _ = pk.pick(wl.reqs)
        wp, _ = pk.pick_weighted_random(wl.reqs, 7, 1)
    out = {n: {"us_median": float(np.median(v)), "us_min": float(np.min(v)), "us_max": float(np.max(v))} for n, v in times.items()}
    out["wrand_k1_over_topk4"] = out["wrand_k1"]["us_median"] / out["topk4"]["us_median"]
    out["herding_max_requests_per_pod"] = {"best_score": int(np.bincount(bp[bp >= 0], minlength=P).max()),
                                           "weighted_random": int(np.bincount(wp[:, 0][wp[:, 0] >= 0], minlength=P).max())}
    out["shape"] = f"{R} x {P}"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
