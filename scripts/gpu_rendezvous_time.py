"""Picker "rendezvous" (SEMANTICS.md §3j) at full size: C5's 64k requests x 4096 pods, and 64k requests x 64 pods.

Times eppk_pick_rendezvous_device -- session form and prefix form, unmasked and under 50 % masks, k = 1, 4, 8 -- and, in the same
process and alternating with them, eppk_pick_topk_device(k = 4) and eppk_pick_weighted_random_device(k = 4) on the same rows, with
HIP events after a warm-up; prints one JSON line.  Kernel times: run it once more under `rocprofv3 --kernel-trace --stats`."""
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
    args = ap.parse_args()
    import torch
    pkg = g.load_package()
    wl = pkg.workload.make_workload(5)
    R = wl.reqs.shape[0]
    rng = np.random.default_rng(5)
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    s = st.cuda_stream
    d_reqs = torch.from_numpy(wl.reqs.view(np.int64)).cuda()
    d_key = torch.from_numpy(rng.integers(0, 2 ** 63, R, dtype=np.int64)).cuda()
    d_pick = torch.empty(R * 8, dtype=torch.int32, device="cuda")
    d_score = torch.empty(R * 8, dtype=torch.float64, device="cuda")
    out = {}
    for P in (wl.pods.shape[0], 64):
        J = (P + 63) // 64
        bits = rng.random((R, J * 64)) < 0.5
        mask = np.packbits(bits.reshape(R, J, 64)[:, :, ::-1], axis=2).view(">u8").reshape(R, J).astype(np.uint64)
        d_mask = torch.from_numpy(mask.view(np.int64)).cuda()
        d_pod = torch.from_numpy(rng.integers(0, 2 ** 63, P, dtype=np.int64)).cuda()
        with pkg.BatchedPicker(wl.chain, max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots) as pk:
            pk.publish(wl.pods[:P])
            if P == wl.pods.shape[0]:       # (the baselines of the 64-pod snapshot see an empty index)
                pk.index_insert(wl.index_hashes, wl.index_pods)

            def rdv(k, m, prefix):
                return lambda: pk.pick_rendezvous_device(d_reqs.data_ptr() if prefix else None, R, k, 7, d_pick.data_ptr(), d_score.data_ptr(),
                                                         None if prefix else d_key.data_ptr(), 4 if prefix else 0, d_pod.data_ptr(),
                                                         d_mask.data_ptr() if m else None, s)

            def topk4():
                rc = pk._lib.eppk_pick_topk_device(pk._ctx, d_reqs.data_ptr(), R, None, 4, d_pick.data_ptr(), d_score.data_ptr(), s)
                assert rc == 0, rc

            legs = {f"{'prefix' if pf else 'session'}{'_masked50' if m else ''}_k{k}": rdv(k, m, pf)
                    for pf in (False, True) for m in (False, True) for k in (1, 4, 8)}
            legs["topk4"] = topk4
            legs["wrand_k4"] = lambda: pk.pick_weighted_random_device(d_reqs.data_ptr(), R, None, 4, 7, d_pick.data_ptr(), d_score.data_ptr(), s)
            t = timed(torch, st, legs, args.reps, args.rounds)
            legs["session_k4"]()
            t["geometry"] = list(pk.launch_geometry())
        t["session_k4_over_wrand_k4"] = t["session_k4"]["us_median"] / t["wrand_k4"]["us_median"]
        t["rounds_1_to_3_over_round_0"] = (t["session_k4"]["us_median"] - t["session_k1"]["us_median"]) / t["session_k1"]["us_median"]
        out[f"{R} x {P}"] = t
    print(json.dumps(out))


if __name__ == "__main__":
    main()
