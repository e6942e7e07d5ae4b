"""The index read-out (SEMANTICS.md §6d) at full size, next to the two full-table scans the library already has.

Two indexes: the headline workload's (C5: 256 prefix groups) and the cold-index workload's (262 144 groups, uniform: 4.2 M hashes on four
pods each, 16.8 M API slots).  In one process and alternating, after a warm-up: eppk_index_export_device with room for every triple and
as the count query (HIP events on the call's stream), then -- host clock around synchronous calls -- eppk_index_trim_pods with a cap
that removes nothing (index_pod_hist_kernel + the cut + the trim walk), eppk_index_selfcheck, the host form of the export end to end, and
ONE eppk_index_import of the exported triples into a fresh context of the same size.  Prints one JSON line per index.  Kernel times
(index_pod_hist_kernel alone, the export's passes one by one): run it once more under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402
from gpu_prefix_costs_time import timed  # noqa: E402


def host_timed(legs, reps, rounds):
    times = {n: [] for n in legs}
    for _ in range(rounds):
        for n, f in legs.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            times[n].append((time.perf_counter() - t0) * 1e6 / reps)
    return {n: {"us_median": float(np.median(v)), "us_min": float(np.min(v)), "us_max": float(np.max(v))} for n, v in times.items()}


def measure(pkg, torch, st, wl, reps, rounds):
    s = st.cuda_stream
    mk = lambda: pkg.BatchedPicker(wl.chain, max_pods=wl.P, max_blocks=wl.B, max_batch=64, index_slots=wl.index_slots)      # noqa: E731
    with mk() as pk:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        h, p, a = pk.index_export()
        n = int(h.shape[0])
        d_h, d_p = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        d_a, d_n = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")

        def export(cap):
            def f():
                rc = pk._lib.eppk_index_export_device(pk._ctx, d_h.data_ptr() if cap else None, d_p.data_ptr() if cap else None,
                                                      d_a.data_ptr() if cap else None, cap, d_n.data_ptr(), s)
                assert rc == 0, rc
            return f

        out = {"triples": n, "hashes": pk.index_size(), "index_slots": wl.index_slots}
        out["device"] = timed(torch, st, {"export_device": export(n), "export_device_count_query": export(0)}, reps, rounds)
        st.synchronize()
        assert int(d_n.item()) == n and pk.launch_status() == 0
        assert np.array_equal(d_h.cpu().numpy().view(np.uint64), h) and np.array_equal(d_p.cpu().numpy().view(np.uint32), p)
        host = {"trim_pods_removing_nothing": lambda: pk.index_trim_pods(0xFFFFFFFF), "selfcheck": pk.index_selfcheck, "export_host": pk.index_export}
        for f in host.values():
            f()
        out["host_clock"] = host_timed(host, max(1, reps // 4), rounds)
        us = out["device"]["export_device"]["us_median"]
        # what one call moves at least: the key words and list lines of both walks, the triples out
        rows = 2 * wl.index_slots + 2
        out["export_gb_per_s"] = (2 * (rows * 8 + pk.index_size() * 64) + n * 13) / us / 1e3
    with mk() as pk2:
        pk2.publish(wl.pods)
        t0 = time.perf_counter()
        pk2.index_import(h, p, a)
        out["import_us"] = (time.perf_counter() - t0) * 1e6
        assert pk2.index_size() == out["hashes"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed calls per leg and round")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of the alternating legs")
    ap.add_argument("--config", type=int, default=5, help="workload configuration (5 = the headline batch)")
    ap.add_argument("--cold-groups", type=int, default=262144, help="prefix groups of the cold index (0: skip it)")
    args = ap.parse_args()
    import torch
    pkg = g.load_package()
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    wl = pkg.workload.make_workload(args.config, R=64)
    print(json.dumps({"headline index": measure(pkg, torch, st, wl, args.reps, args.rounds)}), flush=True)
    if args.cold_groups:
        wl = pkg.workload.make_workload(args.config, R=64, n_groups=args.cold_groups, zipf_s=0.0, pods_per_group=4)
        print(json.dumps({"cold index": measure(pkg, torch, st, wl, args.reps, args.rounds)}), flush=True)


if __name__ == "__main__":
    main()
