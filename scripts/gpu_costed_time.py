"""Cost-weighted caps for the bounded and banded pickers (SEMANTICS.md §3f) at full size: C5 (64k requests x 4096 pods, full chain +
prefix index), k = 4, SHED.

Times the resolve alone over the lists eppk_pick_topk_device delivers -- HIP events on the launch stream after a warm-up, `--rounds`
rounds of `--reps` calls each, the legs alternating in one process, median / min / max over the rounds:
  plain, banded_1, banded_3       eppk_bounded_resolve_device and eppk_banded_resolve_device (1 and 3 bands), cap_all = 64 requests
  costed_unit_1, costed_unit_3    eppk_costed_resolve_device with every cost 1: the price of the cost machinery over the banded resolve
  costed_tail_1, costed_tail_3    ... with a seeded heavy-tailed cost per request in 1 .. 8192 and cap_all = 64 x the mean cost
The last batch of every leg is checked against the restatements under tests/: a timing of wrong picks is worth nothing.  Then the number
the feature exists for: on the heavy-tailed batch, the heaviest pod's load IN COST UNITS under the count cap of 64 requests and under
the cost cap, against the cap.  One JSON line.

`--existing-only` times plain, banded_1 and banded_3 alone and touches nothing newer; with `--root DIR` the package is loaded from
another checkout (built there): the PARENT commit's figures in the same session, which this commit's existing legs must agree with."""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="timed calls per leg and round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds of the alternating legs")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--cap", type=int, default=64, help="the count cap; the cost cap is this many mean costs")
    ap.add_argument("--existing-only", action="store_true")
    ap.add_argument("--root", default=HERE, help="the checkout whose package is timed")
    args = ap.parse_args()
    import torch
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    g = _load(os.path.join(root, "__graft_entry__.py"), "__graft_entry__")
    pkg = g.load_package()
    wl = pkg.workload.make_workload(5)
    R, P, k, cap = wl.reqs.shape[0], wl.pods.shape[0], args.k, args.cap
    rng = np.random.default_rng(0xC057)
    band3 = rng.integers(0, 3, size=R).astype(np.uint8)
    tail = np.clip(np.floor((rng.pareto(1.1, size=R) + 1.0) * 4.0), 1, 8192).astype(np.uint32)
    cost_cap = cap * int(round(float(tail.mean())))
    with pkg.BatchedPicker(wl.chain, max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots) as pk:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
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
        d_band3 = torch.from_numpy(band3).cuda()
        d_unit = torch.ones(R, dtype=torch.int32, device="cuda")
        d_tail = torch.from_numpy(tail.view(np.int32)).cuda()
        assert pk._lib.eppk_pick_topk_device(pk._ctx, d_reqs.data_ptr(), R, None, k, d_lists.data_ptr(), d_ls.data_ptr(), s) == 0
        torch.cuda.synchronize()
        out_ptrs = (d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr(), s)
        tables = {1: [(0, 0)], 3: [(0, 0)] * 3}
        bands = {1: (None, None), 3: (band3, d_band3.data_ptr())}

        def plain(load=None):
            pk.bounded_resolve_device(d_lists.data_ptr(), d_ls.data_ptr(), R, k, None, cap, 0, load, *out_ptrs)
        legs = {"plain": plain}
        for nb in (1, 3):
            legs[f"banded_{nb}"] = (lambda load=None, nb=nb: pk.bounded_resolve_banded_device(
                d_lists.data_ptr(), d_ls.data_ptr(), R, k, bands[nb][1], tables[nb], None, cap, load, *out_ptrs))
        costed = {}
        if not args.existing_only:
            for name, d_cost, cost, c_all in (("unit", d_unit, np.ones(R, dtype=np.uint32), cap), ("tail", d_tail, tail, cost_cap)):
                for nb in (1, 3):
                    costed[f"costed_{name}_{nb}"] = (cost, nb, c_all)
                    legs[f"costed_{name}_{nb}"] = (lambda load=None, nb=nb, d_cost=d_cost, c_all=c_all: pk.bounded_resolve_costed_device(
                        d_lists.data_ptr(), d_ls.data_ptr(), R, k, d_cost.data_ptr(), 0, bands[nb][1], tables[nb], None, c_all, load, *out_ptrs))
        for f in legs.values():                 # warm-up: code objects, scratch
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
        out["shape"], out["k"], out["cap_all"], out["reps"], out["rounds"], out["root"] = f"{R} x {P}", k, cap, args.reps, args.rounds, os.path.basename(root)
        out["geometry"] = dict(zip(("chunk", "one_launch_max"), pk.bounded_geometry()))
        lists, totals = d_lists.cpu().numpy(), d_ls.cpu().numpy()

        def outputs(f):
            d_load.zero_()
            f(d_load.data_ptr())
            assert pk.launch_status() == 0
            return d_pick.cpu().numpy(), d_score.cpu().numpy(), d_rank.cpu().numpy(), d_load.cpu().numpy().view(np.uint32)

        def same(got, want, name):
            for a, b, what in zip(got, want[:4], ("picks", "scores", "ranks", "loads")):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name}: {what} differ from the restatement"

        tests = os.path.join(HERE, "tests")
        zeros = np.zeros(P, dtype=np.uint32)
        got = {}
        banded_ref = _load(os.path.join(tests, "banded_ref.py"), "banded_ref")
        got["plain"] = outputs(plain)
        same(got["plain"], banded_ref.ref.resolve(lists, totals, P, None, cap, 0, zeros), "plain")
        for nb in (1, 3):
            got[f"banded_{nb}"] = outputs(legs[f"banded_{nb}"])
            same(got[f"banded_{nb}"], banded_ref.resolve(lists, totals, P, tables[nb], bands[nb][0], None, cap, zeros), f"banded_{nb}")
        if costed:
            ref = _load(os.path.join(tests, "costed_ref.py"), "costed_ref")
            for name, (cost, nb, c_all) in costed.items():
                got[name] = outputs(legs[name])
                same(got[name], ref.resolve(lists, totals, P, cost, tables[nb], bands[nb][0], None, c_all, zeros), name)
            # what the feature is for: the heaviest pod in COST units, under the count cap and under the cost cap
            out["mean_cost"], out["max_cost"], out["cost_cap"] = float(tail.mean()), int(tail.max()), cost_cap
            heaviest = {}
            for name in ("banded_1", "banded_3", "costed_tail_1", "costed_tail_3"):
                pick = got[name][0]
                units = np.zeros(P, dtype=np.int64)
                np.add.at(units, pick[pick >= 0], tail[pick >= 0].astype(np.int64))
                heaviest[name] = {"heaviest_pod_cost_units": int(units.max()), "over_cost_cap": float(units.max()) / cost_cap,
                                  "pods_over_cost_cap": int(np.sum(units > cost_cap)), "shed": int(np.sum(pick < 0)),
                                  "placed_cost_units": int(units.sum())}
            out["heaviest_pod"] = heaviest
        for name in got:
            out[name]["checked_against_restatement"] = True
    print(json.dumps(out))


if __name__ == "__main__":
    main()
