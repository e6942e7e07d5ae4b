"""Fair shares between flows (SEMANTICS.md §3g) at full size: C5 (64k requests x 4096 pods, full chain + prefix index), k = 4, SHED.

Times the resolve alone over the lists eppk_pick_topk_device delivers -- HIP events on the launch stream after a warm-up, `--rounds`
rounds of `--reps` calls each, the legs alternating in one process, median / min / max over the rounds:
  banded_1, banded_3, costed_unit_*, costed_tail_*   the resolves this one is built on (eppk_banded_resolve_device,
                                                    eppk_costed_resolve_device), cap_all = `--cap` requests / that many mean costs
  fair_{unit,tail}_f{1,16,256,1024}_b{1,3}          eppk_fair_resolve_device: no cost array / the heavy-tailed costs of §3.13; the flows
                                                    drawn heavy-tailed (one flow holds about a third of the batch); one band / three
  order_fair_f*_b*, order_band_b*                   the order alone: the same calls on a context WITHOUT pods (the rounds are skipped):
                                                    the memsets, the three order launches and the finish launch -- the fair order
                                                    against the band order of the costed resolve
  small_{64,512}_{costed,fair}                      a batch of 64 and of 512 requests: the one-launch costed call against the fair call,
                                                    which always takes the permutation route
The last batch of every fair and costed leg is checked against the restatements under tests/: a timing of wrong picks is worth nothing.
Then the numbers the feature exists for: the busiest flow's share of the placed requests and the flows that get nothing, under the
costed resolve and under the fair one.  One JSON line.

`--existing-only` times the banded and costed legs alone and touches nothing newer; with `--root DIR` the package is loaded from another
checkout (built there): the PARENT commit's figures in the same session, which this commit's existing legs must agree with.

The order_* legs are a DIFFERENCE (fair order against band order, each with its memsets and its finish), not the time of the three
launches.  Times per kernel take a run of their own under `rocprofv3 --kernel-trace --stats` with `--rounds 1 --reps 20`, as
scripts/gpu_costed_time.py is profiled; no such figures are recorded yet."""
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
    ap.add_argument("--reps", type=int, default=50, help="timed calls per leg and round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds of the alternating legs")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--cap", type=int, default=8, help="the count cap (8 x 4096 pods: room for half the batch); the cost cap is this many mean costs")
    ap.add_argument("--existing-only", action="store_true")
    ap.add_argument("--root", default=HERE, help="the checkout whose package is timed")
    args = ap.parse_args()
    import torch
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    g = _load(os.path.join(root, "__graft_entry__.py"), "__graft_entry__")
    pkg = g.load_package()
    fc = _load(os.path.join(HERE, "tests", "fair_cases.py"), "fair_cases")
    wl = pkg.workload.make_workload(5)
    R, P, k, cap = wl.reqs.shape[0], wl.pods.shape[0], args.k, args.cap
    rng = np.random.default_rng(0xFA12)
    band3 = rng.integers(0, 3, size=R).astype(np.uint8)
    tail = np.clip(np.floor((rng.pareto(1.1, size=R) + 1.0) * 4.0), 1, 8192).astype(np.uint32)
    cost_cap = cap * int(round(float(tail.mean())))
    flows = {nf: fc.heavy_flows(rng, R, nf) for nf in (1, 16, 256, 1024)}
    with pkg.BatchedPicker(wl.chain, max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots) as pk, \
            pkg.BatchedPicker([(1, 1)], max_pods=64, max_blocks=0, max_batch=64) as empty:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        st = torch.cuda.Stream()
        torch.cuda.set_stream(st)
        s = st.cuda_stream
        d_reqs = torch.from_numpy(wl.reqs.view(np.int64)).cuda()
        d_lists = torch.empty((R, k), dtype=torch.int32, device="cuda")
        d_none = torch.full((R, k), -1, dtype=torch.int32, device="cuda")
        d_ls = torch.empty((R, k), dtype=torch.float64, device="cuda")
        d_pick = torch.empty(R, dtype=torch.int32, device="cuda")
        d_score = torch.empty(R, dtype=torch.float64, device="cuda")
        d_rank = torch.empty(R, dtype=torch.uint8, device="cuda")
        d_load = torch.zeros(P, dtype=torch.int32, device="cuda")
        d_band3 = torch.from_numpy(band3).cuda()
        d_unit = torch.ones(R, dtype=torch.int32, device="cuda")
        d_tail = torch.from_numpy(tail.view(np.int32)).cuda()
        d_flows = {nf: torch.from_numpy(f.view(np.int16)).cuda() for nf, f in flows.items()}
        assert pk._lib.eppk_pick_topk_device(pk._ctx, d_reqs.data_ptr(), R, None, k, d_lists.data_ptr(), d_ls.data_ptr(), s) == 0
        torch.cuda.synchronize()
        out_ptrs = (d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr(), s)
        tables = {1: [(0, 0)], 3: [(0, 0)] * 3}
        bands = {1: (None, None), 3: (band3, d_band3.data_ptr())}
        costs = {"unit": (None, None, cap), "tail": (tail, d_tail.data_ptr(), cost_cap)}
        legs, costed, fair = {}, {}, {}
        for nb in (1, 3):
            legs[f"banded_{nb}"] = (lambda load=None, nb=nb: pk.bounded_resolve_banded_device(
                d_lists.data_ptr(), d_ls.data_ptr(), R, k, bands[nb][1], tables[nb], None, cap, load, *out_ptrs))
            for name, d_cost, cost, c_all in (("unit", d_unit, np.ones(R, dtype=np.uint32), cap), ("tail", d_tail, tail, cost_cap)):
                costed[f"costed_{name}_{nb}"] = (cost, nb, c_all)
                legs[f"costed_{name}_{nb}"] = (lambda load=None, nb=nb, d_cost=d_cost, c_all=c_all: pk.bounded_resolve_costed_device(
                    d_lists.data_ptr(), d_ls.data_ptr(), R, k, d_cost.data_ptr(), 0, bands[nb][1], tables[nb], None, c_all, load, *out_ptrs))
        for n in (64, 512):
            legs[f"small_{n}_costed"] = (lambda load=None, n=n: pk.bounded_resolve_costed_device(
                d_lists.data_ptr(), d_ls.data_ptr(), n, k, d_tail.data_ptr(), 0, d_band3.data_ptr(), tables[3], None, cost_cap, load, *out_ptrs))
        if not args.existing_only:
            empty.publish(np.zeros(0, dtype=pkg.picker.POD_DTYPE))      # (no pods: every resolve skips its rounds)
            for nb in (1, 3):
                legs[f"order_band_b{nb}"] = (lambda load=None, nb=nb: empty.bounded_resolve_costed_device(
                    d_none.data_ptr(), None, R, k, d_tail.data_ptr(), 0, bands[nb][1], tables[nb], None, cost_cap, load, *out_ptrs))
                for nf in flows:
                    legs[f"order_fair_f{nf}_b{nb}"] = (lambda load=None, nb=nb, nf=nf: empty.bounded_resolve_fair_device(
                        d_none.data_ptr(), None, R, k, d_flows[nf].data_ptr(), nf, d_tail.data_ptr(), 0, bands[nb][1], tables[nb], None, cost_cap, load, *out_ptrs))
                    for name, (cost, d_cost, c_all) in costs.items():
                        fair[f"fair_{name}_f{nf}_b{nb}"] = (cost, nf, nb, c_all)
                        legs[f"fair_{name}_f{nf}_b{nb}"] = (lambda load=None, nb=nb, nf=nf, d_cost=d_cost, c_all=c_all: pk.bounded_resolve_fair_device(
                            d_lists.data_ptr(), d_ls.data_ptr(), R, k, d_flows[nf].data_ptr(), nf, d_cost, 0, bands[nb][1], tables[nb], None, c_all, load,
                            *out_ptrs))
            for n in (64, 512):
                legs[f"small_{n}_fair"] = (lambda load=None, n=n: pk.bounded_resolve_fair_device(
                    d_lists.data_ptr(), d_ls.data_ptr(), n, k, d_flows[16].data_ptr(), 16, d_tail.data_ptr(), 0, d_band3.data_ptr(), tables[3], None, cost_cap,
                    load, *out_ptrs))
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
        out["mean_cost"], out["cost_cap"] = float(tail.mean()), cost_cap
        lists, totals = d_lists.cpu().numpy(), d_ls.cpu().numpy()

        def outputs(f):
            d_load.zero_()
            f(d_load.data_ptr())
            assert pk.launch_status() == 0
            return d_pick.cpu().numpy(), d_score.cpu().numpy(), d_rank.cpu().numpy(), d_load.cpu().numpy().view(np.uint32)

        def same(got, want, name):
            for a, b, what in zip(got, want[:4], ("picks", "scores", "ranks", "loads")):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name}: {what} differ from the restatement"

        zeros = np.zeros(P, dtype=np.uint32)
        got = {}
        for name, (cost, nb, c_all) in costed.items():
            got[name] = outputs(legs[name])
            same(got[name], fc.ref.costed.resolve(lists, totals, P, cost, tables[nb], bands[nb][0], None, c_all, zeros), name)
        for name, (cost, nf, nb, c_all) in fair.items():
            got[name] = outputs(legs[name])
            same(got[name], fc.ref.resolve(lists, totals, P, flows[nf], nf, cost, tables[nb], bands[nb][0], None, c_all, zeros), name)
        for name in got:
            out[name]["checked_against_restatement"] = True
        if fair:
            # what the feature is for: who gets the room.  The busiest flow's share of the batch, of the placed requests under the costed
            # resolve (batch order) and under the fair one, and the flows with requests that get nothing
            shares = {}
            for nf in (16, 256, 1024):
                for kind in ("unit", "tail"):
                    for nb in (1, 3):
                        f = flows[nf]
                        cnt = np.bincount(f, minlength=nf)
                        big = int(np.argmax(cnt))
                        row = {"busiest_flow_share_of_batch": float(cnt[big]) / R, "flows_with_requests": int(np.count_nonzero(cnt))}
                        for label, name in (("costed", f"costed_{kind}_{nb}"), ("fair", f"fair_{kind}_f{nf}_b{nb}")):
                            placed = got[name][2] < k
                            slots = np.bincount(f[placed], minlength=nf)
                            row[label] = {"placed": int(placed.sum()), "busiest_flow_share_of_placed": float(slots[big]) / max(1, int(placed.sum())),
                                          "flows_with_nothing": int(np.count_nonzero((cnt > 0) & (slots == 0)))}
                        shares[f"{kind}_f{nf}_b{nb}"] = row
            out["shares"] = shares
    print(json.dumps(out))


if __name__ == "__main__":
    main()
