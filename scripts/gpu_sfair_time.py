"""Fair shares in cost units (SEMANTICS.md §3i) at full size: C5 (64k requests x 4096 pods, full chain + prefix index), k = 4, SHED, the
heavy-tailed costs of DESIGN.md §3.13, one band and three, 1 / 16 / 256 / 1 024 flows drawn heavy-tailed.

Times the resolve alone over the lists eppk_pick_topk_device delivers -- HIP events on the launch stream after a warm-up of every leg,
`--rounds` rounds of `--reps` calls each, the legs alternating in one process, median / min / max over the rounds:
  sfair_f*_b*        eppk_sfair_resolve_device, NULL weights, d_service carried from call to call (zeroed in front of every round)
  wfair_f*_b*        eppk_wfair_resolve_device, NULL weights, d_turns carried alike: §3h on the same batch
  costed_b*          eppk_costed_resolve_device: what is below the order
  order_f*_b*        eppk_sfair_resolve_device on a second context WITHOUT pods: the twenty order launches and the finish alone
  small{64,512}_*    the first 64 / 512 requests: sfair with pods, sfair without pods, wfair, costed
`--root DIR` takes the package of another built checkout (the parent's) and times the wfair and costed legs alone.  The last sfair
batch of every leg is checked against tests/sfair_ref.py, the service included.  Then what the feature is for, on the same batch under
§3h and under §3i: the share of the placed COST the busiest flow takes, and the flows that get nothing.  One JSON line.

Times per kernel take a run of their own under `rocprofv3 --kernel-trace --stats` with `--rounds 1 --reps 20`."""
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
    ap.add_argument("--reps", type=int, default=20, help="timed calls per leg and round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds of the alternating legs")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--cap", type=int, default=8, help="the cost cap is this many mean costs (8 x 4096 pods: room for half the batch)")
    ap.add_argument("--flows", default="1,16,256,1024")
    ap.add_argument("--root", default=HERE, help="another built checkout: its wfair and costed legs alone")
    args = ap.parse_args()
    import torch
    own = os.path.realpath(args.root) == os.path.realpath(HERE)
    sys.path.insert(0, args.root)
    pkg = _load(os.path.join(args.root, "__graft_entry__.py"), "__graft_entry__").load_package()
    ref = _load(os.path.join(HERE, "tests", "sfair_ref.py"), "sfair_ref")
    heavy_flows = _load(os.path.join(HERE, "tests", "fair_cases.py"), "fair_cases").heavy_flows
    wl = pkg.workload.make_workload(5)
    R, P, k = wl.reqs.shape[0], wl.pods.shape[0], args.k
    rng = np.random.default_rng(0x3FA1)
    band3 = rng.integers(0, 3, size=R).astype(np.uint8)
    tail = np.clip(np.floor((rng.pareto(1.1, size=R) + 1.0) * 4.0), 1, 8192).astype(np.uint32)
    cost_cap = args.cap * int(round(float(tail.mean())))
    n_flows = [int(x) for x in args.flows.split(",")]
    flows = {nf: heavy_flows(rng, R, nf) for nf in n_flows}
    with pkg.BatchedPicker(wl.chain, max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots) as pk, \
            pkg.BatchedPicker([(1, 1)], max_pods=P, max_blocks=0, max_batch=R) as bare:
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        bare.publish(np.zeros(0, dtype=pkg.picker.POD_DTYPE))          # (no pods: the resolve skips its rounds)
        st = torch.cuda.Stream()
        torch.cuda.set_stream(st)
        s = st.cuda_stream
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view({2: np.int16, 4: np.int32, 8: np.int64}.get(a.dtype.itemsize, a.dtype))).cuda()  # noqa: E731
        d_reqs, d_band3, d_tail = dev(wl.reqs), torch.from_numpy(band3).cuda(), dev(tail)
        d_lists, d_ls = torch.empty((R, k), dtype=torch.int32, device="cuda"), torch.empty((R, k), dtype=torch.float64, device="cuda")
        d_pick, d_score = torch.empty(R, dtype=torch.int32, device="cuda"), torch.empty(R, dtype=torch.float64, device="cuda")
        d_rank, d_load = torch.empty(R, dtype=torch.uint8, device="cuda"), torch.zeros(P, dtype=torch.int32, device="cuda")
        d_flows = {nf: dev(f) for nf, f in flows.items()}
        d_table = {(nf, nb): torch.zeros((nb, nf), dtype=torch.int32, device="cuda") for nf in n_flows for nb in (1, 3)}
        d_none = torch.full((R, k), -1, dtype=torch.int32, device="cuda")
        assert pk._lib.eppk_pick_topk_device(pk._ctx, d_reqs.data_ptr(), R, None, k, d_lists.data_ptr(), d_ls.data_ptr(), s) == 0
        torch.cuda.synchronize()
        outs = (d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr(), s)
        tables = {1: [(0, 0)], 3: [(0, 0)] * 3}
        bands = {1: (None, None), 3: (band3, d_band3.data_ptr())}
        legs = {}
        for nb in (1, 3):
            rest = (d_tail.data_ptr(), 0, bands[nb][1], tables[nb], None, cost_cap)
            for n, tag in ((R, ""), (64, "small64_"), (512, "small512_")):
                legs[f"{tag}costed_b{nb}"] = (lambda load=None, n=n, rest=rest: pk.bounded_resolve_costed_device(d_lists.data_ptr(), d_ls.data_ptr(), n, k, *rest, load, *outs))
            for nf in n_flows:
                for n, tag in ((R, ""), (64, "small64_"), (512, "small512_")):
                    if tag and nf != 16:
                        continue
                    head, t = (d_lists.data_ptr(), d_ls.data_ptr(), n, k, d_flows[nf].data_ptr(), nf, None), d_table[(nf, nb)].data_ptr()
                    legs[f"{tag}wfair_f{nf}_b{nb}"] = (lambda load=None, head=head, t=t, rest=rest: pk.bounded_resolve_wfair_device(*head, t, *rest, load, *outs))
                    if own:
                        legs[f"{tag}sfair_f{nf}_b{nb}"] = (lambda load=None, head=head, t=t, rest=rest: pk.bounded_resolve_sfair_device(*head, t, *rest, load, *outs))
                        legs[f"{tag}order_f{nf}_b{nb}"] = (lambda load=None, head=head, t=t, rest=rest: bare.bounded_resolve_sfair_device(
                            d_none.data_ptr(), None, *head[2:], t, *rest, load, *outs))

        def reset():
            for t in d_table.values():
                t.zero_()

        for f in legs.values():                 # warm-up: code objects, scratch, the dynamic-LDS limits
            for _ in range(2):
                f()
        torch.cuda.synchronize()
        times = {n: [] for n in legs}
        for _ in range(args.rounds):
            reset()
            for n, f in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(args.reps):
                    f()
                e1.record(st)
                e1.synchronize()
                times[n].append(e0.elapsed_time(e1) * 1e3 / args.reps)
        out = {n: {"us_median": float(np.median(v)), "us_min": float(np.min(v)), "us_max": float(np.max(v))} for n, v in times.items()}
        out["shape"], out["k"], out["reps"], out["rounds"], out["root"] = f"{R} x {P}", k, args.reps, args.rounds, "own" if own else "other"
        out["geometry"] = dict(zip(("chunk", "one_launch_max"), pk.bounded_geometry()))
        out["mean_cost"], out["cost_cap"] = float(tail.mean()), cost_cap
        if own:
            lists, totals, zeros, effect = d_lists.cpu().numpy(), d_ls.cpu().numpy(), np.zeros(P, dtype=np.uint32), {}
            for nb in (1, 3):
                for nf in n_flows:
                    placed = {}
                    for fam in ("sfair", "wfair"):
                        reset()
                        d_load.zero_()
                        legs[f"{fam}_f{nf}_b{nb}"](d_load.data_ptr())
                        assert pk.launch_status() == 0
                        got = (d_pick.cpu().numpy(), d_score.cpu().numpy(), d_rank.cpu().numpy(), d_load.cpu().numpy().view(np.uint32))
                        placed[fam] = got[2] < k
                        if fam == "sfair":
                            want = ref.resolve(lists, totals, P, flows[nf], nf, None, np.zeros((nb, nf), dtype=np.uint32), tail, tables[nb], bands[nb][0], None,
                                               cost_cap, zeros)
                            for a, b, what in zip(got, want[:4], ("picks", "scores", "ranks", "loads")):
                                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"sfair_f{nf}_b{nb}: {what} differ from the restatement"
                            assert np.array_equal(d_table[(nf, nb)].cpu().numpy().view(np.uint32), want[5]), f"sfair_f{nf}_b{nb}: service differs"
                            out[f"sfair_f{nf}_b{nb}"]["checked_against_restatement"] = True
                    row = {}
                    for fam, p in placed.items():      # per flow the cost placed: the busiest flow's share of it, and the flows with requests that get none
                        by_flow = np.bincount(flows[nf][p], weights=tail[p].astype(np.float64), minlength=nf)
                        busiest = int(np.argmax(np.bincount(flows[nf], weights=tail.astype(np.float64), minlength=nf)))
                        row[fam] = {"placed_rows": int(p.sum()), "placed_cost": float(by_flow.sum()), "busiest_flow_share_of_placed_cost": float(by_flow[busiest] / by_flow.sum()),
                                    "flows_with_requests_and_nothing_placed": int(np.count_nonzero((np.bincount(flows[nf], minlength=nf) > 0) & (by_flow == 0)))}
                    effect[f"f{nf}_b{nb}"] = row
            out["effect"] = effect
    print(json.dumps(out))


if __name__ == "__main__":
    main()
