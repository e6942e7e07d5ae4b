"""Weighted fair shares with carried turns (SEMANTICS.md §3h) at full size: C5 (64k requests x 4096 pods, full chain + prefix index),
k = 4, SHED, the heavy-tailed costs of DESIGN.md §3.13, one band and three, 1 / 16 / 256 / 1 024 flows drawn heavy-tailed.

Times the resolve alone over the lists eppk_pick_topk_device delivers -- HIP events on the launch stream after a warm-up of every leg,
`--rounds` rounds of `--reps` calls each, the legs alternating in one process, median / min / max over the rounds:
  fair_f*_b*        (a) eppk_fair_resolve_device: the yardstick, in the same run (eppk_fair.hip.h is not edited by §3h)
  wfair_null_f*_b*  (b) eppk_wfair_resolve_device with d_weight and d_turns NULL: the same answer through the weighted order
  wfair_wt_f*_b*    (c) ... with random weights 1 .. 16 and random turns of up to four cycles, d_turns carried from call to call (reset in
                    front of every round, outside the timed window)
  wfair_w_f*_b*     (c) without d_turns: the weighted order alone.  (c) - this = the two trailing launches (wfair_taken_kernel,
                    wfair_carry_kernel), and whatever turns other than zero cost the scatter
The last batch of every leg is checked against the restatements under tests/: a timing of wrong picks is worth nothing.  Then what the
feature is for, per leg (c): the share of the placed requests per weight class against the share of the weights, next to the same
under equal weights (b).  One JSON line.

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
    ap.add_argument("--reps", type=int, default=50, help="timed calls per leg and round")
    ap.add_argument("--rounds", type=int, default=5, help="rounds of the alternating legs")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--cap", type=int, default=8, help="the cost cap is this many mean costs (8 x 4096 pods: room for half the batch)")
    ap.add_argument("--flows", default="1,16,256,1024")
    args = ap.parse_args()
    import torch
    sys.path.insert(0, HERE)
    g = _load(os.path.join(HERE, "__graft_entry__.py"), "__graft_entry__")
    pkg = g.load_package()
    wc = _load(os.path.join(HERE, "tests", "wfair_cases.py"), "wfair_cases")
    wl = pkg.workload.make_workload(5)
    R, P, k = wl.reqs.shape[0], wl.pods.shape[0], args.k
    rng = np.random.default_rng(0x3FA1)
    band3 = rng.integers(0, 3, size=R).astype(np.uint8)
    tail = np.clip(np.floor((rng.pareto(1.1, size=R) + 1.0) * 4.0), 1, 8192).astype(np.uint32)
    cost_cap = args.cap * int(round(float(tail.mean())))
    n_flows = [int(x) for x in args.flows.split(",")]
    flows = {nf: wc.fc.heavy_flows(rng, R, nf) for nf in n_flows}
    weights = {nf: rng.integers(1, 17, size=nf).astype(np.uint16) for nf in n_flows}
    turns = {(nf, nb): (rng.random((nb, nf)) * 4 * weights[nf]).astype(np.uint32) for nf in n_flows for nb in (1, 3)}
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
        d_tail = torch.from_numpy(tail.view(np.int32)).cuda()
        d_flows = {nf: torch.from_numpy(f.view(np.int16)).cuda() for nf, f in flows.items()}
        d_weights = {nf: torch.from_numpy(w.view(np.int16)).cuda() for nf, w in weights.items()}
        d_turns0 = {key: torch.from_numpy(t.view(np.int32)).cuda() for key, t in turns.items()}
        d_turns = {key: t.clone() for key, t in d_turns0.items()}
        assert pk._lib.eppk_pick_topk_device(pk._ctx, d_reqs.data_ptr(), R, None, k, d_lists.data_ptr(), d_ls.data_ptr(), s) == 0
        torch.cuda.synchronize()
        out_ptrs = (d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr(), s)
        tables = {1: [(0, 0)], 3: [(0, 0)] * 3}
        bands = {1: (None, None), 3: (band3, d_band3.data_ptr())}
        legs, checks = {}, {}
        for nb in (1, 3):
            for nf in n_flows:
                head = (d_lists.data_ptr(), d_ls.data_ptr(), R, k, d_flows[nf].data_ptr(), nf)
                rest = (d_tail.data_ptr(), 0, bands[nb][1], tables[nb], None, cost_cap)
                legs[f"fair_f{nf}_b{nb}"] = (lambda load=None, head=head, rest=rest: pk.bounded_resolve_fair_device(*head, *rest, load, *out_ptrs))
                for name, d_w, d_t in (("null", None, None), ("wt", d_weights[nf].data_ptr(), d_turns[(nf, nb)].data_ptr()), ("w", d_weights[nf].data_ptr(), None)):
                    legs[f"wfair_{name}_f{nf}_b{nb}"] = (lambda load=None, head=head, rest=rest, d_w=d_w, d_t=d_t: pk.bounded_resolve_wfair_device(
                        *head, d_w, d_t, *rest, load, *out_ptrs))
                    checks[f"wfair_{name}_f{nf}_b{nb}"] = (nf, nb, None if d_w is None else weights[nf], None if d_t is None else turns[(nf, nb)])
                checks[f"fair_f{nf}_b{nb}"] = (nf, nb, None, None)

        def reset_turns():
            for key, t in d_turns.items():
                t.copy_(d_turns0[key])

        for f in legs.values():                 # warm-up: code objects, scratch, the dynamic-LDS limit
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {n: [] for n in legs}
        for _ in range(args.rounds):
            reset_turns()
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
        out["geometry"] = dict(zip(("chunk", "one_launch_max"), pk.bounded_geometry()))
        out["mean_cost"], out["cost_cap"] = float(tail.mean()), cost_cap
        lists, totals = d_lists.cpu().numpy(), d_ls.cpu().numpy()
        zeros = np.zeros(P, dtype=np.uint32)
        got = {}
        for name, (nf, nb, w, t) in checks.items():
            reset_turns()
            d_load.zero_()
            legs[name](d_load.data_ptr())
            assert pk.launch_status() == 0
            got[name] = (d_pick.cpu().numpy(), d_score.cpu().numpy(), d_rank.cpu().numpy(), d_load.cpu().numpy().view(np.uint32))
            want = wc.ref.resolve(lists, totals, P, flows[nf], nf, w, t, tail, tables[nb], bands[nb][0], None, cost_cap, zeros)
            for a, b, what in zip(got[name], want[:4], ("picks", "scores", "ranks", "loads")):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{name}: {what} differ from the restatement"
            if t is not None:
                assert np.array_equal(d_turns[(nf, nb)].cpu().numpy().view(np.uint32), want[5]), f"{name}: turns differ from the restatement"
            out[name]["checked_against_restatement"] = True
        # the differences the documents quote, per leg: (b) - (a), (c) - (a), and the trailing launches (c) - (c without d_turns)
        diffs = {}
        for nb in (1, 3):
            for nf in n_flows:
                a, b, c, w = (out[f"{p}_f{nf}_b{nb}"]["us_median"] for p in ("fair", "wfair_null", "wfair_wt", "wfair_w"))
                diffs[f"f{nf}_b{nb}"] = {"fair_us": a, "null_minus_fair_us": b - a, "weighted_minus_fair_us": c - a, "trailing_launches_us": c - w,
                                        "trailing_share_of_weighted": (c - w) / c}
        out["differences"] = diffs
        # what the feature is for: the share of the placed requests per weight class against the share of the weights among the flows that
        # have requests (turns of zero, so that the batch alone is seen), next to the same flows under equal weights
        shares = {}
        for nf in n_flows:
            if nf == 1:
                continue
            for nb in (1, 3):
                f, w = flows[nf], weights[nf].astype(np.int64)
                live = np.bincount(f, minlength=nf) > 0
                placed_w, placed_e = got[f"wfair_w_f{nf}_b{nb}"][2] < k, got[f"wfair_null_f{nf}_b{nb}"][2] < k
                row = {"placed_weighted": int(placed_w.sum()), "placed_equal": int(placed_e.sum()), "classes": {}}
                for lo, hi in ((1, 4), (5, 8), (9, 12), (13, 16)):
                    cls = live & (w >= lo) & (w <= hi)
                    row["classes"][f"w{lo}-{hi}"] = {
                        "flows": int(cls.sum()), "share_of_weights": float(w[cls].sum()) / float(w[live].sum()),
                        "share_of_requests": float(np.count_nonzero(cls[f])) / R,
                        "share_of_placed_weighted": float(np.count_nonzero(cls[f[placed_w]])) / max(1, int(placed_w.sum())),
                        "share_of_placed_equal": float(np.count_nonzero(cls[f[placed_e]])) / max(1, int(placed_e.sum()))}
                shares[f"f{nf}_b{nb}"] = row
        out["shares"] = shares
    print(json.dumps(out))


if __name__ == "__main__":
    main()
