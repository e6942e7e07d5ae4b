"""Priority bands over the bounded picker (SEMANTICS.md §3e) at full size: C5 (64k requests x 4096 pods, full chain + prefix index), k = 4,
SHED, cap_all = 64.

Times the resolve alone over the lists eppk_pick_topk_device delivers: the plain eppk_bounded_resolve_device, and
eppk_banded_resolve_device with band bytes uniform over 1, 3 and 8 bands (reserves 0) and over 3 bands with reserves 0 / 8 / 16 -- HIP
events on the launch stream after a warm-up, `--rounds` rounds of `--reps` calls each, the legs alternating in one process, median / min /
max over the rounds.  The last batch of every leg is checked against tests/banded_ref.py: a timing of wrong picks is worth nothing.  Then
the number the bands exist for: with band bytes drawn 10 % / 60 % / 30 % (critical / standard / sheddable), how many CRITICAL requests
the plain resolve sheds, and how many the banded one.  One JSON line.

`--plain-only` times the plain resolve alone and touches nothing newer; with `--root DIR` the package is loaded from another checkout
(built there): the PARENT commit's figure in the same session, which this commit's plain leg must agree with."""
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
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--root", default=HERE, help="the checkout whose package is timed")
    args = ap.parse_args()
    import torch
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    g = _load(os.path.join(root, "__graft_entry__.py"), "__graft_entry__")
    pkg = g.load_package()
    wl = pkg.workload.make_workload(5)
    R, P, k, cap = wl.reqs.shape[0], wl.pods.shape[0], args.k, args.cap
    rng = np.random.default_rng(0xBA2D)
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
        assert pk._lib.eppk_pick_topk_device(pk._ctx, d_reqs.data_ptr(), R, None, k, d_lists.data_ptr(), d_ls.data_ptr(), s) == 0
        torch.cuda.synchronize()

        def plain(load=None):
            pk.bounded_resolve_device(d_lists.data_ptr(), d_ls.data_ptr(), R, k, None, cap, 0, load, d_pick.data_ptr(), d_score.data_ptr(), d_rank.data_ptr(), s)
        legs = {"plain": plain}
        banded = {}
        if not args.plain_only:
            for name, nb, reserves in (("banded_1", 1, (0,)), ("banded_3", 3, (0, 0, 0)), ("banded_8", 8, (0,) * 8), ("banded_3_reserve_0_8_16", 3, (0, 8, 16))):
                band = rng.integers(0, nb, size=R).astype(np.uint8)
                banded[name] = (band, torch.from_numpy(band).cuda(), [(0, r) for r in reserves])
            mix = rng.choice(3, size=R, p=[0.1, 0.6, 0.3]).astype(np.uint8)
            banded["banded_3_mix_10_60_30"] = (mix, torch.from_numpy(mix).cuda(), [(0, 0)] * 3)
            for name, (_, d_band, bands) in banded.items():
                legs[name] = (lambda load=None, d_band=d_band, bands=bands: pk.bounded_resolve_banded_device(
                    d_lists.data_ptr(), d_ls.data_ptr(), R, k, d_band.data_ptr(), bands, None, cap, load, d_pick.data_ptr(), d_score.data_ptr(),
                    d_rank.data_ptr(), s))
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

        tests = os.path.join(HERE if args.plain_only else root, "tests")
        zeros = np.zeros(P, dtype=np.uint32)
        got_plain = outputs(plain)
        same(got_plain, _load(os.path.join(tests, "bounded_ref.py"), "bounded_ref").resolve(lists, totals, P, None, cap, 0, zeros), "plain")
        out["plain"]["checked_against_restatement"] = True
        if not args.plain_only:
            ref = _load(os.path.join(tests, "banded_ref.py"), "banded_ref")
            for name, (band, _, bands) in banded.items():
                got = outputs(legs[name])
                same(got, ref.resolve(lists, totals, P, bands, band, None, cap, zeros), name)
                out[name]["checked_against_restatement"] = True
                out[name]["shed_per_band"] = [int(np.sum((got[0] < 0) & (band == b))) for b in range(len(bands))]
                out[name]["rows_per_band"] = [int(np.sum(band == b)) for b in range(len(bands))]
            mix = banded["banded_3_mix_10_60_30"][0]
            out["critical_shed"] = {"critical_requests": int(np.sum(mix == 0)), "plain": int(np.sum((got_plain[0] < 0) & (mix == 0))),
                                    "banded": out["banded_3_mix_10_60_30"]["shed_per_band"][0]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
