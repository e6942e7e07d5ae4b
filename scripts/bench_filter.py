"""The Filter phase's metric predicates (SEMANTICS.md §2c) at full size: C5 (64k requests x 4096 pods, full chain + prefix index).

Device events around EVERY launch, a warm-up, the median of `--launches` (>= 200) launches per leg; the legs that are compared alternate
inside one loop, in one process.  Legs:
  (a) eppk_filter_masks_device with and without mask_in for a threshold-only program, a LoRA program and one with QUEUE_WITHIN
      (a context per program: eppk_set_filters between launches would rebuild the planes every time).  For the non-WITHIN legs the
      achieved bytes/s from 2 R J 8 bytes (R J 8 without mask_in) against the 6.29 TB/s measured-copy ceiling.
  (b) eppk_pick_filtered_device(k = 1) against eppk_pick_topk_device(k = 1) on the SAME mask rows, prebuilt by the filter: the
      difference is what the filter costs a caller.
  (c) the host-built alternative the feature replaces: the numpy restatement's masks (timed on `--host-rows` rows and scaled to the
      batch: it is a per-row loop), then eppk_pick_topk with those rows from host memory (wall clock).
Prints a table and one JSON line."""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

COPY_CEILING = 6.29e12      # bytes/s, measured device copy


def _ref():
    spec = importlib.util.spec_from_file_location("filter_ref", os.path.join(ROOT, "tests", "filter_ref.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200, help="timed launches per leg (median)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-rows", type=int, default=2048, help="rows the numpy restatement is timed on (scaled to the batch)")
    ap.add_argument("--requests", type=int, default=None, help="override R (default: C5's 65536)")
    args = ap.parse_args()
    assert args.launches >= 200 or args.requests, "the median is over at least 200 launches"
    import torch
    pkg = g.load_package()
    ref = _ref()
    PK = pkg.picker.PredicateKind
    REQ, PREF = int(pkg.picker.OnEmpty.REQUIRE), int(pkg.picker.OnEmpty.PREFER)
    wl = pkg.workload.make_workload(5, R=args.requests)
    R, P = wl.reqs.shape[0], wl.pods.shape[0]
    J = (P + 63) // 64
    rng = np.random.default_rng(5)
    mask = rng.integers(0, 1 << 63, (R, J), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (R, J), dtype=np.uint64)     # 50 % density
    programs = {"thr": [(PK.KV_LE, REQ, 0.8), (PK.QUEUE_LE, PREF, 48)],
                "lora": [(PK.LORA_SERVABLE, REQ, 0), (PK.KV_LE, PREF, 0.9)],
                "within": [(PK.KV_LE, REQ, 0.9), (PK.QUEUE_WITHIN, PREF, 8)]}
    st = torch.cuda.Stream()
    torch.cuda.set_stream(st)
    s = st.cuda_stream
    d_reqs = torch.from_numpy(wl.reqs.view(np.int64)).cuda()
    d_mask = torch.from_numpy(mask.view(np.int64)).cuda()
    d_out = torch.empty((R, J), dtype=torch.int64, device="cuda")
    d_built = torch.empty((R, J), dtype=torch.int64, device="cuda")
    d_verdict = torch.empty(R, dtype=torch.uint8, device="cuda")
    d_pick = torch.empty(R, dtype=torch.int32, device="cuda")
    d_score = torch.empty(R, dtype=torch.float64, device="cuda")
    pks = {}
    for name, prog in programs.items():
        pk = pkg.BatchedPicker(wl.chain, max_pods=P, max_blocks=wl.B, max_batch=R, index_slots=wl.index_slots)
        pk.publish(wl.pods)
        pk.index_insert(wl.index_hashes, wl.index_pods)
        pk.set_filters([prog])
        pks[name] = pk
    legs = {}
    for name, pk in pks.items():
        for m in (True, False):
            legs[f"filter_{name}_{'mask' if m else 'nomask'}"] = (
                lambda pk=pk, m=m: pk.filter_masks_device(d_reqs.data_ptr(), R, None, d_mask.data_ptr() if m else None, d_out.data_ptr(), d_verdict.data_ptr(), s))
    pk = pks["thr"]
    pk.filter_masks_device(d_reqs.data_ptr(), R, None, d_mask.data_ptr(), d_built.data_ptr(), None, s)      # the prebuilt rows of leg (b)
    lib = pk._lib

    def topk_prebuilt():
        rc = lib.eppk_pick_topk_device(pk._ctx, d_reqs.data_ptr(), R, d_built.data_ptr(), 1, d_pick.data_ptr(), d_score.data_ptr(), s)
        assert rc == 0, rc
    legs["pick_filtered_k1"] = lambda: pk.pick_filtered_device(d_reqs.data_ptr(), R, None, d_mask.data_ptr(), 1, d_pick.data_ptr(), d_score.data_ptr(),
                                                               d_verdict.data_ptr(), s)
    legs["pick_topk_k1_prebuilt"] = topk_prebuilt
    for _ in range(args.warmup):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    events = {n: [] for n in legs}
    for _ in range(args.launches):                       # the legs alternate: launch i of every leg before launch i + 1 of any
        for n, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            f()
            e1.record(st)
            events[n].append((e0, e1))
    torch.cuda.synchronize()
    out = {"shape": f"{R} x {P}", "launches": args.launches}
    for n, ev in events.items():
        us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
        out[n] = {"us_median": float(np.median(us)), "us_p10": float(np.percentile(us, 10)), "us_p90": float(np.percentile(us, 90))}
        if n.startswith("filter_") and "within" not in n:
            nbytes = (2 if n.endswith("_mask") else 1) * R * J * 8
            out[n]["bytes"] = nbytes
            out[n]["TB_per_s"] = nbytes / (out[n]["us_median"] * 1e-6) / 1e12
            out[n]["of_copy_ceiling"] = out[n]["TB_per_s"] * 1e12 / COPY_CEILING
    out["filter_cost_us"] = out["pick_filtered_k1"]["us_median"] - out["pick_topk_k1_prebuilt"]["us_median"]

    # (c) the host-built alternative: masks by the restatement on the host, then eppk_pick_topk with 33.5 MB of mask rows from host memory
    hr = min(args.host_rows, R)
    adapter = (wl.reqs[:, 0] & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    t0 = time.perf_counter()
    host_masks, _ = ref.filter_mask_words(wl.pods, [programs["thr"]], adapter[:hr], None, mask[:hr])
    t_ref = (time.perf_counter() - t0) * R / hr
    torch.cuda.synchronize()
    built = d_built.cpu().numpy().view(np.uint64)
    assert np.array_equal(built[:hr], host_masks), "the device's rows differ from the restatement's"
    walls = []
    for _ in range(5):
        t0 = time.perf_counter()
        pk.pick_topk(wl.reqs, 1, built)
        walls.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    pk.pick_filtered(wl.reqs, 1, None, mask)
    out["host_built"] = {"restatement_masks_s_scaled": t_ref, "pick_topk_host_masks_ms": float(np.median(walls)) * 1e3,
                         "pick_filtered_host_call_ms": (time.perf_counter() - t0) * 1e3}
    for pk in pks.values():
        pk.close()
    for n, v in out.items():
        if isinstance(v, dict) and "us_median" in v:
            extra = f"  {v['TB_per_s']:.2f} TB/s ({100 * v['of_copy_ceiling']:.0f} % of the copy ceiling)" if "TB_per_s" in v else ""
            print(f"{n:28s} {v['us_median']:9.1f} us  (p10 {v['us_p10']:.1f}, p90 {v['us_p90']:.1f}){extra}")
    print(f"filter cost in pick_filtered  {out['filter_cost_us']:9.1f} us;  host-built: {out['host_built']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
