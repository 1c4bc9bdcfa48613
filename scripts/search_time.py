"""Device time of the compressed-vector search (dllm_search_vectors) next to the only way to ask the
same question without it: decompress the store to f32, then torch normalise, matmul and topk.

Store: rows x dim codes (default 1 Mi x 768, the default configuration's hidden size, 0.8 GB), 8-bit
rows of N(0,1) data; nq = 1, 4, 16; k = 10.  One process, the search and the baseline interleaved in
every round, 0.2 s warm-up per op, HIP events around `reps` back-to-back calls straight into the
C-ABI (the table is prebuilt: it is per store, not per query).  Every op rotates over `sets` stores;
one store alone is already three times the 256 MiB Infinity Cache, so the bytes between two uses of
a line exceed it and the figures are HBM figures.  A second, separate pass under the torch profiler
splits the call into its kernels (scan, select, query); it is not used for the whole-call time.

codes_TB_per_s = passes x rows x dim bytes / time, passes = ceil(nq / 4) query tiles, each of which
streams the codes once; set against the 6.3 TB/s the microarchitecture notes give as achievable.

Usage: python scripts/search_time.py [--rows 1048576] [--dim 768] [--rounds 7] [--reps 20] [--sets 2]
                                     [--out profiles/search/times.json]"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

TILE = 4        # kScanTile of csrc/search.hip
SLICE = 2048    # kSlice


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--base-reps", type=int, default=2)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as g
    d = g.load_package()
    L = d._lib.load()
    assert torch.cuda.is_available(), "needs a GPU: a timing taken elsewhere says nothing"
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    rows, dim, k = args.rows, args.dim, args.k

    stores = []
    gen = torch.Generator(device="cuda").manual_seed(0)
    for _ in range(args.sets):
        codes = torch.empty(rows, dim, dtype=torch.uint8, device="cuda")
        scales = torch.empty(rows, device="cuda")
        zps = torch.empty(rows, device="cuda")
        step = 1 << 16            # compress in pieces: the f32 source of the whole store is 3.2 GB
        for a in range(0, rows, step):
            x = torch.randn(min(step, rows - a), dim, generator=gen, device="cuda")
            c, s, z = d.compress_vectors(x, 8)
            codes[a:a + step], scales[a:a + step], zps[a:a + step] = c, s, z
        stores.append((codes, scales, zps, d.search_table(codes, scales, zps)))
    torch.cuda.synchronize()

    # the table pass on its own: one read of the codes
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tab_times = []
    for r in range(args.rounds):
        codes, scales, zps, tab = stores[r % args.sets]
        a.record()
        assert L.dllm_search_table(P(codes), rows, dim, P(scales), P(zps), P(tab), st) == 0
        b.record()
        torch.cuda.synchronize()
        tab_times.append(a.elapsed_time(b) * 1e3)
    results = {"rows": rows, "dim": dim, "k": k, "rounds": args.rounds, "reps": args.reps, "sets": args.sets,
               "query_tile": TILE, "select_slice": SLICE, "store_bytes": rows * dim,
               "table_us": {"median": round(statistics.median(tab_times), 1), "min": round(min(tab_times), 1)},
               "table_TB_per_s": round(rows * dim / (statistics.median(tab_times) * 1e-6) / 1e12, 3), "cases": []}
    print(json.dumps({kk: v for kk, v in results.items() if kk != "cases"}), flush=True)

    for nq in (1, 4, 16):
        Q = torch.randn(nq, dim, generator=gen, device="cuda")
        idx = torch.empty(nq, k, dtype=torch.int32, device="cuda")
        out = torch.empty(nq, k, device="cuda")
        wsb = L.dllm_search_workspace(nq, rows, k)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        turn = [0]

        def nxt():
            turn[0] = (turn[0] + 1) % args.sets
            return stores[turn[0]]

        def search(store=None):
            codes, _, _, tab = store or nxt()
            rc = L.dllm_search_vectors(P(Q), nq, P(codes), P(tab), rows, dim, k, P(idx), P(out), P(ws), wsb, st)
            assert rc == 0

        def baseline(store=None):
            codes, scales, zps, _ = store or nxt()
            x = d.decompress_vectors(codes, scales, zps)
            xn = torch.nn.functional.normalize(x, dim=1)
            del x
            s = torch.nn.functional.normalize(Q, dim=1) @ xn.T
            return torch.topk(s, k, dim=1)

        # the two agree on what they find (ids; the scores differ by their roundings)
        search(stores[0])
        base = baseline(stores[0])
        agree = float((base.indices.int() == idx).float().mean())

        ops = {"search": (search, args.reps), "baseline": (baseline, args.base_reps)}
        for fn, _ in ops.values():
            t0 = time.time()
            while time.time() - t0 < 0.2:
                fn()
            torch.cuda.synchronize()
        times = {name: [] for name in ops}
        for _ in range(args.rounds):
            for name, (fn, reps) in ops.items():
                a.record()
                for _ in range(reps):
                    fn()
                b.record()
                torch.cuda.synchronize()
                times[name].append(a.elapsed_time(b) / reps * 1e3)
        passes = -(-nq // TILE)
        row = {"nq": nq, "passes": passes, "ids_agree_with_baseline": round(agree, 4)}
        for name, ts in times.items():
            row[name] = {"median_us": round(statistics.median(ts), 1), "min_us": round(min(ts), 1),
                         "max_us": round(max(ts), 1)}
        row["search"]["codes_TB_per_s"] = round(passes * rows * dim / (row["search"]["median_us"] * 1e-6) / 1e12, 3)
        row["speedup_vs_baseline"] = round(row["baseline"]["median_us"] / row["search"]["median_us"], 1)

        # per kernel, in a pass of its own under the profiler
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(args.reps):
                    search()
                torch.cuda.synchronize()
            kernels = {}
            for ev in prof.key_averages():
                total = getattr(ev, "device_time_total", None)
                if total is None:
                    total = getattr(ev, "cuda_time_total", 0.0)
                for tag in ("search_scan", "search_select", "search_query"):
                    if tag in ev.key:
                        kernels[tag] = round(kernels.get(tag, 0.0) + total / args.reps, 1)
            row["kernels_us_per_call"] = kernels
            if kernels.get("search_scan"):
                row["scan_codes_TB_per_s"] = round(passes * rows * dim / (kernels["search_scan"] * 1e-6) / 1e12, 3)
        except Exception as e:      # the split is an extra; the event timings above stand without it
            row["kernels_us_per_call"] = f"profiler unavailable: {type(e).__name__}: {e}"
        print(json.dumps(row), flush=True)
        results["cases"].append(row)
        if args.out:                    # after every case: a later failure keeps what was measured
            out_path = Path(args.out)
            out_path.parent.mkdir(parents=True, exist_ok=True)
            out_path.write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
