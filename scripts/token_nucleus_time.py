"""Device time of top-p / min-p sampling (dllm_token_sample_ex) at the real vocabulary, V = 50257, for
M in {1, 64, 2048} rows of f16 and f32 logits, temperature 0.7, against the sampler's own arms in the
same process (dllm_token_sample with top_k 0 and 50) and the torch route a caller had before: sort
descending, softmax, cumsum, mask, torch.multinomial on f32.

Arms, interleaved in every round of one process: `sample_k0`, `sample_k50`, `ex_p90` (top_p 0.9),
`ex_k50_p90` (top_k 50, then top_p 0.9), `ex_m05` (min_p 0.05), `torch_p90`, on padded rows
(ld = 50260: every group of four aligned).  0.2 s warm-up per arm, HIP events around `reps`
back-to-back calls (the library's straight into the C ABI).  Every arm rotates over enough buffer
sets that the bytes between two uses of a line exceed the 256 MiB Infinity Cache where that takes at
most `max_sets` sets; at M = 1 it cannot, and the figures there are launch-latency figures.  Within
one call the search's later passes find their row in L2 or the Infinity Cache whatever the rotation.

Usage: python scripts/token_nucleus_time.py [--rounds 7] [--reps 20] [--out profiles/token_nucleus/times.json]"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

V = 50257
LD = 50260
T = 0.7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-sets", type=int, default=96)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as g
    d = g.load_package()
    L = d._lib.load()
    assert torch.cuda.is_available(), "needs a GPU: a timing taken elsewhere says nothing"
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    results = []
    for dtype, code, esize in ((torch.float16, 1, 2), (torch.float32, 0, 4)):
        for M in (1, 64, 2048):
            nbytes = M * V * esize
            sets = max(2, min(args.max_sets, -(-(512 << 20) // nbytes)))
            gen = torch.Generator(device="cuda").manual_seed(M)
            bufs = [(2.0 * torch.randn(M, LD, device="cuda", generator=gen)).to(dtype) for _ in range(sets)]
            tokens = torch.empty(M, dtype=torch.int32, device="cuda")
            stats = torch.empty(M, 4, device="cuda")
            wsb = L.dllm_token_sample_ex_workspace(M, V, 50, 0.9, 0.05)
            ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
            k = [0]
            calls = [0]

            def nxt():
                k[0] = (k[0] + 1) % sets
                return bufs[k[0]]

            def sample(top_k):
                calls[0] += 1
                assert L.dllm_token_sample(P(nxt()), code, M, V, LD, T, top_k, None, 1234, calls[0] * M, P(tokens),
                                           P(stats), P(ws), wsb, st) == 0

            def ex(top_k, top_p, min_p):
                calls[0] += 1
                assert L.dllm_token_sample_ex(P(nxt()), code, M, V, LD, T, top_k, top_p, min_p, None, 1234, calls[0] * M,
                                              P(tokens), P(stats), P(ws), wsb, st) == 0

            def torch_arm(top_p):
                x = nxt()[:, :V].float()
                srt, idx = torch.sort(x / T, dim=-1, descending=True)
                p = torch.softmax(srt, dim=-1)
                before = torch.cumsum(p, dim=-1) - p                  # the mass above each place
                p = p.masked_fill(before >= top_p, 0.0)
                return idx.gather(-1, torch.multinomial(p, 1))

            ops = {"sample_k0": lambda: sample(0), "sample_k50": lambda: sample(50), "ex_p90": lambda: ex(0, 0.9, 0.0),
                   "ex_k50_p90": lambda: ex(50, 0.9, 0.0), "ex_m05": lambda: ex(0, 1.0, 0.05),
                   "torch_p90": lambda: torch_arm(0.9)}
            # the arms compute the same thing: the mean number of tokens the nucleus keeps, both routes
            ex(0, 0.9, 0.0)
            torch.cuda.synchronize()
            y = bufs[k[0]][:, :V].float() * (1.0 / T)
            kept = float((y >= stats[:, 3:4]).sum(dim=-1).float().mean())
            p = torch.softmax(y.double(), dim=-1).sort(dim=-1, descending=True).values
            kept_f64 = float(((torch.cumsum(p, dim=-1) - p) < 0.9).sum(dim=-1).float().mean())
            for fn in ops.values():
                t0 = time.time()
                while time.time() - t0 < 0.2:
                    fn()
                torch.cuda.synchronize()
            times = {name: [] for name in ops}
            for _ in range(args.rounds):
                for name, fn in ops.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.reps):
                        fn()
                    b.record()
                    torch.cuda.synchronize()
                    times[name].append(a.elapsed_time(b) / args.reps * 1e3)
            row = {"M": M, "V": V, "dtype": "f16" if code else "f32", "temperature": T, "logits_bytes": nbytes,
                   "sets": sets, "rounds": args.rounds, "reps": args.reps, "nucleus_kept_mean": kept,
                   "nucleus_kept_mean_f64_softmax": kept_f64}
            for name, ts in times.items():
                med = statistics.median(ts)
                row[name] = {"median_us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}
            for name, parent in (("ex_p90", "sample_k0"), ("ex_k50_p90", "sample_k50"), ("ex_m05", "sample_k0")):
                row[name]["over_" + parent] = round(row[name]["median_us"] / row[parent]["median_us"], 2)
                row[name]["search_us"] = round(row[name]["median_us"] - row[parent]["median_us"], 2)
            row["ex_p90"]["torch_over_this"] = round(row["torch_p90"]["median_us"] / row["ex_p90"]["median_us"], 2)
            print(json.dumps(row), flush=True)
            results.append(row)
            del bufs
            torch.cuda.empty_cache()
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
