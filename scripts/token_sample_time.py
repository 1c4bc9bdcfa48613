"""Device time of token sampling (dllm_token_sample) at the real vocabulary, V = 50257, for M in
{1, 64, 2048} rows of f16 and f32 logits and top_k in {0, 50}, temperature 0.7, against two
baselines: dllm_token_readout (tokens + stats) on the same logits -- the floor: one read of the
logits and the same EXP work -- and the torch route a caller had before: a torch.topk mask,
softmax(logits / T), torch.multinomial.

Arms, interleaved in every round of one process: `readout`, `sample_k0`, `sample_k50`, `torch_k0`,
`torch_k50`, on padded rows (ld = 50260: every group of four aligned).  0.2 s warm-up per arm, HIP
events around `reps` back-to-back calls (the library's straight into the C-ABI).  Every arm rotates
over enough buffer sets that the bytes between two uses of a line exceed the 256 MiB Infinity Cache
where that takes at most `max_sets` sets; at M = 1 it cannot, and the figures there are
launch-latency figures.  Within one call the select's later passes and the pick's re-read of one
chunk find their row in L2 or the Infinity Cache whatever the rotation.

Usage: python scripts/token_sample_time.py [--rounds 7] [--reps 20] [--out profiles/token_sample/times.json]"""
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
            stats = torch.empty(M, 3, device="cuda")
            wsb = max(L.dllm_token_sample_workspace(M, V, 50), L.dllm_token_readout_workspace(M, V))
            ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
            k = [0]
            calls = [0]

            def nxt():
                k[0] = (k[0] + 1) % sets
                return bufs[k[0]]

            def readout():
                assert L.dllm_token_readout(P(nxt()), code, M, V, LD, P(tokens), P(stats), None, P(ws), wsb, st) == 0

            def sample(top_k):
                calls[0] += 1
                assert L.dllm_token_sample(P(nxt()), code, M, V, LD, T, top_k, None, 1234, calls[0] * M, P(tokens),
                                           P(stats), P(ws), wsb, st) == 0

            def torch_arm(top_k):
                x = nxt()[:, :V].float()
                if top_k:
                    kth = torch.topk(x, top_k, dim=-1).values[:, -1:]
                    x = x.masked_fill(x < kth, float("-inf"))
                return torch.multinomial(torch.softmax(x / T, dim=-1), 1)

            ops = {"readout": readout, "sample_k0": lambda: sample(0), "sample_k50": lambda: sample(50),
                   "torch_k0": lambda: torch_arm(0), "torch_k50": lambda: torch_arm(50)}
            # the arms compute the same thing: with top_k = 1 the draw is the readout's greedy token
            readout()
            greedy = tokens.clone()
            assert L.dllm_token_sample(P(bufs[k[0]]), code, M, V, LD, T, 1, None, 0, 0, P(tokens), P(stats), P(ws), wsb, st) == 0
            torch.cuda.synchronize()
            agree = float((tokens == greedy).float().mean())
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
                   "sets": sets, "rounds": args.rounds, "reps": args.reps, "top1_agrees_with_readout": agree}
            for name, ts in times.items():
                med = statistics.median(ts)
                row[name] = {"median_us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}
            for name in ("sample_k0", "sample_k50"):
                row[name]["over_readout"] = round(row[name]["median_us"] / row["readout"]["median_us"], 2)
                row[name]["torch_over_this"] = round(row["torch_" + name[7:]]["median_us"] / row[name]["median_us"], 2)
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
