"""Per-shape timing behind the routing rule of `orp_token_linear_pays`: two sides at the linears of Swin-T, batch 1 -- the stock span
(F.linear plus its F.gelu or its residual addition: what the modules launch) and the one bf16-pieces launch (token_linear(force=True)).

    python tests/checks/time_token_linear.py [--out FILE.jsonl] [--calls 20] [--rounds 4] [--size 1024]

Each side: HIP events around `calls` calls (at least 20) after a warm-up pass, replayed as ONE captured graph -- how the benchmark and
the captured inference path run them; an eager loop would time the host --, cycling through enough distinct input / residual / output
buffers (more than 320 MiB in total: beyond the 256 MB Infinity Cache) that no call finds its operands or its own previous output in
a cache.  The sides alternate `rounds` times; the first round is dropped, the others kept.  Run it at --size 1024 and --size 1536 and
route a (K, N, epilogue) row only where the SLOWEST kept figure of the new launch is below the FASTEST kept figure of the stock span at
both sizes (docs/notebook/round29.md).  Prints (and with --out appends) one JSON line per shape: the raw times, the bytes the fused
launch has to move (x + residual + y; the stock span moves y again per extra kernel), its FLOP (fp32-equivalent), the floors at
6.29 TB/s and at six bf16 products per FLOP pair on 2.5 PFLOP/s, and which of the two bounds the row."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

HBM, MATRIX = 6.29e12, 2.5e15 / 6
RING_BYTES = 320 << 20
DEPTHS = (2, 2, 6, 2)


def shapes(size):
    """(name, tokens, K, N, bias, act, residual, calls per image) of Swin-T at a size x size image: 4 stages x 4 linears + 3 merges"""
    out = []
    side = size // 4
    for s in range(4):
        C, T = 96 << s, side * side
        out += [("s%d qkv" % (s + 1), T, C, 3 * C, True, None, False, DEPTHS[s]), ("s%d proj" % (s + 1), T, C, C, True, None, True, DEPTHS[s]),
                ("s%d fc1" % (s + 1), T, C, 4 * C, True, 'gelu', False, DEPTHS[s]), ("s%d fc2" % (s + 1), T, 4 * C, C, True, None, True, DEPTHS[s])]
        if s < 3:
            side = (side + 1) // 2
            out.append(("s%d merge" % (s + 1), side * side, 4 * C, 2 * C, False, None, False, 1))
    return out


def time_shape(dev, T, K, N, bias, act, res, calls, rounds):
    from orientedreppoints_amd.mmdet_ops.token_linear import stock_linear, token_linear
    lin = torch.nn.Linear(K, N, bias=bias).to(dev).eval()
    per_set = (K + (2 if res else 1) * N) * T * 4
    nbuf = max(3, -(-RING_BYTES // per_set))
    xs = [torch.randn(1, T, K, device=dev) for _ in range(nbuf)]
    rs = [torch.randn(1, T, N, device=dev) if res else None for _ in range(nbuf)]
    outs = [None] * nbuf                  # the last nbuf outputs stay alive: the allocator hands out nbuf distinct blocks in turn
    n = max(20, calls, 2 * nbuf)

    def stock(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = stock_linear(lin, xs[i % nbuf], act, rs[i % nbuf])

    def fused(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = token_linear(xs[i % nbuf], lin, act, rs[i % nbuf], force=True)

    def run(fn):
        for i in range(nbuf):
            fn(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for i in range(n):
                fn(i)
        graph.replay()
        torch.cuda.synchronize()
        e0.record()
        graph.replay()
        e1.record()
        torch.cuda.synchronize()
        del graph
        for i in range(nbuf):
            outs[i] = None
        return e0.elapsed_time(e1) * 1e3 / n          # us per call

    t = {"stock": [], "fused": []}
    with torch.no_grad():
        for _ in range(rounds):
            t["stock"].append(run(stock))
            t["fused"].append(run(fused))
    return {k: v[1:] for k, v in t.items()}, per_set, nbuf, n          # (one round dropped)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4, help="alternations of the two sides; the first is dropped")
    ap.add_argument("--size", type=int, default=1024, help="image side")
    ap.add_argument("--only", default="", help="substring of the row names to time")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_token_linear.py needs a GPU")
    dev = torch.device("cuda:0")
    for name, T, K, N, bias, act, res, per_image in shapes(args.size):
        if args.only not in name:
            continue
        t, nbytes, nbuf, n = time_shape(dev, T, K, N, bias, act, res, args.calls, max(2, args.rounds))
        flop = 2.0 * T * K * N
        floor_mem, floor_mat = nbytes / HBM * 1e6, flop / MATRIX * 1e6
        row = dict(name=name, size=args.size, tokens=T, k=K, n=N, epilogue=(1 if bias else 0) | (2 if act else 0) | (4 if res else 0),
                   calls_per_image=per_image, buffers=nbuf, calls=n, stock_us=[round(v, 2) for v in t["stock"]],
                   fused_us=[round(v, 2) for v in t["fused"]], bytes=nbytes, flop=flop, hbm_floor_us=round(floor_mem, 2),
                   matrix_floor_us=round(floor_mat, 2), binds="HBM" if floor_mem >= floor_mat else "matrix",
                   fused_gbs=round(nbytes / (max(t["fused"]) * 1e-6) / 1e9, 1), fused_tflops=round(flop / (max(t["fused"]) * 1e-6) / 1e12, 1),
                   pays=max(t["fused"]) < min(t["stock"]))
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
