"""Per-span timing behind the routing rule of `orp_token_layernorm_pays`: two sides at every LayerNorm span of Swin-T, batch 1 -- the
stock span as mmdet_models/swin.py runs it with the switch off (the LayerNorm alone, pad + cat + LayerNorm, the contiguous copy +
LayerNorm, LayerNorm + the permuting copy) and the one launch (token_layernorm(force=True)).

    python tests/checks/time_swin_norm.py [--out FILE.jsonl] [--calls 20] [--rounds 4] [--size 1024] [--only NAME] [--blocks]

The method of tests/checks/time_token_linear.py: each side is HIP events around `calls` calls (at least 20) replayed as ONE captured
graph after a warm-up pass, cycling through enough distinct source / output buffers (more than 320 MiB in total: beyond the 256 MB
Infinity Cache) that no call finds its operands in a cache.  The sides alternate `rounds` times; the first round is dropped, the others
kept.  Run it at --size 1024 and --size 1536 and route a (width, layout) row only where the SLOWEST kept figure of the launch is below
the FASTEST kept figure of the stock span at both sizes (docs/notebook/round32.md).  One JSON line per span: the raw times, the bytes
the launch has to move (source + destination), the 8 T C floor at 6.29 TB/s, and the traffic rate the launch reached.

--blocks times one un-shifted SwinBlock per stage instead (tests/checks/time_swin_linear.py's method in one process): block.fuse_token_norm
False / None (the shipped routing) / forced, everything else of the block as shipped."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

HBM = 6.29e12
RING_BYTES = 320 << 20
DEPTHS = (2, 2, 6, 2)
HEADS = (3, 6, 12, 24)


class _Owner(object):
    """what `swin._norm` asks of the module that owns the LayerNorm"""
    fuse_token_norm, force_token_norm = False, False


def spans(size):
    """(name, layout, source shape, hw, normalised width, output rows, calls per image) of Swin-T at a size x size image: the embedding,
    4 stages x (norm1 / norm2, the output norm) and 3 merges"""
    side = size // 4
    out = [("embed", 'from_nchw', (1, 96, side * side), None, 96, side * side, 1)]
    for s in range(4):
        C, T = 96 << s, side * side
        out.append(("s%d norm" % (s + 1), 'tokens', (1, T, C), None, C, T, 2 * DEPTHS[s]))
        out.append(("s%d out" % (s + 1), 'to_nchw', (1, T, C), (side, side), C, T, 1))
        if s < 3:
            half = (side + 1) // 2
            out.append(("s%d merge" % (s + 1), 'merge', (1, side, side, C), None, 4 * C, half * half, 1))
            side = half
    return out


def _timed(fn, nbuf, n, clear):
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
    clear()
    return e0.elapsed_time(e1) * 1e3 / n          # us per call


def time_span(dev, layout, shape, hw, C, rows, calls, rounds):
    from orientedreppoints_amd.mmdet_models.swin import _norm
    from orientedreppoints_amd.mmdet_ops.token_norm import token_layernorm
    ln = torch.nn.LayerNorm(C).to(dev).eval()
    elems = 1
    for s in shape:
        elems *= s
    per_set = (elems + rows * C) * 4
    nbuf = max(3, -(-RING_BYTES // per_set))
    xs = [torch.randn(shape, device=dev) for _ in range(nbuf)]
    outs = [None] * nbuf                  # the last nbuf outputs stay alive: the allocator hands out nbuf distinct blocks in turn
    n = max(20, calls, 2 * nbuf)
    owner = _Owner()

    def stock(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = _norm(owner, ln, xs[i % nbuf], layout, hw)

    def fused(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = token_layernorm(xs[i % nbuf], ln, layout, hw, force=True)

    def clear():
        for i in range(nbuf):
            outs[i] = None

    t = {"stock": [], "fused": []}
    with torch.no_grad():
        for _ in range(rounds):
            t["stock"].append(_timed(stock, nbuf, n, clear))
            t["fused"].append(_timed(fused, nbuf, n, clear))
    return {k: v[1:] for k, v in t.items()}, per_set, nbuf, n          # (one round dropped)


def time_block(dev, stage, size, calls, rounds):
    from orientedreppoints_amd.mmdet_models.swin import SwinBlock
    side = size // 4
    for _ in range(stage):
        side = (side + 1) // 2
    C, T = 96 << stage, side * side
    torch.manual_seed(0)
    blk = SwinBlock(C, HEADS[stage], 7, 0, 4., True, None, 0., 0., 0.).to(dev).eval()
    nbuf = max(3, -(-RING_BYTES // (2 * T * C * 4)))
    xs = [torch.randn(1, T, C, device=dev) for _ in range(nbuf)]
    outs = [None] * nbuf
    n = max(20, calls, 2 * nbuf)

    def fn(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = blk(xs[i % nbuf], side, side, None)

    def clear():
        for i in range(nbuf):
            outs[i] = None

    t = {"stock": [], "routed": [], "forced": []}
    with torch.no_grad():
        for _ in range(rounds):
            for name, fuse, force in (("stock", False, False), ("routed", None, False), ("forced", None, True)):
                blk.fuse_token_norm, blk.force_token_norm = fuse, force
                t[name].append(_timed(fn, nbuf, n, clear))
    return {k: [round(x, 2) for x in v[1:]] for k, v in t.items()}, T, C, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4, help="alternations of the sides; the first is dropped")
    ap.add_argument("--size", type=int, default=1024, help="image side")
    ap.add_argument("--only", default="", help="substring of the span names to time")
    ap.add_argument("--blocks", action="store_true", help="one un-shifted block per stage instead of the spans")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_swin_norm.py needs a GPU")
    dev = torch.device("cuda:0")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    if args.blocks:
        for stage in range(4):
            t, T, C, n = time_block(dev, stage, args.size, args.calls, max(2, args.rounds))
            emit(dict(name="s%d block" % (stage + 1), size=args.size, tokens=T, c=C, blocks_per_image=DEPTHS[stage], calls=n,
                      stock_us=t["stock"], routed_us=t["routed"], forced_us=t["forced"]))
        return
    for name, layout, shape, hw, C, T, per_image in spans(args.size):
        if args.only not in name:
            continue
        t, nbytes, nbuf, n = time_span(dev, layout, shape, hw, C, T, args.calls, max(2, args.rounds))
        emit(dict(name=name, size=args.size, layout=layout, tokens=T, c=C, calls_per_image=per_image, buffers=nbuf, calls=n,
                  stock_us=[round(v, 2) for v in t["stock"]], fused_us=[round(v, 2) for v in t["fused"]], bytes=nbytes,
                  floor_us=round(8.0 * T * C / HBM * 1e6, 2), fused_tbs=round(nbytes / (max(t["fused"]) * 1e-6) / 1e12, 2),
                  pays=max(t["fused"]) < min(t["stock"])))


if __name__ == "__main__":
    main()
