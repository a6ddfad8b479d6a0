"""Per-shape timing behind the routing rule of `orp_conv1x1_bn_act_pieces_dual_pays`: two sides at the four first-block shapes of
R-50 -- today's route (library downsample convolution + the bf16-pieces conv3 launch that applies the downsample BatchNorm to it,
conv1x1_bn_act(residual=downsample(x2), residual_bn=..., pieces=True)) and the dual launch (conv1x1_bn_act_dual).

    python tests/checks/time_bottleneck_dual.py [--out FILE.jsonl] [--calls 20] [--rounds 2] [--batch 1] [--size 1024]

As time_bottleneck_1x1_pieces.py: HIP events around `calls` calls (at least 20) replayed as one captured graph after a warm-up pass,
cycling through enough distinct input / output buffers (more than 320 MiB in total: beyond the Infinity Cache) that no call finds its
operands in a cache; the sides alternate `rounds` times.  Run it twice at each of the three corners the project uses (--size 1024,
--size 1024 --batch 2, --size 1536) and route a shape only where the SLOWEST dual figure of all runs beats the FASTEST figure of the
pair (docs/notebook/round17.md).  Prints (and with --out appends) one JSON line per shape with the raw times, the bytes the dual
launch has to move (x + the sampled half of the fetched lines of x2 counted as the lines it touches + y), both contractions' FLOP
(fp32-equivalent) and the floors at 6.29 TB/s and at six bf16 products per FLOP pair on 2.5 PFLOP/s."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

# (name, Cin of conv3, Cin2 of the downsample convolution, Cout, output H = W at a 1024^2 image, stride of the downsample convolution)
SHAPES = [("l1.0", 64, 64, 256, 256, 1), ("l2.0", 128, 256, 512, 128, 2), ("l3.0", 256, 512, 1024, 64, 2), ("l4.0", 512, 1024, 2048, 32, 2)]
HBM, MATRIX = 6.29e12, 2.5e15 / 6
RING_BYTES = 320 << 20


def _bn(c, dev):
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c) + 0.5); bn.bias.copy_(torch.randn(c) * 0.3)
        bn.running_mean.copy_(torch.randn(c) * 0.5); bn.running_var.copy_(torch.rand(c) + 0.3)
    return bn.to(dev).eval()


def time_shape(dev, cin, cin2, cout, side, stride, calls, rounds, batch=1):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act, conv1x1_bn_act_dual
    conv = torch.nn.Conv2d(cin, cout, 1, bias=False).to(dev).eval()
    ds = torch.nn.Conv2d(cin2, cout, 1, stride=stride, bias=False).to(dev).eval()
    bn, bnd = _bn(cout, dev), _bn(cout, dev)
    side2 = side * stride
    per_set = (cin * side * side + cin2 * side2 * side2 + cout * side * side) * 4 * batch       # x, all of x2, y
    nbuf = max(3, -(-RING_BYTES // per_set))
    xs = [torch.randn(batch, cin, side, side, device=dev) for _ in range(nbuf)]
    x2s = [torch.randn(batch, cin2, side2, side2, device=dev) for _ in range(nbuf)]
    outs = [None] * nbuf
    n = max(20, calls, 2 * nbuf)

    def pair(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = conv1x1_bn_act(xs[i % nbuf], conv, bn, residual=ds(x2s[i % nbuf]).contiguous(), residual_bn=bnd, relu=True,
                                        pieces=True)

    def dual(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = conv1x1_bn_act_dual(xs[i % nbuf], conv, bn, x2s[i % nbuf], ds, bnd, relu=True)

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

    t = {"pair": [], "dual": []}
    with torch.no_grad():
        for _ in range(rounds):
            t["pair"].append(run(pair))
            t["dual"].append(run(dual))
    return t, nbuf, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024, help="image side (a multiple of 32): the maps scale with it")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bottleneck_dual.py needs a GPU")
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act_dual_tile
    dev = torch.device("cuda:0")
    for name, cin, cin2, cout, side, stride in SHAPES:
        side = side * args.size // 1024
        hw = side * side
        t, nbuf, n = time_shape(dev, cin, cin2, cout, side, stride, args.calls, args.rounds, args.batch)
        # what the dual launch has to move: x, y, and of x2 the cache lines of every stride-th row (all of them: half of each is used)
        nbytes = (cin * hw + cout * hw + cin2 * hw * stride) * 4 * args.batch
        flop = 2.0 * (cin + cin2) * cout * hw * args.batch
        floor_mem, floor_mat = nbytes / HBM * 1e6, flop / MATRIX * 1e6
        row = dict(name=name, cin=cin, cin2=cin2, cout=cout, hw=hw, stride=stride, batch=args.batch, buffers=nbuf, calls=n,
                   tile=conv1x1_bn_act_dual_tile(cin, cin2, cout, hw, args.batch),
                   pair_us=[round(v, 2) for v in t["pair"]], dual_us=[round(v, 2) for v in t["dual"]], bytes=nbytes,
                   hbm_floor_us=round(floor_mem, 2), matrix_floor_us=round(floor_mat, 2),
                   binds="HBM" if floor_mem >= floor_mat else "matrix",
                   dual_tflops=round(flop / (max(t["dual"]) * 1e-6) / 1e12, 1),
                   pays=max(t["dual"]) < min(t["pair"]))
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
