"""Per-shape timing behind the routing rule of `orp_conv3x3_bn_s2_pays`: library convolution + bn_act against the narrow-pass fp16-pieces
launch (conv3x3_bn_s2(force=True)) at the stride-2 conv2 shapes of R-50: 128 channels on the 256^2 map (stage 2 block 0) and 256
channels on the 128^2 map (stage 3 block 0).

    python tests/checks/time_bottleneck_3x3_s2.py [--out FILE.jsonl] [--calls 20] [--rounds 2] [--batch 1] [--size 1024] [--eager 0]

Each side as time_bottleneck_3x3_deep.py times it: HIP events around ONE captured graph of `calls` calls (at least 20; an eager loop
times the host: --eager 1) after a warm-up pass, cycling through enough distinct input / output buffers (more than 320 MiB in total)
that no call finds its activations in a cache; the sides alternate `rounds` times.  Run it at the corners the project uses (--size 1024,
--size 1024 --batch 2, --size 1536) and route a shape only where the SLOWEST new figure of all rounds, plus what the range word costs
its producer, beats the FASTEST library figure.  The producer rows time conv1 (`conv1x1_bn_act`, on whichever path its own routing
gives it at that shape) with and without `want_range`: the fill launch and the range epilogue or range pass are the price of the
new conv2 and are charged to it (`range_cost_us` = the largest difference seen, at least 0).  Prints (and with --out appends) one JSON
line per shape with the times, its FLOP (fp32-equivalent: 2 x output positions x C x C x 9), the matrix floor (three fp16 products per
FLOP pair at 2.5 PFLOP/s), the memory floor (input + output + packed weights once at 8 TB/s) and which of the two bounds the launch."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

# (name, channels, INPUT H = W at a 1024^2 image, conv1's input channels)
SHAPES = [("l2.0 conv2", 128, 256, 256), ("l3.0 conv2", 256, 128, 512)]
MATRIX = 2.5e15 / 3
HBM_BYTES_PER_S = 8.0e12
RING_BYTES = 320 << 20


def _bn(c, dev):
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c) + 0.5); bn.bias.copy_(torch.randn(c) * 0.3)
        bn.running_mean.copy_(torch.randn(c) * 0.5); bn.running_var.copy_(torch.rand(c) + 0.3)
    return bn.to(dev).eval()


def _run(fn, nbuf, n, outs, eager):
    for i in range(nbuf):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if eager:
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
    else:
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


def time_shape(dev, C, side, calls, rounds, batch, eager):
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act, conv3x3_bn_s2
    conv = torch.nn.Conv2d(C, C, 3, stride=2, padding=1, bias=False).to(dev).eval()
    bn = _bn(C, dev)
    so = (side - 1) // 2 + 1
    per_set = C * (side * side + so * so) * 4 * batch
    nbuf = max(3, -(-RING_BYTES // per_set))
    xs = [torch.relu(torch.randn(batch, C, side, side, device=dev)) for _ in range(nbuf)]
    bits = [x.max().reshape(1).view(torch.int32) for x in xs]
    outs = [None] * nbuf                  # the last nbuf outputs stay alive: the allocator hands out nbuf distinct blocks in turn
    n = max(20, calls, 2 * nbuf)

    def lib(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = bn_act(conv(xs[i % nbuf]).contiguous(), bn, relu=True)

    def new(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = conv3x3_bn_s2(xs[i % nbuf], conv, bn, relu=True, force=True, range_bits=bits[i % nbuf])

    t_lib, t_new = [], []
    with torch.no_grad():
        for _ in range(rounds):
            t_lib.append(_run(lib, nbuf, n, outs, eager))
            t_new.append(_run(new, nbuf, n, outs, eager))
    return t_lib, t_new, per_set, nbuf, n


def time_producer(dev, cin, C, side, calls, rounds, batch, eager):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act
    conv = torch.nn.Conv2d(cin, C, 1, bias=False).to(dev).eval()
    bn = _bn(C, dev)
    per_set = (cin + C) * side * side * 4 * batch
    nbuf = max(3, -(-RING_BYTES // per_set))
    xs = [torch.randn(batch, cin, side, side, device=dev) for _ in range(nbuf)]
    outs = [None] * nbuf
    n = max(20, calls, 2 * nbuf)

    def plain(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = conv1x1_bn_act(xs[i % nbuf], conv, bn, relu=True)

    def ranged(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = conv1x1_bn_act(xs[i % nbuf], conv, bn, relu=True, want_range=True)[0]

    t_plain, t_ranged = [], []
    with torch.no_grad():
        for _ in range(rounds):
            t_plain.append(_run(plain, nbuf, n, outs, eager))
            t_ranged.append(_run(ranged, nbuf, n, outs, eager))
    return t_plain, t_ranged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024, help="image side (a multiple of 32): the maps scale with it")
    ap.add_argument("--eager", type=int, default=0, help="1: time an eager loop of calls instead of a captured graph of them")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bottleneck_3x3_s2.py needs a GPU")
    dev = torch.device("cuda:0")
    for name, C, side, cin1 in SHAPES:
        side = side * args.size // 1024
        t_lib, t_new, nbytes, nbuf, n = time_shape(dev, C, side, args.calls, args.rounds, args.batch, bool(args.eager))
        t_plain, t_ranged = time_producer(dev, cin1, C, side, args.calls, args.rounds, args.batch, bool(args.eager))
        range_cost = max(0.0, max(t_ranged) - min(t_plain))
        so = (side - 1) // 2 + 1
        flop = 2.0 * 9 * C * C * so * so * args.batch
        wgs = -(-so // 2) * -(-so // 16) * args.batch * (C // 128)
        matrix_us = flop / MATRIX * 1e6
        memory_us = (nbytes + 4 * 9 * C * C) / HBM_BYTES_PER_S * 1e6
        row = dict(name=name, channels=C, stride=2, height=side, width=side, batch=args.batch,
                   buffers=nbuf, calls=n, eager=bool(args.eager), lib_us=[round(t, 2) for t in t_lib],
                   s2_us=[round(t, 2) for t in t_new], conv1_us=[round(t, 2) for t in t_plain],
                   conv1_range_us=[round(t, 2) for t in t_ranged], range_cost_us=round(range_cost, 2), bytes=nbytes,
                   workgroups=wgs, matrix_floor_us=round(matrix_us, 2), memory_floor_us=round(memory_us, 2),
                   bound_by="memory" if memory_us > matrix_us else "matrix",
                   x_matrix_floor=round(max(t_new) / matrix_us, 2), x_memory_floor=round(max(t_new) / memory_us, 2),
                   s2_tflops=round(flop / (max(t_new) * 1e-6) / 1e12, 1),
                   pays=max(t_new) + range_cost < min(t_lib))
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
