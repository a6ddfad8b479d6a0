"""Per-shape timing behind the routing rule of `orp_conv3x3_bn_act_pays`: library convolution + bn_act against the fused fp16-pieces
launch (conv3x3_bn_act(force=True)) at the stride-1 conv2 shapes of R-50 stages 1 - 3.

    python tests/checks/time_bottleneck_3x3.py [--out FILE.json] [--calls 20] [--rounds 2] [--batch 1] [--size 1024]

Each side: HIP events around `calls` calls (at least 20) after a warm-up pass, cycling through enough distinct input / output buffers
(more than 320 MiB in total: beyond the Infinity Cache) that no call finds its operands or its own previous output in a cache; the
sides alternate `rounds` times.  Run it as two processes and route a shape only where the SLOWEST fused figure of all rounds, plus
what the range word costs its producer, beats the FASTEST library figure (docs/notebook/round15.md).  The producer rows time conv1
(`conv1x1_bn_act`, on whichever path the routing of round 12 gives it) with and without `want_range`: the fill launch and the
epilogue's maximum are the price of the fused conv2 and are charged to it (`range_cost_us` = the largest difference seen, at least 0).
Prints one JSON line per shape with the times, the bytes the fused launch has to move (x + y), its FLOP (fp32-equivalent:
2 x positions x Cin x Cout x 9) and the floors at 6.29 TB/s and at the fp16 matrix rate under the power cap (three products per
FLOP pair at 1.33 PFLOP/s)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

# (name, channels, H = W at a 1024^2 image, conv1's input channels, calls per image)
SHAPES = [("l1 conv2", 64, 256, 256, 3), ("l2 conv2", 128, 128, 512, 3), ("l3 conv2", 256, 64, 1024, 5)]
HBM, MATRIX = 6.29e12, 1.33e15 / 3
RING_BYTES = 320 << 20


def _bn(c, dev):
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c) + 0.5); bn.bias.copy_(torch.randn(c) * 0.3)
        bn.running_mean.copy_(torch.randn(c) * 0.5); bn.running_var.copy_(torch.rand(c) + 0.3)
    return bn.to(dev).eval()


def _run(fn, nbuf, n):
    for i in range(nbuf):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n          # us per call


def time_shape(dev, c, side, calls, rounds, batch):
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act, conv3x3_bn_act
    conv = torch.nn.Conv2d(c, c, 3, padding=1, bias=False).to(dev).eval()
    bn = _bn(c, dev)
    per_set = 2 * c * side * side * 4 * batch
    nbuf = max(3, -(-RING_BYTES // per_set))
    xs = [torch.relu(torch.randn(batch, c, side, side, device=dev)) for _ in range(nbuf)]
    bits = [x.max().reshape(1).view(torch.int32) for x in xs]
    outs = [None] * nbuf                  # the last nbuf outputs stay alive: the allocator hands out nbuf distinct blocks in turn
    n = max(20, calls, 2 * nbuf)

    def lib(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = bn_act(conv(xs[i % nbuf]).contiguous(), bn, relu=True)

    def fused(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = conv3x3_bn_act(xs[i % nbuf], conv, bn, relu=True, force=True, range_bits=bits[i % nbuf])

    t_lib, t_fused = [], []
    with torch.no_grad():
        for _ in range(rounds):
            t_lib.append(_run(lib, nbuf, n))
            t_fused.append(_run(fused, nbuf, n))
    return t_lib, t_fused, per_set, nbuf, n


def time_producer(dev, cin, c, side, calls, rounds, batch):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act
    conv = torch.nn.Conv2d(cin, c, 1, bias=False).to(dev).eval()
    bn = _bn(c, dev)
    per_set = (cin + c) * side * side * 4 * batch
    nbuf = max(3, -(-RING_BYTES // per_set))
    xs = [torch.randn(batch, cin, side, side, device=dev) for _ in range(nbuf)]
    outs = [None] * nbuf
    n = max(20, calls, 2 * nbuf)

    def plain(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = conv1x1_bn_act(xs[i % nbuf], conv, bn, relu=True)

    def ranged(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = conv1x1_bn_act(xs[i % nbuf], conv, bn, relu=True, want_range=True)

    t_plain, t_ranged = [], []
    with torch.no_grad():
        for _ in range(rounds):
            t_plain.append(_run(plain, nbuf, n))
            t_ranged.append(_run(ranged, nbuf, n))
    return t_plain, t_ranged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024, help="image side (a multiple of 32): the maps scale with it")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bottleneck_3x3.py needs a GPU")
    dev = torch.device("cuda:0")
    rows = []
    for name, c, side, cin1, per_image in SHAPES:
        side = side * args.size // 1024
        t_lib, t_fused, nbytes, nbuf, n = time_shape(dev, c, side, args.calls, args.rounds, args.batch)
        t_plain, t_ranged = time_producer(dev, cin1, c, side, args.calls, args.rounds, args.batch)
        range_cost = max(0.0, max(t_ranged) - min(t_plain))
        flop = 2.0 * 9 * c * c * side * side * args.batch
        floor_mem, floor_mat = nbytes / HBM * 1e6, flop / MATRIX * 1e6
        row = dict(name=name, channels=c, height=side, width=side, batch=args.batch, calls_per_image=per_image, buffers=nbuf, calls=n,
                   lib_us=[round(t, 2) for t in t_lib], fused_us=[round(t, 2) for t in t_fused],
                   conv1_us=[round(t, 2) for t in t_plain], conv1_range_us=[round(t, 2) for t in t_ranged],
                   range_cost_us=round(range_cost, 2), bytes=nbytes, hbm_floor_us=round(floor_mem, 2),
                   matrix_floor_us=round(floor_mat, 2), binds="HBM" if floor_mem >= floor_mat else "matrix",
                   fused_tflops=round(flop / (max(t_fused) * 1e-6) / 1e12, 1),
                   pays=max(t_fused) + range_cost < min(t_lib))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
