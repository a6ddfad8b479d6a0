"""Per-corner timing behind the routing rule of `orp_stem_pays`: library 7x7 convolution + bn_relu_maxpool (two launches, the raw map
written and read back) against the one launch of `stem_conv_bn_relu_maxpool` at the R-50 stem.

    python tests/checks/time_stem.py [--out FILE.jsonl] [--calls 20] [--rounds 2] [--batch 1] [--size 1024]

Each side as time_bottleneck_3x3.py --kernel s2 times it: HIP events around ONE captured graph of `calls` calls (at least 20) after a warm-up pass,
cycling through enough distinct input / output buffers (more than 320 MiB in total) that no call finds its image in a cache; the sides
alternate `rounds` times.  Run it twice (two processes) at each corner the project uses (--size 1024, --size 1024 --batch 2, --size 1536)
and route a corner only where the SLOWEST new figure of all rounds beats the FASTEST library figure.  Prints (and with --out appends)
one JSON line with the times, the FLOP (2 x conv positions x 64 x 147), the matrix floor (exact fp32 MFMA, 157 TFLOP/s), the memory floor
(image in, pooled map out, at 6.3 TB/s) and the launch's time as a multiple of both."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

MATRIX = 157.0e12
HBM_BYTES_PER_S = 6.3e12
RING_BYTES = 320 << 20


def _bn(c, dev):
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c) + 0.5); bn.bias.copy_(torch.randn(c) * 0.3)
        bn.running_mean.copy_(torch.randn(c) * 0.5); bn.running_var.copy_(torch.rand(c) + 0.3)
    return bn.to(dev).eval()


def _run(fn, nbuf, n, outs):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the JSON line to this file")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024, help="image side")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_stem.py needs a GPU")
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_relu_maxpool, stem_conv_bn_relu_maxpool
    dev = torch.device("cuda:0")
    side, batch = args.size, args.batch
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).to(dev).eval()
    bn = _bn(64, dev)
    so = (side - 1) // 2 + 1
    sp = (so - 1) // 2 + 1
    needed = (3 * side * side + 64 * sp * sp) * 4 * batch                 # what the result needs: image in, pooled map out
    nbuf = max(3, -(-RING_BYTES // needed))
    xs = [torch.randn(batch, 3, side, side, device=dev) for _ in range(nbuf)]
    outs = [None] * nbuf                  # the last nbuf outputs stay alive: the allocator hands out nbuf distinct blocks in turn
    n = max(20, args.calls, 2 * nbuf)

    def lib(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = bn_relu_maxpool(conv(xs[i % nbuf]).contiguous(), bn)

    def new(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = stem_conv_bn_relu_maxpool(xs[i % nbuf], conv, bn)

    t_lib, t_new = [], []
    with torch.no_grad():
        for _ in range(args.rounds):
            t_lib.append(_run(lib, nbuf, n, outs))
            t_new.append(_run(new, nbuf, n, outs))
    flop = 2.0 * 147 * 64 * so * so * batch
    matrix_us = flop / MATRIX * 1e6
    memory_us = needed / HBM_BYTES_PER_S * 1e6
    row = dict(name="stem", height=side, width=side, batch=batch, buffers=nbuf, calls=n, lib_us=[round(t, 2) for t in t_lib],
               stem_us=[round(t, 2) for t in t_new], bytes=needed, workgroups=-(-sp // 4) * -(-sp // 16) * batch,
               matrix_floor_us=round(matrix_us, 2), memory_floor_us=round(memory_us, 2),
               bound_by="memory" if memory_us > matrix_us else "matrix", x_matrix_floor=round(max(t_new) / matrix_us, 2),
               x_memory_floor=round(max(t_new) / memory_us, 2), stem_tflops=round(flop / (max(t_new) * 1e-6) / 1e12, 1),
               pays=max(t_new) < min(t_lib))
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
