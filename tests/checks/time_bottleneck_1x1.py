"""Per-shape timing behind the routing rule of `orp_conv1x1_bn_act_pays`: library convolution + bn_act against the fused launch
(conv1x1_bn_act(force=True)) at the conv1 / conv3 shapes of R-50 at 1024 x 1024, B = 1.

    python tests/checks/time_bottleneck_1x1.py [--out FILE.json] [--calls 20] [--rounds 2] [--batch 1] [--size 1024]

Each side: HIP events around `calls` calls (at least 20) after a warm-up pass, cycling through enough distinct input / residual /
output buffers (more than 256 MiB in total, the Infinity Cache) that no call finds its operands or its own previous output in a cache;
the sides alternate `rounds` times.  Run it as two processes and route a shape to the fused kernel only where the SLOWEST fused figure of
all rounds beats the FASTEST library figure (docs/notebook/round12.md).  Prints one JSON line per shape with the times, the bytes the
fused launch has to move (x + residual + y) and its FLOP, against the floors 6.29 TB/s and 155 TFLOP/s."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

# (name, Cin, Cout, H = W, residual form: None | 'plain' | 'affine', calls per image)
SHAPES = [
    ("l1.0 conv1", 64, 64, 256, None, 1), ("l1.x conv1", 256, 64, 256, None, 2),
    ("l1.0 conv3", 64, 256, 256, 'affine', 1), ("l1.x conv3", 64, 256, 256, 'plain', 2),
    ("l2.0 conv1", 256, 128, 256, None, 1), ("l2.x conv1", 512, 128, 128, None, 3),
    ("l2.0 conv3", 128, 512, 128, 'affine', 1), ("l2.x conv3", 128, 512, 128, 'plain', 3),
    ("l3.0 conv1", 512, 256, 128, None, 1), ("l3.x conv1", 1024, 256, 64, None, 5),
    ("l3.0 conv3", 256, 1024, 64, 'affine', 1), ("l3.x conv3", 256, 1024, 64, 'plain', 5),
    ("l4.0 conv1", 1024, 512, 64, None, 1), ("l4.x conv1", 2048, 512, 32, None, 2),
    ("l4.0 conv3", 512, 2048, 32, 'affine', 1), ("l4.x conv3", 512, 2048, 32, 'plain', 2),
]
HBM, MATRIX = 6.29e12, 155e12
RING_BYTES = 320 << 20


def _bn(c, dev):
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c) + 0.5); bn.bias.copy_(torch.randn(c) * 0.3)
        bn.running_mean.copy_(torch.randn(c) * 0.5); bn.running_var.copy_(torch.rand(c) + 0.3)
    return bn.to(dev).eval()


def time_shape(dev, cin, cout, hw_side, form, calls, rounds, batch=1):
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act, conv1x1_bn_act
    hw = hw_side * hw_side
    conv = torch.nn.Conv2d(cin, cout, 1, bias=False).to(dev).eval()
    bn, bnd = _bn(cout, dev), (_bn(cout, dev) if form == 'affine' else None)
    per_set = (cin + (2 if form else 1) * cout) * hw * 4 * batch
    nbuf = max(3, -(-RING_BYTES // per_set))
    xs = [torch.randn(batch, cin, hw_side, hw_side, device=dev) for _ in range(nbuf)]
    rs = [torch.randn(batch, cout, hw_side, hw_side, device=dev) if form else None for _ in range(nbuf)]
    outs = [None] * nbuf                  # the last nbuf outputs stay alive: the allocator hands out nbuf distinct blocks in turn
    n = max(20, calls, 2 * nbuf)

    def lib(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = bn_act(conv(xs[i % nbuf]).contiguous(), bn, residual=rs[i % nbuf], residual_bn=bnd, relu=True)

    def fused(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = conv1x1_bn_act(xs[i % nbuf], conv, bn, residual=rs[i % nbuf], residual_bn=bnd, relu=True, force=True)

    def run(fn):
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

    t_lib, t_fused = [], []
    with torch.no_grad():
        for _ in range(rounds):
            t_lib.append(run(lib))
            t_fused.append(run(fused))
    return t_lib, t_fused, per_set, nbuf, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024, help="image side (a multiple of 32): the maps scale with it")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bottleneck_1x1.py needs a GPU")
    dev = torch.device("cuda:0")
    rows = []
    for name, cin, cout, side, form, per_image in SHAPES:
        side = side * args.size // 1024
        t_lib, t_fused, nbytes, nbuf, n = time_shape(dev, cin, cout, side, form, args.calls, args.rounds, args.batch)
        flop = 2.0 * cin * cout * side * side * args.batch
        floor_mem, floor_mat = nbytes / HBM * 1e6, flop / MATRIX * 1e6
        row = dict(name=name, cin=cin, cout=cout, hw=side * side, batch=args.batch, residual=form, calls_per_image=per_image, buffers=nbuf, calls=n,
                   lib_us=[round(t, 2) for t in t_lib], fused_us=[round(t, 2) for t in t_fused], bytes=nbytes,
                   hbm_floor_us=round(floor_mem, 2), matrix_floor_us=round(floor_mat, 2),
                   binds="HBM" if floor_mem >= floor_mat else "matrix",
                   fused_gbs=round(nbytes / (max(t_fused) * 1e-6) / 1e9, 1), fused_tflops=round(flop / (max(t_fused) * 1e-6) / 1e12, 1),
                   pays=max(t_fused) < min(t_lib))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
