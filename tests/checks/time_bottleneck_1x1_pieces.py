"""Per-shape timing behind the routing rule of `orp_conv1x1_bn_act_pieces_pays`: three sides at the conv1 / conv3 shapes of R-50 --
library convolution + bn_act, the fp32 fused launch (conv1x1_bn_act(force=True)) and the bf16-pieces launch
(conv1x1_bn_act(pieces=True)).

    python tests/checks/time_bottleneck_1x1_pieces.py [--out FILE.jsonl] [--calls 20] [--rounds 2] [--batch 1] [--size 1024] [--eager 0]

Each side: HIP events around `calls` calls (at least 20) after a warm-up pass -- replayed as one captured graph, which is how the
benchmark and the captured inference path run them (an eager loop times the host: --eager 1) --, cycling through enough distinct input / residual /
output buffers (more than 320 MiB in total: beyond the Infinity Cache) that no call finds its operands or its own previous output in a
cache; the sides alternate `rounds` times.  Run it at the three corners the project uses (--size 1024, --size 1024 --batch 2,
--size 1536) and route a shape to the pieces kernel only where its SLOWEST figure of all rounds beats the FASTEST figure of either
other side (docs/notebook/round16.md).  The conv1 rows whose output feeds the fused conv2 are timed as they run there, with
want_range on all three sides.  Prints (and with --out appends) one JSON line per shape with the raw times, the bytes the launch
has to move (x + residual + y), its FLOP (fp32-equivalent) and the floors at 6.29 TB/s and at six bf16 products per FLOP pair on
2.5 PFLOP/s."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

# (name, Cin, Cout, H = W at a 1024^2 image, residual form: None | 'plain' | 'affine', leaves a range word, calls per image)
SHAPES = [
    ("l1.0 conv1", 64, 64, 256, None, True, 1), ("l1.x conv1", 256, 64, 256, None, True, 2),
    ("l1.0 conv3", 64, 256, 256, 'affine', False, 1), ("l1.x conv3", 64, 256, 256, 'plain', False, 2),
    ("l2.0 conv1", 256, 128, 256, None, False, 1), ("l2.x conv1", 512, 128, 128, None, True, 3),
    ("l2.0 conv3", 128, 512, 128, 'affine', False, 1), ("l2.x conv3", 128, 512, 128, 'plain', False, 3),
    ("l3.0 conv1", 512, 256, 128, None, False, 1), ("l3.x conv1", 1024, 256, 64, None, True, 5),
    ("l3.0 conv3", 256, 1024, 64, 'affine', False, 1), ("l3.x conv3", 256, 1024, 64, 'plain', False, 5),
    ("l4.0 conv1", 1024, 512, 64, None, False, 1), ("l4.x conv1", 2048, 512, 32, None, False, 2),
    ("l4.0 conv3", 512, 2048, 32, 'affine', False, 1), ("l4.x conv3", 512, 2048, 32, 'plain', False, 2),
]
HBM, MATRIX = 6.29e12, 2.5e15 / 6
RING_BYTES = 320 << 20


def _bn(c, dev):
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c) + 0.5); bn.bias.copy_(torch.randn(c) * 0.3)
        bn.running_mean.copy_(torch.randn(c) * 0.5); bn.running_var.copy_(torch.rand(c) + 0.3)
    return bn.to(dev).eval()


def time_shape(dev, cin, cout, hw_side, form, ranged, calls, rounds, batch=1, eager=False):
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
        outs[i % nbuf] = bn_act(conv(xs[i % nbuf]).contiguous(), bn, residual=rs[i % nbuf], residual_bn=bnd, relu=True, want_range=ranged)

    def fp32(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = conv1x1_bn_act(xs[i % nbuf], conv, bn, residual=rs[i % nbuf], residual_bn=bnd, relu=True, force=True,
                                        want_range=ranged)

    def pieces(i):
        outs[i % nbuf] = None
        outs[i % nbuf] = conv1x1_bn_act(xs[i % nbuf], conv, bn, residual=rs[i % nbuf], residual_bn=bnd, relu=True, pieces=True,
                                        want_range=ranged)

    def run(fn):
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
            # the n calls as ONE captured graph, as the benchmark runs them: the fused launches take less than the host needs to
            # issue one, and an eager loop would time the host
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

    t = {"lib": [], "fp32": [], "pieces": []}
    with torch.no_grad():
        for _ in range(rounds):
            t["lib"].append(run(lib))
            t["fp32"].append(run(fp32))
            t["pieces"].append(run(pieces))
    return t, per_set, nbuf, n


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
        raise SystemExit("time_bottleneck_1x1_pieces.py needs a GPU")
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act_pieces_tile
    dev = torch.device("cuda:0")
    for name, cin, cout, side, form, ranged, per_image in SHAPES:
        side = side * args.size // 1024
        t, nbytes, nbuf, n = time_shape(dev, cin, cout, side, form, ranged, args.calls, args.rounds, args.batch, bool(args.eager))
        flop = 2.0 * cin * cout * side * side * args.batch
        floor_mem, floor_mat = nbytes / HBM * 1e6, flop / MATRIX * 1e6
        row = dict(name=name, cin=cin, cout=cout, hw=side * side, batch=args.batch, residual=form, range_word=ranged,
                   calls_per_image=per_image, buffers=nbuf, calls=n, eager=bool(args.eager), tile=conv1x1_bn_act_pieces_tile(cin, cout, side * side, args.batch),
                   lib_us=[round(v, 2) for v in t["lib"]], fp32_us=[round(v, 2) for v in t["fp32"]],
                   pieces_us=[round(v, 2) for v in t["pieces"]], bytes=nbytes,
                   hbm_floor_us=round(floor_mem, 2), matrix_floor_us=round(floor_mat, 2),
                   binds="HBM" if floor_mem >= floor_mat else "matrix",
                   pieces_gbs=round(nbytes / (max(t["pieces"]) * 1e-6) / 1e9, 1),
                   pieces_tflops=round(flop / (max(t["pieces"]) * 1e-6) / 1e12, 1),
                   pays=max(t["pieces"]) < min(min(t["lib"]), min(t["fp32"])))
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
