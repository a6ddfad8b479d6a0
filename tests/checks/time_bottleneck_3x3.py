"""Per-shape timing behind the routing rules of the fused conv2 kernels (`orp_conv3x3_bn_act_pays`, `orp_conv3x3_bn_deep_pays`,
`orp_conv3x3_bn_s2_pays`): library convolution + bn_act against the kernel's forced launch at its R-50 conv2 shapes.

    python tests/checks/time_bottleneck_3x3.py [--kernel act|deep|s2] [--out FILE] [--calls 20] [--rounds 2] [--batch 1] [--size 1024]
                                               [--eager 0|1]

--kernel is a kind of `fused_norm.CONV3X3_KERNELS` (default act); KERNELS below has its shapes, how it is timed by default and what its
rows hold:
  act   stride 1, 64 / 128 / 256 channels (stages 1 - 3).  An eager loop of calls; --out FILE.json is written once, as a list
        (docs/notebook/round15.md).  Floors at 6.29 TB/s over x + y and at the fp16 matrix rate under the power cap (three products per
        FLOP pair at 1.33 PFLOP/s).
  deep  512 channels: stride 2 on the 64^2 map (stage 4 block 0), stride 1 on the 32^2 map (blocks 1 and 2).  ONE captured graph of the
        calls, as time_bottleneck_1x1_pieces.py (--eager 1: an eager loop, which times the host); --out FILE.jsonl is appended to
        (docs/notebook/round23.md).  The matrix floor as above and the weight-stream figure of the kernel's layout (every workgroup
        reads its 128 output channels' planes once, 64 B/clk per CU at 2.4 GHz; workgroups beyond the 256 CUs queue behind the first wave).
  s2    stride 2: 128 channels on the 256^2 map (stage 2 block 0), 256 on the 128^2 map (stage 3 block 0).  Timed and written as deep
        (docs/notebook/round24.md).  The matrix floor at 2.5 PFLOP/s, the memory floor (input + output + packed weights once at 8 TB/s)
        and which of the two bounds the launch.

Each side: HIP events around `calls` calls (at least 20) after a warm-up pass, cycling through enough distinct input / output buffers
(more than 320 MiB in total: beyond the Infinity Cache) that no call finds its operands or its own previous output in a cache; the
sides alternate `rounds` times.  Run it at the corners the project uses (--size 1024, --size 1024 --batch 2, --size 1536), as two
processes, and route a shape only where the SLOWEST new figure of all rounds, plus what the range word costs its producer, beats the
FASTEST library figure.  The producer rows time conv1 (`conv1x1_bn_act`, on whichever path its own routing gives it at that shape) with
and without `want_range`: the fill launch and the range epilogue or range pass are the price of the new conv2 and are charged to it
(`range_cost_us` = the largest difference seen, at least 0).  Prints one JSON line per shape; FLOP are fp32-equivalent: 2 x output
positions x C x C x 9.

(time_bottleneck_3x3_deep.py and time_bottleneck_3x3_s2.py, which the notebooks of rounds 23 and 24 name, are --kernel deep / s2 here.)"""
import argparse
import functools
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

RING_BYTES = 320 << 20
CU_BYTES_PER_S, CUS = 64 * 2.4e9, 256


def _act_row(c, so, batch, nbytes, flop, t_new):
    floor_mem, floor_mat = nbytes / 6.29e12 * 1e6, flop / (1.33e15 / 3) * 1e6
    return dict(hbm_floor_us=round(floor_mem, 2), matrix_floor_us=round(floor_mat, 2), binds="HBM" if floor_mem >= floor_mat else "matrix")


def _deep_row(c, so, batch, nbytes, flop, t_new):
    wgs = -(-so // 2) * -(-so // 16) * batch * 4
    stream_us = -(-wgs // CUS) * (128 * 9 * c * 4) / CU_BYTES_PER_S * 1e6
    return dict(workgroups=wgs, matrix_floor_us=round(flop / (1.33e15 / 3) * 1e6, 2), weight_stream_us=round(stream_us, 2))


def _s2_row(c, so, batch, nbytes, flop, t_new):
    matrix_us, memory_us = flop / (2.5e15 / 3) * 1e6, (nbytes + 4 * 9 * c * c) / 8.0e12 * 1e6
    return dict(workgroups=-(-so // 2) * -(-so // 16) * batch * (c // 128), matrix_floor_us=round(matrix_us, 2),
                memory_floor_us=round(memory_us, 2), bound_by="memory" if memory_us > matrix_us else "matrix",
                x_matrix_floor=round(max(t_new) / matrix_us, 2), x_memory_floor=round(max(t_new) / memory_us, 2))


# per kind: shapes = (name, channels, stride, INPUT H = W at a 1024^2 image, conv1's input channels, calls per image); label = what the
# new side's fields are called; eager / out_list = its defaults (above); row = its own figures; fields = what a line holds, in order
KERNELS = {
    "act": dict(shapes=[("l1 conv2", 64, 1, 256, 256, 3), ("l2 conv2", 128, 1, 128, 512, 3), ("l3 conv2", 256, 1, 64, 1024, 5)],
                label="fused", eager=1, out_list=True, row=_act_row,
                fields="name channels height width batch calls_per_image buffers calls lib_us fused_us conv1_us conv1_range_us "
                       "range_cost_us bytes hbm_floor_us matrix_floor_us binds fused_tflops pays"),
    "deep": dict(shapes=[("l4.0 conv2", 512, 2, 64, 1024, 1), ("l4.x conv2", 512, 1, 32, 2048, 2)],
                 label="deep", eager=0, out_list=False, row=_deep_row,
                 fields="name channels stride height width batch calls_per_image buffers calls eager lib_us deep_us conv1_us "
                        "conv1_range_us range_cost_us bytes workgroups matrix_floor_us weight_stream_us deep_tflops pays"),
    "s2": dict(shapes=[("l2.0 conv2", 128, 2, 256, 256, None), ("l3.0 conv2", 256, 2, 128, 512, None)],
               label="s2", eager=0, out_list=False, row=_s2_row,
               fields="name channels stride height width batch buffers calls eager lib_us s2_us conv1_us conv1_range_us range_cost_us "
                      "bytes workgroups matrix_floor_us memory_floor_us bound_by x_matrix_floor x_memory_floor s2_tflops pays"),
}


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


def _ring(per_set, calls):
    """(distinct buffer sets, calls) of a timed loop over sets of per_set bytes"""
    nbuf = max(3, -(-RING_BYTES // per_set))
    return nbuf, max(20, calls, 2 * nbuf)


def _alternate(first, second, nbuf, n, rounds, eager):
    """the two sides (buffer set index -> what the call leaves alive) timed in turn, `rounds` times"""
    outs = [None] * nbuf                  # the last nbuf outputs stay alive: the allocator hands out nbuf distinct blocks in turn

    def ring(side):
        def call(i):
            outs[i % nbuf] = None
            outs[i % nbuf] = side(i % nbuf)
        return call
    t_first, t_second = [], []
    with torch.no_grad():
        for _ in range(rounds):
            t_first.append(_run(ring(first), nbuf, n, outs, eager))
            t_second.append(_run(ring(second), nbuf, n, outs, eager))
    return t_first, t_second


def time_shape(dev, launch, c, stride, side, calls, rounds, batch, eager):
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act
    conv = torch.nn.Conv2d(c, c, 3, stride=stride, padding=1, bias=False).to(dev).eval()
    bn = _bn(c, dev)
    so = (side - 1) // stride + 1
    per_set = c * (side * side + so * so) * 4 * batch
    nbuf, n = _ring(per_set, calls)
    xs = [torch.relu(torch.randn(batch, c, side, side, device=dev)) for _ in range(nbuf)]
    bits = [x.max().reshape(1).view(torch.int32) for x in xs]
    t_lib, t_new = _alternate(lambda j: bn_act(conv(xs[j]).contiguous(), bn, relu=True),
                              lambda j: launch(xs[j], conv, bn, relu=True, force=True, range_bits=bits[j]), nbuf, n, rounds, eager)
    return t_lib, t_new, per_set, nbuf, n


def time_producer(dev, cin, c, side, calls, rounds, batch, eager):
    from orientedreppoints_amd.mmdet_ops.fused_norm import conv1x1_bn_act
    conv = torch.nn.Conv2d(cin, c, 1, bias=False).to(dev).eval()
    bn = _bn(c, dev)
    nbuf, n = _ring((cin + c) * side * side * 4 * batch, calls)
    xs = [torch.randn(batch, cin, side, side, device=dev) for _ in range(nbuf)]
    return _alternate(lambda j: conv1x1_bn_act(xs[j], conv, bn, relu=True),
                      lambda j: conv1x1_bn_act(xs[j], conv, bn, relu=True, want_range=True)[0], nbuf, n, rounds, eager)


def main():
    from orientedreppoints_amd.mmdet_ops import fused_norm
    kinds = [k.kind for k in fused_norm.CONV3X3_KERNELS]
    assert sorted(kinds) == sorted(KERNELS), "a kernel of fused_norm.CONV3X3_KERNELS has no shapes here"
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", choices=kinds, default="act")
    ap.add_argument("--out", default=None, help="act: written as one JSON list; deep / s2: the JSON lines are appended to this file")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--size", type=int, default=1024, help="image side (a multiple of 32): the maps scale with it")
    ap.add_argument("--eager", type=int, default=None,
                    help="1: time an eager loop of calls, 0: a captured graph of them (default: 1 for act, 0 for deep / s2)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_bottleneck_3x3.py needs a GPU")
    dev = torch.device("cuda:0")
    K = KERNELS[args.kernel]
    eager = bool(K["eager"] if args.eager is None else args.eager)
    launch = functools.partial(fused_norm._conv3x3_launch, args.kernel)
    rows = []
    for name, c, stride, side, cin1, per_image in K["shapes"]:
        side = side * args.size // 1024
        t_lib, t_new, nbytes, nbuf, n = time_shape(dev, launch, c, stride, side, args.calls, args.rounds, args.batch, eager)
        t_plain, t_ranged = time_producer(dev, cin1, c, side, args.calls, args.rounds, args.batch, eager)
        range_cost = max(0.0, max(t_ranged) - min(t_plain))
        so = (side - 1) // stride + 1
        flop = 2.0 * 9 * c * c * so * so * args.batch
        row = dict(name=name, channels=c, stride=stride, height=side, width=side, batch=args.batch, calls_per_image=per_image,
                   buffers=nbuf, calls=n, eager=eager, lib_us=[round(t, 2) for t in t_lib], conv1_us=[round(t, 2) for t in t_plain],
                   conv1_range_us=[round(t, 2) for t in t_ranged], range_cost_us=round(range_cost, 2), bytes=nbytes,
                   pays=max(t_new) + range_cost < min(t_lib), **K["row"](c, so, args.batch, nbytes, flop, t_new))
        row[K["label"] + "_us"] = [round(t, 2) for t in t_new]
        row[K["label"] + "_tflops"] = round(flop / (max(t_new) * 1e-6) / 1e12, 1)
        row = {f: row[f] for f in K["fields"].split()}
        rows.append(row)
        line = json.dumps(row)
        print(line, flush=True)
        if args.out and not K["out_list"]:
            with open(args.out, "a") as f:
                f.write(line + "\n")
    if args.out and K["out_list"]:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
