"""Per-plane timing of the backbone's fused BatchNorm passes in TRAINING (`bn_act_train`: `orp_affine_act` / `orp_affine2_act` forward,
`orp_affine_act_backward` / `orp_affine2_act_backward` backward; switch ORP_BN_TRAIN_FUSE) against the stock route: forward + backward
of the span behind one convolution output -- eval-mode BatchNorm with trainable weight / bias (+ residual | + BatchNorm of the raw
downsample output) + ReLU -- at the R-50 planes of two 1024^2 images, gradients for the input(s) and the BatchNorm parameters.

    python tests/checks/time_bn_train.py [--out FILE.jsonl] [--calls 20] [--rounds 3] [--batch 2] [--step-timeout 120]

Each plane is a STEP: a fresh child process of this script (`--step CHANNELS,SIDE`) under its own time limit; the parent stops at the
first step that fails or runs out of time and starts nothing after it.  A step times each form (no residual, residual, and at the
stage-output planes the downsample form) as time_stem.py does: HIP events around ONE captured graph of `calls` forward + backward passes
after a warm-up pass, cycling through enough distinct buffers (more than 320 MiB in total: beyond the Infinity Cache) that no call finds
its tensors in a cache; the sides alternate `rounds` times after one dropped round.  Prints (and with --out appends) one JSON line per
(plane, form): the times per call in microseconds on both sides, the bytes the span must move -- forward: read x (+ r), write y;
backward: read grad_y, y, x (+ x2), write grad_x (+ g | grad_x2) -- the floor at 6.3 TB/s and the achieved bytes/s of the new route."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# (channels, side) behind conv1 / conv2 and behind conv3 of every R-50 stage at a 1024^2 image
PLANES = [(64, 256), (256, 256), (128, 128), (512, 128), (256, 64), (1024, 64), (512, 32), (2048, 32)]
STAGE_OUTPUTS = (256, 512, 1024, 2048)          # the planes that also end a stage's first block (downsample form)
HBM_BYTES_PER_S = 6.3e12
RING_BYTES = 320 << 20


def _bn(c, dev):
    import torch
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c) + 0.5); bn.bias.copy_(torch.randn(c) * 0.3)
        bn.running_mean.copy_(torch.randn(c) * 0.5); bn.running_var.copy_(torch.rand(c) + 0.3)
    return bn.to(dev).eval()


def _time(fn, nbuf, n, keep):
    import torch
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
    for i in range(len(keep)):
        keep[i] = None
    return e0.elapsed_time(e1) * 1e3 / n          # us per call


def run_step(C, side, batch, calls, rounds):
    import torch
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act_train
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    plane = batch * C * side * side * 4
    nbuf = max(3, -(-RING_BYTES // (3 * plane)))
    n = max(20, calls, 2 * nbuf)
    xs = [torch.randn(batch, C, side, side, device=dev).requires_grad_() for _ in range(nbuf)]
    rs = [torch.randn(batch, C, side, side, device=dev).requires_grad_() for _ in range(nbuf)]
    gys = [torch.randn(batch, C, side, side, device=dev) for _ in range(nbuf)]
    bn, bn2 = _bn(C, dev), _bn(C, dev)
    relu = torch.nn.ReLU(inplace=True)
    keep = [None] * nbuf                  # the last nbuf results stay alive: the allocator hands out nbuf distinct blocks in turn
    rows = []
    for form in ('none', 'residual') + (('downsample',) if C in STAGE_OUTPUTS else ()):
        params = list(bn.parameters()) + (list(bn2.parameters()) if form == 'downsample' else [])

        def leaves(i):
            return [xs[i % nbuf]] + ([rs[i % nbuf]] if form != 'none' else []) + params

        def stock(i):
            out = bn(xs[i % nbuf])
            if form == 'residual':
                out += rs[i % nbuf]
            elif form == 'downsample':
                out += bn2(rs[i % nbuf])
            keep[i % nbuf] = None
            keep[i % nbuf] = torch.autograd.grad(relu(out), leaves(i), gys[i % nbuf])

        def fused(i):
            r = rs[i % nbuf] if form != 'none' else None
            y = bn_act_train(xs[i % nbuf], bn, residual=r, relu=True, residual_bn=bn2 if form == 'downsample' else None)
            keep[i % nbuf] = None
            keep[i % nbuf] = torch.autograd.grad(y, leaves(i), gys[i % nbuf])

        times = {'stock': [], 'fused': []}
        for _ in range(rounds + 1):                                # the first round warms up and is dropped
            for name, fn in (('stock', stock), ('fused', fused)):
                times[name].append(round(_time(fn, nbuf, n, keep), 2))
        has_res = form != 'none'
        nbytes = plane * ((2 + has_res) + (4 + has_res + (form == 'downsample')))
        floor_us = nbytes / HBM_BYTES_PER_S * 1e6
        best = min(times['fused'][1:])
        rows.append({'channels': C, 'side': side, 'batch': batch, 'form': form, 'buffers': nbuf, 'calls': n,
                     'stock_us': times['stock'][1:], 'fused_us': times['fused'][1:], 'bytes': nbytes, 'floor_us': round(floor_us, 2),
                     'fused_TBps': round(nbytes / (best * 1e-6) / 1e12, 2), 'x_floor': round(best / floor_us, 2),
                     'speedup': round(min(times['stock'][1:]) / max(times['fused'][1:]), 2)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--step-timeout', type=int, default=120)
    ap.add_argument('--step')
    args = ap.parse_args()
    if args.step:
        C, side = (int(v) for v in args.step.split(','))
        for row in run_step(C, side, args.batch, args.calls, args.rounds):
            print(json.dumps(row))
        return 0
    for C, side in PLANES:
        cmd = [sys.executable, os.path.abspath(__file__), '--step', '%d,%d' % (C, side), '--calls', str(args.calls),
               '--rounds', str(args.rounds), '--batch', str(args.batch)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print('step %d,%d ran out of time: stopping' % (C, side))
            return 124
        if r.returncode != 0:
            print('step %d,%d failed with status %d: stopping' % (C, side, r.returncode))
            return r.returncode
        for line in [l for l in r.stdout.strip().splitlines() if l.startswith('{')]:
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as f:
                    f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
