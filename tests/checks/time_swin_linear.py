"""Per-block timing of the Swin block linears on the bf16-pieces launch (`orp_token_linear`, switch ORP_SWIN_LINEAR_FUSE) against the
library's linears, the fused window attention on both sides: one SwinBlock of every Swin-T stage at a size^2 image, un-shifted and
shifted, batch 1, fp32, eval mode, no grad.  The method of tests/checks/time_swin_attention.py.

    python tests/checks/time_swin_linear.py [--out FILE.jsonl] [--calls 20] [--rounds 3] [--size 1024] [--step-timeout 120]

Three sides: `stock` (block.fuse_token_linear = False), `routed` (the shipped rule: each linear where `orp_token_linear_pays` says so)
and `forced` (block.force_token_linear: all four).  Each (stage, shift) is a STEP: a fresh child process of this script under its own
time limit; the parent stops at the first step that fails or runs out of time and starts nothing after it.  A step times the sides with
HIP events around `calls` block forwards replayed as one captured graph, cycling through more than 320 MiB of distinct inputs; the
sides alternate `rounds` times after one dropped round.  One JSON line per step: the raw times per call in microseconds."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

STAGES = [(96, 3), (192, 6), (384, 12), (768, 24)]          # (channels, heads) of Swin-T; the map halves per stage from size / 4
RING_BYTES = 320 << 20
SIDES = (('stock', False, False), ('routed', True, False), ('forced', True, True))


def run_step(stage, shift, size, calls, rounds):
    import torch
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_models.swin import SwinStage
    dev = torch.device('cuda', 0)
    C, heads = STAGES[stage]
    side = size // 4
    for _ in range(stage):
        side = (side + 1) // 2
    torch.manual_seed(0)
    st = SwinStage(C, 2, heads, 7, 4., True, None, 0., 0., [0., 0.], False, False).to(dev).eval()
    blk = st.blocks[1 if shift else 0]
    blk.fuse_window_attention = True
    nbuf = max(3, -(-RING_BYTES // (side * side * C * 4)))
    xs = [torch.randn(1, side * side, C, device=dev) for _ in range(nbuf)]
    n = max(calls, nbuf)
    times = {name: [] for name, _, _ in SIDES}
    launches = {}
    real = _lib.lib()

    class Counting:
        count = 0

        def __getattr__(self, name):
            fn = getattr(real, name)
            if name != 'orp_token_linear':
                return fn

            def counted(*a):
                Counting.count += 1
                return fn(*a)
            return counted
    with torch.no_grad():
        graphs = {}
        for name, on, force in SIDES:
            blk.fuse_token_linear, blk.force_token_linear = on, force
            assert blk.fuses_linears(xs[0]) == on
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                _lib.lib = Counting
                Counting.count = 0
                blk(xs[0], side, side, None)
                launches[name] = Counting.count
                _lib.lib = lambda: real
            torch.cuda.current_stream().wait_stream(s)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for i in range(n):
                    blk(xs[i % nbuf], side, side, None)
            graphs[name] = g
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(rounds + 1):                            # the first round warms up and is dropped
            for name, g in graphs.items():
                e0.record()
                g.replay()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(round(e0.elapsed_time(e1) * 1e3 / n, 2))
    row = {'stage': stage, 'size': size, 'channels': C, 'heads': heads, 'tokens': side * side, 'shift': 3 if shift else 0, 'calls': n,
           'token_linear_launches': launches}
    row.update({name + '_us': v[1:] for name, v in times.items()})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--step-timeout', type=int, default=120)
    ap.add_argument('--step')
    args = ap.parse_args()
    if args.step:
        stage, shift = (int(v) for v in args.step.split(','))
        print(json.dumps(run_step(stage, shift, args.size, args.calls, args.rounds)))
        return 0
    for stage in range(len(STAGES)):
        for shift in (0, 1):
            cmd = [sys.executable, os.path.abspath(__file__), '--step', '%d,%d' % (stage, shift), '--calls', str(args.calls),
                   '--rounds', str(args.rounds), '--size', str(args.size)]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                print('step %d,%d ran out of time: stopping' % (stage, shift))
                return 124
            if r.returncode != 0:
                print('step %d,%d failed with status %d: stopping' % (stage, shift, r.returncode))
                return r.returncode
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            if args.out:
                with open(args.out, 'a') as f:
                    f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
