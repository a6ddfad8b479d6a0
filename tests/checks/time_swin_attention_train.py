"""Per-block timing of the fused Swin window attention in TRAINING (`orp_window_attention_train` / `orp_window_attention_backward`,
switch ORP_SWIN_ATTN_TRAIN_FUSE) against the stock route: forward + backward of one SwinBlock of every Swin-T stage at a 1024^2 image
(256^2 / 128^2 / 64^2 / 32^2 tokens, 96 / 192 / 384 / 768 channels, 3 / 6 / 12 / 24 heads), un-shifted and shifted, batch 1, fp32, train
mode, gradients for the input and every parameter.

    python tests/checks/time_swin_attention_train.py [--out FILE.jsonl] [--calls 20] [--rounds 3] [--size 1024] [--step-timeout 120]

Each (stage, shift) is a STEP: a fresh child process of this script (`--step STAGE,SHIFT`) under its own time limit; the parent stops at
the first step that fails or runs out of time and starts nothing after it.  A step times both sides with HIP events around `calls`
eager forward + backward passes (autograd's backward is not captured here, so at the small stages the figure is the host's launch
rate on both sides), cycling through enough distinct inputs (more than 320 MiB in total: beyond the Infinity Cache) that no call finds
its input in a cache; the sides alternate `rounds` times after one dropped round.  It also records `torch.cuda.max_memory_allocated`
over one forward + backward of each side, less what was allocated before it.  Prints (and with --out appends) one JSON line per step:
the raw times per call in microseconds and the peak bytes, both sides."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

STAGES = [(96, 3), (192, 6), (384, 12), (768, 24)]          # (channels, heads) of Swin-T; the map halves per stage from size / 4
RING_BYTES = 320 << 20


def run_step(stage, shift, size, calls, rounds):
    import torch
    from orientedreppoints_amd.mmdet_models.swin import SwinStage
    dev = torch.device('cuda', 0)
    C, heads = STAGES[stage]
    side = size // 4 >> stage
    torch.manual_seed(0)
    st = SwinStage(C, 2, heads, 7, 4., True, None, 0., 0., [0., 0.], False, False).to(dev).train()
    blk = st.blocks[1 if shift else 0]
    nbuf = max(3, -(-RING_BYTES // (side * side * C * 4)))
    xs = [torch.randn(1, side * side, C, device=dev).requires_grad_() for _ in range(nbuf)]
    w = torch.randn(1, side * side, C, device=dev)
    n = max(calls, nbuf)
    mask = st.shift_mask(side, side, dev)
    params = list(blk.parameters())

    def once(x):
        torch.autograd.grad((blk(x, side, side, mask) * w).sum(), [x] + params)

    def select(on):
        blk.fuse_window_attention_train = on
        assert blk.fuses_attention_train(xs[0]) == on and not blk.fuses_attention(xs[0])
    times, peak = {'stock': [], 'fused': []}, {}
    for name, on in (('stock', False), ('fused', True)):
        select(on)
        once(xs[0])                                            # first launches load code objects, libraries pick algorithms
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        once(xs[1])
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated(dev) - before
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds + 1):                                # the first round warms up and is dropped
        for name, on in (('stock', False), ('fused', True)):
            select(on)
            e0.record()
            for i in range(n):
                once(xs[i % nbuf])
            e1.record()
            torch.cuda.synchronize()
            times[name].append(round(e0.elapsed_time(e1) * 1e3 / n, 2))
    return {'stage': stage, 'channels': C, 'heads': heads, 'tokens': side * side, 'shift': 3 if shift else 0, 'calls': n,
            'stock_us': times['stock'][1:], 'fused_us': times['fused'][1:], 'stock_peak_bytes': peak['stock'], 'fused_peak_bytes': peak['fused']}


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
