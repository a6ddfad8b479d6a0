"""Per-block timing of the fused Swin window attention under fp16 / bf16 AUTOCAST (`orp_window_attention_h` /
`orp_window_attention_backward_h`, switch ORP_SWIN_ATTN_HALF_FUSE) against the stock autocast route: one SwinBlock of every Swin-T stage
at a 1024^2 image (256^2 / 128^2 / 64^2 / 32^2 tokens, 96 / 192 / 384 / 768 channels, 3 / 6 / 12 / 24 heads), un-shifted and shifted, batch
1, fp32 parameters, forward only (`no_grad`, eval mode) and forward + backward (train mode, gradients for the input and every parameter).

    python tests/checks/time_swin_attention_half.py [--out FILE.jsonl] [--dtype fp16] [--calls 20] [--rounds 3] [--size 1024] [--step-timeout 120]

Each (stage, shift) is a STEP: a fresh child process of this script (`--step STAGE,SHIFT`) under its own time limit; the parent stops at
the first step that fails or runs out of time and starts nothing after it.  A step times both sides of both modes with HIP events
around `calls` eager passes, cycling through enough distinct inputs (more than 320 MiB in total: beyond the Infinity Cache) that no
call finds its input in a cache; the sides alternate `rounds` times after one dropped round.  The input tokens are fp32 at stage 1 and
of the autocast dtype at the later stages, as PatchMerging's linear layer hands them over.  It also records
`torch.cuda.max_memory_allocated` over one pass of each side, less what was allocated before it.  Prints (and with --out appends) one
JSON line per step: the raw times per call in microseconds and the peak bytes, both sides, both modes."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

STAGES = [(96, 3), (192, 6), (384, 12), (768, 24)]          # (channels, heads) of Swin-T; the map halves per stage from size / 4
RING_BYTES = 320 << 20


def run_step(stage, shift, size, calls, rounds, dtype):
    import torch
    from orientedreppoints_amd.mmdet_models.swin import SwinStage
    from orientedreppoints_amd.mmdet_ops import window_attention_half, window_attention_train_half
    dev = torch.device('cuda', 0)
    dt = dict(fp16=torch.float16, bf16=torch.bfloat16)[dtype]
    xdt = torch.float32 if stage == 0 else dt
    C, heads = STAGES[stage]
    side = size // 4 >> stage
    torch.manual_seed(0)
    st = SwinStage(C, 2, heads, 7, 4., True, None, 0., 0., [0., 0.], False, False).to(dev)
    blk = st.blocks[1 if shift else 0]
    nbuf = max(3, -(-RING_BYTES // (side * side * C * xdt.itemsize)))
    xs = [torch.randn(1, side * side, C, device=dev).to(xdt).requires_grad_() for _ in range(nbuf)]
    w = torch.randn(1, side * side, C, device=dev)
    n = max(calls, nbuf)
    mask = st.shift_mask(side, side, dev)
    params = list(blk.parameters())

    def forward(x):
        with torch.no_grad(), torch.autocast('cuda', dtype=dt):
            blk(x, side, side, mask)

    def both(x):
        with torch.autocast('cuda', dtype=dt):
            y = blk(x, side, side, mask)
        torch.autograd.grad((y.float() * w).sum(), [x] + params)

    def select(on, grad):
        blk.fuse_window_attention_half = on
        with torch.autocast('cuda', dtype=dt), torch.set_grad_enabled(grad):
            assert blk.fused_attention(xs[0]) is ((window_attention_train_half if grad else window_attention_half) if on else None)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    result = {'stage': stage, 'channels': C, 'heads': heads, 'tokens': side * side, 'shift': 3 if shift else 0, 'calls': n, 'dtype': dtype}
    for mode, once, grad in (('fwd', forward, False), ('fwd_bwd', both, True)):
        st.train(grad)
        times, peak = {'stock': [], 'fused': []}, {}
        for name, on in (('stock', False), ('fused', True)):
            select(on, grad)
            once(xs[0])                                        # first launches load code objects, libraries pick algorithms
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            before = torch.cuda.memory_allocated(dev)
            once(xs[1])
            torch.cuda.synchronize()
            peak[name] = torch.cuda.max_memory_allocated(dev) - before
        for _ in range(rounds + 1):                            # the first round warms up and is dropped
            for name, on in (('stock', False), ('fused', True)):
                select(on, grad)
                e0.record()
                for i in range(n):
                    once(xs[i % nbuf])
                e1.record()
                torch.cuda.synchronize()
                times[name].append(round(e0.elapsed_time(e1) * 1e3 / n, 2))
        result[mode] = {'stock_us': times['stock'][1:], 'fused_us': times['fused'][1:], 'stock_peak_bytes': peak['stock'],
                        'fused_peak_bytes': peak['fused']}
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--dtype', choices=('fp16', 'bf16'), default='fp16')
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--step-timeout', type=int, default=120)
    ap.add_argument('--step')
    args = ap.parse_args()
    if args.step:
        stage, shift = (int(v) for v in args.step.split(','))
        print(json.dumps(run_step(stage, shift, args.size, args.calls, args.rounds, args.dtype)))
        return 0
    for stage in range(len(STAGES)):
        for shift in (0, 1):
            cmd = [sys.executable, os.path.abspath(__file__), '--step', '%d,%d' % (stage, shift), '--calls', str(args.calls),
                   '--rounds', str(args.rounds), '--size', str(args.size), '--dtype', args.dtype]
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
