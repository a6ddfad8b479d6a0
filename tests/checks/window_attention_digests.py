"""SHA-256 digests of everything the six window-attention operators write (`window_attention`, `window_attention_forward_lse`,
`window_attention_backward` and their `_half` forms), for fixed seeds, at the smallest shapes that reach every code path of the kernels:
what two builds of the library have to agree on, byte for byte, when a change claims to leave the arithmetic alone.

    python tests/checks/window_attention_digests.py [--out FILE.jsonl] [--step-timeout 120]

Run it on both builds and compare the files (the lines carry no time and no build id, so equal behaviour gives equal files).

Each (dtype, heads, head dim) is a STEP: a fresh child process of this script (`--step DTYPE,HEADS,HEAD_DIM`) under its own time limit;
the parent stops at the first step that fails or runs out of time and starts nothing after it.  A step runs its cases and prints
(and with --out the parent appends) one JSON line per case:
  * (heads, head dim): (2, 4), (2, 12), (1, 28) -- one key per unrolled step -- and (3, 32) -- half a row in flight;
  * (B, H, W, shift): (1, 15, 20, 3) padded on both axes and shifted, (2, 14, 14, 0) whole windows and two images, (1, 5, 9, 3) a map
    smaller than one window;
  * with and without a qkv bias; the backward with a bias also without `grad_qkv_bias` (straight through the C entry point: the Python
    operator always asks for it);
  * fp32, fp16, bf16.
A case's line holds the digest of every output tensor: out of the inference forward; out and lse of the training forward; grad_qkv,
grad_qkv_bias and grad_bias_table of the backward.  It reads nothing outside the repository."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

HEADS = [(2, 4), (2, 12), (1, 28), (3, 32)]                     # (heads, head dim)
MAPS = [(1, 15, 20, 3), (2, 14, 14, 0), (1, 5, 9, 3)]           # (B, H, W, shift)
DTYPES = ('fp32', 'fp16', 'bf16')


def digest(t):
    import torch
    return None if t is None else hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def run_step(dtype, heads, hd):
    import torch
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd import mmdet_ops as wa
    from orientedreppoints_amd.mmdet_ops.window_attention import HALF_DTYPES
    dev = torch.device('cuda', 0)
    dt = dict(fp32=torch.float32, fp16=torch.float16, bf16=torch.bfloat16)[dtype]
    half = dtype != 'fp32'
    infer = wa.window_attention_half if half else wa.window_attention
    forward = wa.window_attention_forward_lse_half if half else wa.window_attention_forward_lse
    backward = wa.window_attention_backward_half if half else wa.window_attention_backward
    C, scale = heads * hd, hd ** -0.5
    lines = []
    for B, H, W, shift in MAPS:
        for with_bias in (True, False):
            g = torch.Generator().manual_seed(1000 * hd + 100 * H + 10 * shift + int(with_bias))
            qkv = torch.randn((B, H * W, 3 * C), generator=g).to(dt).to(dev)
            go = torch.randn((B, H * W, C), generator=g).to(dt).to(dev)
            table = (0.5 * torch.randn((169, heads), generator=g)).to(dev)
            bias = torch.randn((3 * C,), generator=g).to(dev) if with_bias else None
            geo = (H, W, heads, 7, shift, scale)
            d = {'inference.out': digest(infer(qkv, bias, table, *geo))}
            out, lse = forward(qkv, bias, table, *geo)
            d['train.out'], d['train.lse'] = digest(out), digest(lse)
            gq, gb, gt = backward(qkv, bias, table, out, lse, go, *geo)
            d['backward.grad_qkv'], d['backward.grad_qkv_bias'], d['backward.grad_bias_table'] = digest(gq), digest(gb), digest(gt)
            if with_bias:                                      # ... and without grad_qkv_bias: the C call, as the operators make it
                L = _lib.lib()
                gq2, gt2 = torch.full_like(gq, 7.0), torch.full_like(gt, 7.0)
                ws = torch.empty(L.orp_window_attention_backward_workspace_bytes(B, H, W, heads, hd, 7), dtype=torch.uint8, device=dev)
                args = [_lib.ptr(t) for t in (qkv, bias, table, out, lse, go)] + [B, H, W, heads, hd, 7, shift, float(scale),
                                                                                _lib.ptr(gq2), None, _lib.ptr(gt2), _lib.ptr(ws), ws.numel()]
                if half:
                    rc = L.orp_window_attention_backward_h(*args, HALF_DTYPES[dt], _lib.stream_of(qkv))
                else:
                    rc = L.orp_window_attention_backward(*args, _lib.stream_of(qkv))
                _lib.check(rc, "orp_window_attention_backward")
                d['backward_no_bias_grad.grad_qkv'], d['backward_no_bias_grad.grad_bias_table'] = digest(gq2), digest(gt2)
            torch.cuda.synchronize()
            lines.append(json.dumps({'dtype': dtype, 'heads': heads, 'head_dim': hd, 'batch': B, 'height': H, 'width': W, 'shift': shift,
                                     'qkv_bias': with_bias, 'digests': d}, sort_keys=True))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--step-timeout', type=int, default=120)
    ap.add_argument('--step')
    args = ap.parse_args()
    if args.step:
        dtype, heads, hd = args.step.split(',')
        print('\n'.join(run_step(dtype, int(heads), int(hd))))
        return 0
    for dtype in DTYPES:
        for heads, hd in HEADS:
            step = '%s,%d,%d' % (dtype, heads, hd)
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', step], stdout=subprocess.PIPE,
                                   universal_newlines=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                print('step %s ran out of time: stopping' % step)
                return 124
            if r.returncode != 0:
                print('step %s failed with status %d: stopping' % (step, r.returncode))
                return r.returncode
            lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
            print('\n'.join(lines), flush=True)
            if args.out:
                with open(args.out, 'a') as f:
                    f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
