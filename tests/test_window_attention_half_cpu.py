"""CPU: what the 16-bit Swin attention route (mmdet_ops/window_attention.py: window_attention_half / window_attention_train_half,
csrc/orp_window_attn.hip) rests on: its routing rules, the rounding rule for padded tokens and the kernels' register budget.

The rounding rule.  Under autocast `attn.qkv` is a 16-bit linear layer on fp32 parameters: it emits 16-bit q / k / v, and for the zero
row of a padded token exactly the bias ROUNDED to that type.  The kernels read the fp32 bias and round it themselves, so the float64
reference that the GPU tests hold them to must be fed the rounded bias: `window_attention_reference(qkv16.double(),
bias.to(dt).double(), ...)`.  Held here against the stock SwinBlock in float64 whose qkv layer emits 16-bit values (float64 product,
rounded to the type, widened): two float64 evaluations of the same real function, 1e-12 of the output's maximum as in
tests/test_window_attention_cpu.py.  With the un-rounded bias in its place the two differ by orders of magnitude more."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from orientedreppoints_amd.mmdet_ops import (window_attention_half_ok, window_attention_ok, window_attention_reference,
                                             window_attention_train_half_ok, window_attention_train_ok)
from test_window_attention_cpu import make_stage
from window_attention_metadata import HEAD_DIMS, KERNELS, OPERANDS, VGPR_CAP, instantiations

DTYPES = [torch.float16, torch.bfloat16]


def test_half_routing_rules_on_the_cpu():
    st = make_stage(24, 2).float()
    x = torch.randn(1, 49, 24)
    for ctx in (torch.no_grad, torch.enable_grad):
        with ctx():
            for blk in st.blocks:
                assert not window_attention_half_ok(blk.attn, x) and not window_attention_train_half_ok(blk.attn, x)      # a CPU tensor
                assert not window_attention_half_ok(blk.attn, x.half()) and not window_attention_train_half_ok(blk.attn, x.half())
                assert blk.fuses_attention_half(x) is None and blk.fused_attention(x) is None
            # unchanged: the fp32 predicates on CPU and 16-bit tensors
            assert not window_attention_ok(st.blocks[0].attn, x) and not window_attention_train_ok(st.blocks[0].attn, x)
            assert not window_attention_ok(st.blocks[0].attn, x.half()) and not window_attention_train_ok(st.blocks[0].attn, x.half())
    assert sorted(k for k in st.state_dict() if 'fuse' in k) == []
    for blk in st.blocks:
        blk.fuse_window_attention_half = True
    assert sorted(k for k in st.state_dict() if 'fuse' in k) == []


class Linear16(nn.Module):
    """a linear layer as autocast runs it, for a float64 model: 16-bit values out (the float64 product rounded to `dt`, widened); a zero
    row gives the bias rounded to `dt`"""

    def __init__(self, lin, dt):
        super().__init__()
        self.weight, self.dt = lin.weight, dt
        self.bias = None if lin.bias is None else lin.bias.detach().float()     # the fp32 parameter

    def forward(self, x):
        b = None if self.bias is None else self.bias.to(self.dt).double()
        return F.linear(x, self.weight, b).to(self.dt).double()


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,shift", [((1, 15, 20), 3), ((1, 15, 20), 0), ((1, 5, 9), 3), ((2, 14, 14), 3)])
def test_padded_tokens_carry_the_bias_rounded_to_the_operand_type(shape, shift, dt):
    B, H, W = shape
    st = make_stage(24, 2)
    blk = st.blocks[1 if shift else 0]
    a = blk.attn
    a.qkv = Linear16(a.qkv, dt)
    bias32 = a.qkv.bias                                                       # the fp32 parameter the kernel reads
    x = torch.randn((B, H * W, 24), generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    with torch.no_grad():
        want = blk(x, H, W, st.shift_mask(H, W, x.device).double())            # the stock route: pad, roll, windows, qkv per window
        qkv16 = a.qkv(blk.norm1(x)).to(dt)                                     # what the fused route hands to the kernel
        assert torch.equal(qkv16.double(), a.qkv(blk.norm1(x)))

        def through(bias):
            y = window_attention_reference(qkv16.double(), bias, a.relative_position_bias_table, H, W, a.num_heads, blk.ws, blk.shift, a.scale)
            y = x + a.proj(y)
            return y + blk.mlp(blk.norm2(y))
        got, unrounded = through(bias32.to(dt).double()), through(bias32.double())
    top = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-12 * top, (shape, shift, dt)
    if H % 7 or W % 7:
        assert float((unrounded - want).abs().max()) > 1e-6 * top               # the un-rounded bias is another function
    else:
        assert torch.equal(unrounded, got)                                     # no padded token: the bias is not read


def test_half_kernels_are_all_there_spill_nothing_and_use_no_scratch():
    """Code-object metadata of the built library: the forward and the backward kernel, eight head dims times three operand types each
    (fp32, fp16, bf16) and nothing else under these names; the sixteen instantiations each on fp16 and on bf16 operands spill no VGPR and
    use no scratch memory at or under the 168 registers their `amdgpu_waves_per_eu(3)` declares; the LDS of every one of them is the
    fp32 instantiation's (K / V staged as fp32)."""
    seen = instantiations()
    assert sorted(seen) == [(k, hd, dt) for k in KERNELS for hd in HEAD_DIMS for dt in OPERANDS], sorted(seen)
    for (kernel, hd, dt), (spill, scratch, vgprs, lds) in seen.items():
        if dt == 0:
            continue                                   # the fp32 budget: tests/test_window_attention_cpu.py, test_window_attention_grad_cpu.py
        assert spill == 0 and scratch == 0 and vgprs <= VGPR_CAP, (kernel, hd, dt, spill, scratch, vgprs)
        assert lds == seen[(kernel, hd, 0)][3], (kernel, hd, dt, lds)
