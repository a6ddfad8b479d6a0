"""CPU: the reformulation the fused Swin attention rests on, its routing rule and the kernel's register budget.

`window_attention_reference` (mmdet_ops/window_attention.py) is the kernel's semantics in plain torch: qkv on the un-padded, un-rolled
tokens, a padded token's q / k / v = the qkv bias, pad / roll / windows / relative-position bias / shift mask / un-roll / crop as index
arithmetic, proj after the crop.  Held here in float64 against the stock SwinBlock (pad, roll, to_windows, scaled_dot_product_attention
with the materialised mask, from_windows, roll, crop): both are float64 evaluations of the same real function and only the order of
the sums differs, so they agree to 1e-12 of the output's maximum."""
import pytest
import torch

from orientedreppoints_amd import switches
from orientedreppoints_amd.mmdet_models.swin import SwinStage, SwinTransformer
from orientedreppoints_amd.mmdet_ops import window_attention_ok, window_attention_reference
from window_attention_metadata import instantiations

DIMS = [(24, 2), (96, 4), (96, 3)]                                  # (channels, heads): head dims 12, 24, 32
MAPS = [(2, 14, 14), (1, 15, 20), (1, 5, 9), (1, 38, 51)]            # whole windows; padded on both axes; smaller than a window; many
CFG = dict(embed_dim=24, depths=[2, 2, 2, 2], num_heads=[2, 4, 4, 8], window_size=7, mlp_ratio=4., qkv_bias=True, qk_scale=None,
           drop_rate=0., attn_drop_rate=0., drop_path_rate=0.2, ape=False, patch_norm=True, out_indices=(1, 2, 3), use_checkpoint=False)


def make_stage(C, heads, qkv_bias=True, qk_scale=None, window=7, attn_drop=0., seed=0):
    """two blocks (un-shifted, shifted by window // 2) with parameters that make every term matter: qkv.bias ~ N(0, 1) (padded tokens),
    table ~ 0.5 N(0, 1), weights ~ N(0, 1 / fan_in)"""
    g = torch.Generator().manual_seed(seed)
    st = SwinStage(C, 2, heads, window, 4., qkv_bias, qk_scale, 0., attn_drop, [0., 0.], False, False).double().eval()
    with torch.no_grad():
        for k, p in st.named_parameters():
            if k.endswith('qkv.bias'):
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64))
            elif 'relative_position_bias_table' in k:
                p.copy_(0.5 * torch.randn(p.shape, generator=g, dtype=torch.float64))
            elif p.dim() == 2:
                p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) / p.size(1) ** 0.5)
            elif k.endswith('bias'):
                p.copy_(0.1 * torch.randn(p.shape, generator=g, dtype=torch.float64))
    return st


def reexpressed(blk, x, H, W):
    """the block as the fused route computes it, with the reference operator in the kernel's place"""
    a = blk.attn
    y = window_attention_reference(a.qkv(blk.norm1(x)), a.qkv.bias, a.relative_position_bias_table, H, W, a.num_heads, blk.ws,
                                   blk.shift, a.scale)
    x = x + a.proj(y)
    return x + blk.mlp(blk.norm2(x))


def check_block(st, shape, shift, seed):
    B, H, W = shape
    blk = st.blocks[1 if shift else 0]
    assert blk.shift == shift
    x = torch.randn((B, H * W, st.blocks[0].attn.dim), generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    with torch.no_grad():
        want = blk(x, H, W, st.shift_mask(H, W, x.device).double())
        got = reexpressed(blk, x, H, W)
    err, top = float((got - want).abs().max()), float(want.abs().max())
    assert err <= 1e-12 * top, (shape, shift, err, top)


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("shape", MAPS)
@pytest.mark.parametrize("dims", DIMS)
def test_reference_operator_is_the_stock_block(dims, shape, shift):
    check_block(make_stage(*dims), shape, shift, seed=7)


def test_reference_operator_without_a_qkv_bias():
    check_block(make_stage(96, 3, qkv_bias=False), (1, 15, 20), 3, seed=8)      # padded tokens' q / k / v are zero


def test_reference_operator_with_a_given_scale():
    st = make_stage(24, 2, qk_scale=0.3)
    assert st.blocks[1].attn.scale == 0.3
    check_block(st, (1, 15, 20), 3, seed=9)


def test_routing_rule_on_the_cpu():
    st = make_stage(24, 2).float()
    x = torch.randn(1, 49, 24)
    with torch.no_grad():
        assert not window_attention_ok(st.blocks[0].attn, x)                      # a CPU tensor
        assert not window_attention_ok(st.blocks[0].attn, x.half())
        assert not window_attention_ok(make_stage(24, 2, window=4).float().blocks[0].attn, x)
        assert not window_attention_ok(make_stage(24, 2, attn_drop=0.1).float().train().blocks[0].attn, x)
        assert not st.blocks[1].fuses_attention(x)
    with torch.enable_grad():
        assert not window_attention_ok(st.blocks[0].attn, x)


def test_cpu_forward_is_bit_identical_with_the_switch_on_and_off(monkeypatch):
    torch.manual_seed(0)
    model = SwinTransformer(**CFG).eval()
    x = torch.randn(1, 3, 61, 97)
    outs = []
    with torch.no_grad():
        for on in (True, False):
            monkeypatch.setattr(switches, 'SWIN_ATTN_FUSE', on)
            outs.append(model(x))
        for m in model.modules():
            if hasattr(m, 'fuses_attention'):
                m.fuse_window_attention = True
        outs.append(model(x))
    for other in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(outs[0], other))
    assert sorted(k for k in model.state_dict() if 'fuse' in k) == []


def test_window_attention_kernels_spill_nothing_and_use_no_scratch():
    """Code-object metadata of the built library: every head-dim instantiation of the forward kernel on fp32 operands (4, 8, ..., 32)
    keeps its query, its accumulators and a window row's key pieces in registers -- no spilled VGPR, no scratch memory -- at three
    waves per SIMD or more (at most 168 registers)."""
    seen = {key: meta for key, meta in instantiations().items() if key[0] == "wattn_fwd_kernel" and key[2] == 0}
    assert sorted(hd for _, hd, _ in seen) == list(range(4, 33, 4)), sorted(seen)
    for key, (spill, scratch, vgprs, _) in seen.items():
        assert spill == 0 and scratch == 0 and vgprs <= 168, (key, spill, scratch, vgprs)
