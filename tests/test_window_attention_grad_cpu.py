"""CPU: what the fused Swin attention's BACKWARD rests on, its routing rule and the training kernels' register budget.

The backward of `orp_window_attention_backward` is defined by `window_attention_reference` (mmdet_ops/window_attention.py), which is
differentiable plain torch.  Held here in float64 against the stock SwinBlock's autograd (pad, roll, to_windows,
scaled_dot_product_attention with the materialised mask, from_windows, roll, crop): gradients with respect to the input tokens,
qkv.weight, qkv.bias, proj.weight and the bias table.  Both are float64 evaluations of the same real function and only the order of
the sums differs, so they agree to 1e-10 of each gradient's maximum."""
import pytest
import torch

from orientedreppoints_amd.mmdet_ops import window_attention_ok, window_attention_train_ok
from test_window_attention_cpu import DIMS, MAPS, make_stage, reexpressed
from window_attention_metadata import instantiations


def check_block_gradients(st, shape, shift, seed):
    B, H, W = shape
    blk = st.blocks[1 if shift else 0]
    assert blk.shift == shift
    a = blk.attn
    params = [a.qkv.weight, a.proj.weight, a.relative_position_bias_table] + ([] if a.qkv.bias is None else [a.qkv.bias])
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, H * W, a.dim), generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn((B, H * W, a.dim), generator=g, dtype=torch.float64)
    want = torch.autograd.grad((blk(x, H, W, st.shift_mask(H, W, x.device).double()) * w).sum(), [x] + params)
    got = torch.autograd.grad((reexpressed(blk, x, H, W) * w).sum(), [x] + params)
    for name, gw, gg in zip(["x", "qkv.weight", "proj.weight", "bias table", "qkv.bias"], want, got):
        err, top = float((gg - gw).abs().max()), float(gw.abs().max())
        assert top > 0 and err <= 1e-10 * top, (shape, shift, name, err, top)


@pytest.mark.parametrize("shift", [0, 3])
@pytest.mark.parametrize("shape", MAPS)
@pytest.mark.parametrize("dims", DIMS)
def test_reference_gradients_are_the_stock_blocks(dims, shape, shift):
    check_block_gradients(make_stage(*dims), shape, shift, seed=17)


def test_reference_gradients_without_a_qkv_bias():
    check_block_gradients(make_stage(96, 3, qkv_bias=False), (1, 15, 20), 3, seed=18)


def test_reference_gradients_with_a_given_scale():
    check_block_gradients(make_stage(24, 2, qk_scale=0.3), (1, 15, 20), 3, seed=19)


def test_training_routing_rule_on_the_cpu():
    st = make_stage(24, 2).float()
    x = torch.randn(1, 49, 24)
    with torch.enable_grad():
        assert not window_attention_train_ok(st.blocks[0].attn, x)                # a CPU tensor
        assert not window_attention_train_ok(st.blocks[0].attn, x.half())
        assert not window_attention_train_ok(make_stage(24, 2, window=4).float().blocks[0].attn, x)
        assert not window_attention_train_ok(make_stage(24, 2, attn_drop=0.1).float().train().blocks[0].attn, x)
        assert not st.blocks[1].fuses_attention_train(x)
        assert not window_attention_ok(st.blocks[0].attn, x)                      # unchanged: never with gradients enabled
    with torch.no_grad():
        assert not window_attention_train_ok(st.blocks[0].attn, x)
        assert not window_attention_ok(st.blocks[0].attn, x)                      # unchanged: a CPU tensor
    assert sorted(k for k in st.state_dict() if 'fuse' in k) == []


def test_training_kernels_spill_nothing_and_use_no_scratch():
    """Code-object metadata of the built library: the eight head-dim instantiations each of the forward and of the backward on fp32
    operands spill no VGPR and use no scratch memory, at or under the 168 registers their `amdgpu_waves_per_eu(3)` declares."""
    seen = {key[:2]: meta for key, meta in instantiations().items() if key[2] == 0}
    assert sorted(seen) == [(k, hd) for k in ("wattn_bwd_kernel", "wattn_fwd_kernel") for hd in range(4, 33, 4)], sorted(seen)
    for key, (spill, scratch, vgprs, _) in seen.items():
        assert spill == 0 and scratch == 0 and vgprs <= 168, (key, spill, scratch, vgprs)
