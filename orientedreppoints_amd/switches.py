"""Every environment switch of the Python layer, read ONCE when the package is imported (never inside a forward pass).

Defaults are the product; each switch exists for A/B timing of one design decision and has a module attribute that overrides it per
object.  The library's own switches (C side) are `ORP_DCN_SPLIT` (arithmetic of the fp32 contractions: 3 default, 6, 9, 0 = exact fp32
MFMA; `orp_dcn_set_split_mode`), `ORP_DCNS_MT` (tile height of the split kernel, dev aid), `ORP_DCN_KSPLIT` (tap-granular split of
the exact-fp32 DeformConv launch), `ORP_CONV_HALO` (0: the 3x3 stride-1 fp16-pieces convolutions on the linear-tile kernel instead of
the halo kernel; `orp_conv_split_set_halo`) and `ORP_FILL=memset` (fills as hipMemsetAsync instead of kernels: the A/B aid of DESIGN.md 4.5).
The table in DESIGN.md section 0 lists them all with what they default to and why.
"""
import os


def _on(name, default='1'):
    return os.environ.get(name, default) == '1'


TOWER_SPLIT = _on('ORP_TOWER_SPLIT')          # head towers on the split matrix-pipe kernel (head.split_towers overrides)
FPN_SPLIT = _on('ORP_FPN_SPLIT')              # FPN output convolutions on it (neck.split_convs overrides)
TOWER_GN_FUSE = _on('ORP_TOWER_GN_FUSE')      # GroupNorm fused around the tower convolutions (head.fuse_tower_norm overrides)
BN_DOWNSAMPLE_FUSE = _on('ORP_BN_DOWNSAMPLE_FUSE')  # downsample BatchNorm inside the block-final pass (block.fuse_downsample_norm overrides)
BN_CONV1X1_FUSE = _on('ORP_BN_CONV1X1_FUSE')  # bottleneck conv1 / conv3 with BatchNorm (+ residual) + ReLU in the epilogue where measured faster (block.fuse_conv1x1 overrides)
BN_CONV1X1_PIECES = _on('ORP_BN_CONV1X1_PIECES')  # bottleneck conv1 / conv3 on the bf16-pieces kernel where measured faster than both the library and the fp32 kernel (block.fuse_conv1x1_pieces overrides)
BN_DOWNSAMPLE_CONV_FUSE = _on('ORP_BN_DOWNSAMPLE_CONV_FUSE')  # the downsample convolution contracted inside conv3's bf16-pieces launch where measured faster than library convolution + that launch (block.fuse_downsample_conv overrides)
BN_CONV3X3_FUSE = _on('ORP_BN_CONV3X3_FUSE')  # bottleneck conv2 (3x3, stride 1) on the fp16-pieces kernel with BatchNorm + ReLU in the epilogue where measured faster (block.fuse_conv3x3 overrides)
BN_CONV3X3_DEEP_FUSE = _on('ORP_BN_CONV3X3_DEEP_FUSE')  # stage 4 conv2 (512 channels, stride 1 and 2) on the K-split fp16-pieces kernel with BatchNorm + ReLU in the epilogue where measured faster; asked only where the kernel above said no (block.fuse_conv3x3_deep overrides)
BN_CONV3X3_S2_FUSE = _on('ORP_BN_CONV3X3_S2_FUSE')  # the stride-2 conv2 of stages 2 and 3 (128 and 256 channels) on the narrow-pass fp16-pieces kernel with BatchNorm + ReLU in the epilogue where measured faster; asked only where the two kernels above said no (block.fuse_conv3x3_s2 overrides)
BN_TRAIN_FUSE = _on('ORP_BN_TRAIN_FUSE')      # training, stages that train: eval-mode BatchNorm (+ residual) + ReLU behind the bottleneck convolutions as one forward pass and one backward pass with dweight / dbias (block.fuse_bn_train overrides)
BN_FROZEN_FUSE = _on('ORP_BN_FROZEN_FUSE')    # training, frozen stem / stages (no parameter and no input that requires a gradient): the inference route, under its own switches above and below (block.fuse_bn_frozen / backbone.fuse_bn_frozen override)
STEM_POOL_FUSE = _on('ORP_STEM_POOL_FUSE')    # stem BatchNorm + ReLU + max-pool as one kernel (backbone.fuse_stem_pool overrides)
STEM_CONV_FUSE = _on('ORP_STEM_CONV_FUSE')    # the whole stem (7x7 convolution + BatchNorm + ReLU + max-pool) as one exact-fp32 MFMA launch where measured faster than library convolution + the kernel above; asked first, does not consult that switch (backbone.fuse_stem_conv overrides)
SWIN_ATTN_FUSE = _on('ORP_SWIN_ATTN_FUSE')    # Swin inference: pad / roll / windows / bias / mask / softmax / P V / un-roll / crop as one fp32 kernel (block.fuse_window_attention overrides)
SWIN_ATTN_TRAIN_FUSE = _on('ORP_SWIN_ATTN_TRAIN_FUSE')  # Swin training: the same between attn.qkv and attn.proj as one fp32 forward kernel that keeps the rows' log-sum-exp, and one backward call (block.fuse_window_attention_train overrides)
SWIN_ATTN_HALF_FUSE = _on('ORP_SWIN_ATTN_HALF_FUSE')  # Swin under fp16 / bf16 autocast, inference and training: the same span on 16-bit operands with fp32 arithmetic, one forward kernel (+ one backward call) (block.fuse_window_attention_half overrides)
SWIN_LINEAR_FUSE = _on('ORP_SWIN_LINEAR_FUSE')  # Swin inference, eval-mode blocks on the fused fp32 attention route: attn.qkv, attn.proj (+ residual), mlp.fc1 (+ GELU), mlp.fc2 (+ residual) and PatchMerging.reduction as bf16-pieces launches with the epilogue fused, each where measured faster than the library's GEMM and its GELU / addition kernels (block.fuse_token_linear / downsample.fuse_token_linear override; force_token_linear routes every supported shape)
SWIN_NORM_FUSE = _on('ORP_SWIN_NORM_FUSE', '0')  # (ships OFF: docs/notebook/round32.md) Swin inference (fp32 device tensors, no gradients, no autocast): every LayerNorm with the copies beside it as one launch -- norm1 / norm2, pad + cat + PatchMerging.norm, the contiguous copy + PatchEmbed.norm, norm<i> + the permuting copy --, each where measured faster than the framework's kernels (fuse_token_norm on the block, the merge, the embedding and the backbone overrides; force_token_norm routes every supported shape)
FPN_TOPDOWN_FUSE = _on('ORP_FPN_TOPDOWN_FUSE')  # FPN lateral GroupNorm + top-down sum + transposition as one pass (neck.fuse_topdown overrides)
TRAIN_SPLIT = _on('ORP_TRAIN_SPLIT')          # training: tower / FPN convolutions as conv_split_train nodes
DETERMINISTIC = _on('ORP_DETERMINISTIC', '0')  # training: fixed-order DeformConv backward for both branches (head.deterministic_backward overrides)


def of(obj, attr, name):
    """the switch `name` as `obj` sees it: its attribute `attr` where that is set (not None), else this module's `name`, read now"""
    on = getattr(obj, attr, None)
    return bool(globals()[name] if on is None else on)
