"""Swin Transformer backbone on stock PyTorch-ROCm (interface of mmdet/models/backbones/swin_transformer.py:450-631:
embed_dim, depths, num_heads, window_size, mlp_ratio, qkv_bias, qk_scale, drop rates, ape, patch_norm, out_indices,
frozen_stages, use_checkpoint; configs/dota/orientedrepoints_swin_tiny_demo.py:9-24).  Out of the HIP hot path: BASELINE.json
keeps the backbone on the framework.  Written from the paper (Liu et al., "Swin Transformer: Hierarchical Vision Transformer
using Shifted Windows", 2021): windowed multi-head self-attention with a learned relative-position bias, every second block
on windows shifted by half a window (cyclic roll + a mask that separates the wrapped-around regions), patch merging between
stages.  Own layout of the computation: one `scaled_dot_product_attention` call per block over all windows with the
(bias + shift mask) tensor as its additive mask, the shift masks built once per (resolution, device).  At inference on fp32 device
tensors a block runs everything between `attn.qkv` and `attn.proj` as one HIP kernel on the un-padded, un-rolled tokens instead
(`SwinBlock.fuses_attention`, mmdet_ops/window_attention.py; switch ORP_SWIN_ATTN_FUSE / `block.fuse_window_attention`); with
gradients enabled the same span is `window_attention_train`, a forward kernel that keeps the rows' log-sum-exp and a backward call
(`SwinBlock.fuses_attention_train`; switch ORP_SWIN_ATTN_TRAIN_FUSE / `block.fuse_window_attention_train`).  Under fp16 / bf16
autocast `attn.qkv` yields 16-bit q / k / v and the span is `window_attention_half` / `window_attention_train_half`: the same kernels
on 16-bit operands, fp32 arithmetic (`SwinBlock.fuses_attention_half`; switch ORP_SWIN_ATTN_HALF_FUSE / `block.fuse_window_attention_half`).
An eval-mode block on the fp32 inference route also runs its four linears -- `attn.qkv`, `attn.proj` with the block input as residual,
`mlp.fc1` with the GELU, `mlp.fc2` with its residual -- and `PatchMerging` its `reduction` as bf16-pieces launches with the epilogue
fused, each where measured faster (`SwinBlock.fuses_linears`, mmdet_ops/token_linear.py; switch ORP_SWIN_LINEAR_FUSE /
`fuse_token_linear`).  On the same fp32 inference route (no gradients, no autocast, contiguous fp32 device tensors) every LayerNorm is
one launch of `token_layernorm` together with the copies around it -- a block's `norm1` / `norm2`, pad + cat + `PatchMerging.norm` as a
gather, the contiguous copy in front of `PatchEmbed.norm`, and `norm<i>` with the permuting copy behind it --, each where measured
faster (`_norm`, mmdet_ops/token_norm.py; switch ORP_SWIN_NORM_FUSE / `fuse_token_norm`, `force_token_norm` for every supported shape).
That switch ships OFF: the eager detector, which waits on the host, did not gain (docs/notebook/round32.md); the captured one does.

Parameter / buffer names are the released checkpoints' (`swin_tiny_patch4_window7_224.pth`): patch_embed.{proj,norm},
layers.<i>.blocks.<j>.{norm1,attn.{relative_position_bias_table,relative_position_index,qkv,proj},norm2,mlp.{fc1,fc2}},
layers.<i>.downsample.{norm,reduction}, norm<i> for every output stage, absolute_pos_embed with ape=True."""
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as cp

from .. import switches
from ..mmdet_ops.token_linear import token_linear, token_linear_ok, token_linear_routed
from ..mmdet_ops.token_norm import token_layernorm_if_routed
from ..mmdet_ops.window_attention import (window_attention, window_attention_half, window_attention_half_ok, window_attention_ok,
                                          window_attention_train, window_attention_train_half, window_attention_train_half_ok,
                                          window_attention_train_ok)
from .registry import BACKBONES


def _linear(owner, linear, x, act=None, residual=None):
    """act(linear(x)) + residual for a module whose linears go through `token_linear`: one launch where the routing table says so
    (`owner.force_token_linear`, tests: at every shape the kernel takes), else the library's launches with their bits"""
    force = bool(getattr(owner, 'force_token_linear', False))
    res_ok = residual is None or (residual.is_contiguous() and residual.dtype == torch.float32)
    if res_ok and (token_linear_ok(linear, x) if force else token_linear_routed(linear, x, act, residual)):
        return token_linear(x, linear, act, residual, force=True)
    y = linear(x)
    if act == 'gelu':
        y = F.gelu(y)
    return y if residual is None else residual + y


def _norm(owner, ln, x, layout='tokens', hw=None):
    """the LayerNorm `ln` with the copies beside it, for a module whose norms go through `token_layernorm`: one launch where the switch is
    on and the routing table says so (`owner.force_token_norm`, tests: at every shape the kernel takes), else the lines as the modules
    always ran them, with their bits.  'tokens': ln(x).  'merge': x [B, H, W, C] -> pad, cat of the 2 x 2 neighbourhood, ln: [B, L/4, 4C].
    'from_nchw': x [B, C, L] -> ln(x.transpose(1, 2)): [B, L, C].  'to_nchw': x [B, L, C] -> ln(x) as contiguous [B, C, H, W]."""
    if switches.of(owner, 'fuse_token_norm', 'SWIN_NORM_FUSE'):
        y = token_layernorm_if_routed(x, ln, layout, hw, force=bool(getattr(owner, 'force_token_norm', False)))
        if y is not None:
            return y
    if layout == 'merge':
        B, H, W, C = x.shape
        if H % 2 or W % 2:
            x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
        # channel order of the released weights: (even row, even col), (odd, even), (even, odd), (odd, odd)
        x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
        return ln(x.view(B, -1, 4 * C))
    if layout == 'from_nchw':
        return ln(x.transpose(1, 2))
    if layout == 'to_nchw':
        return ln(x).view(-1, hw[0], hw[1], x.size(-1)).permute(0, 3, 1, 2).contiguous()
    return ln(x)


class StochasticDepth(nn.Module):
    """Drops the residual branch of whole samples with probability p (training only), rescaling the survivors."""

    def __init__(self, p):
        super().__init__()
        self.p = float(p)

    def forward(self, x):
        if self.p == 0.0 or not self.training:
            return x
        keep = torch.rand((x.size(0),) + (1,) * (x.dim() - 1), device=x.device, dtype=x.dtype) >= self.p
        return x * keep / (1.0 - self.p)


def to_windows(x, ws):
    """[B, H, W, C] (H, W multiples of ws) -> [B * nW, ws * ws, C], windows in row-major order."""
    B, H, W, C = x.shape
    x = x.view(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5)
    return x.reshape(-1, ws * ws, C)


def from_windows(w, ws, H, W):
    B = w.size(0) // ((H // ws) * (W // ws))
    x = w.view(B, H // ws, W // ws, ws, ws, -1).permute(0, 1, 3, 2, 4, 5)
    return x.reshape(B, H, W, -1)


class WindowAttention(nn.Module):
    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.dim, self.ws, self.num_heads = dim, window_size, num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window_size - 1) ** 2, num_heads))
        # pair (i, j) of window positions -> row of the table: (dy + ws - 1) * (2 ws - 1) + (dx + ws - 1)
        ys, xs = torch.meshgrid(torch.arange(window_size), torch.arange(window_size), indexing='ij')
        pos = torch.stack([ys.flatten(), xs.flatten()])                       # [2, N]
        rel = pos[:, :, None] - pos[:, None, :] + (window_size - 1)             # [2, N, N]
        self.register_buffer('relative_position_index', rel[0] * (2 * window_size - 1) + rel[1])
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)

    def forward(self, x, shift_mask=None):
        """x [nWB, N, C]; shift_mask None or [nW, N, N] (0 / -100)."""
        BW, N, C = x.shape
        q, k, v = self.qkv(x).view(BW, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        bias = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(N, N, -1).permute(2, 0, 1)
        bias = bias.unsqueeze(0).to(q.dtype)                                   # [1, heads, N, N]
        if shift_mask is not None:
            nW = shift_mask.size(0)
            bias = (bias + shift_mask.to(q.dtype).unsqueeze(1)).repeat(BW // nW, 1, 1, 1)
        out = F.scaled_dot_product_attention(q, k, v, attn_mask=bias, scale=self.scale,
                                             dropout_p=self.attn_drop.p if self.training else 0.0)
        return self.proj_drop(self.proj(out.transpose(1, 2).reshape(BW, N, C)))


class Mlp(nn.Module):
    def __init__(self, dim, hidden, drop=0.):
        super().__init__()
        self.fc1, self.act, self.fc2, self.drop = nn.Linear(dim, hidden), nn.GELU(), nn.Linear(hidden, dim), nn.Dropout(drop)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


class SwinBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size, shift, mlp_ratio, qkv_bias, qk_scale, drop, attn_drop, drop_path):
        super().__init__()
        self.ws, self.shift = window_size, shift
        self.norm1 = nn.LayerNorm(dim)
        self.attn = WindowAttention(dim, window_size, num_heads, qkv_bias, qk_scale, attn_drop, drop)
        self.drop_path = StochasticDepth(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio), drop)
        self.fuse_token_norm, self.force_token_norm = None, False     # (`_norm`: None = the switch)

    def fuses_attention(self, x):
        """inference on fp32 device tokens: everything between attn.qkv and attn.proj as one kernel (mmdet_ops/window_attention.py)"""
        return switches.of(self, 'fuse_window_attention', 'SWIN_ATTN_FUSE') and window_attention_ok(self.attn, x)

    def fuses_attention_train(self, x):
        """the same with gradients enabled: a forward kernel that keeps the rows' log-sum-exp, and one backward call"""
        return switches.of(self, 'fuse_window_attention_train', 'SWIN_ATTN_TRAIN_FUSE') and window_attention_train_ok(self.attn, x)

    def fuses_attention_half(self, x):
        """under fp16 / bf16 autocast: `attn.qkv` yields 16-bit q / k / v and the kernels take them as they are (fp32 arithmetic);
        `window_attention_half` without gradients, `window_attention_train_half` with"""
        if not switches.of(self, 'fuse_window_attention_half', 'SWIN_ATTN_HALF_FUSE'):
            return None
        if window_attention_half_ok(self.attn, x):
            return window_attention_half
        return window_attention_train_half if window_attention_train_half_ok(self.attn, x) else None

    def fused_attention(self, x):
        """the operator this block runs between attn.qkv and attn.proj on `x`, or None for the stock route: fp32 inference, fp32
        training, 16-bit inference, 16-bit training, in this order"""
        if self.fuses_attention(x):
            return window_attention
        return window_attention_train if self.fuses_attention_train(x) else self.fuses_attention_half(x)

    def fuses_linears(self, x):
        """an eval-mode block (dropout and drop_path are identities) on the fp32 inference attention route, contiguous tokens: qkv,
        proj + residual, fc1 + GELU and fc2 + residual through `token_linear`, each where routed"""
        return bool(not self.training and switches.of(self, 'fuse_token_linear', 'SWIN_LINEAR_FUSE') and self.fuses_attention(x) and
                    x.is_contiguous())

    def forward(self, x, H, W, shift_mask):
        if self.fuses_linears(x):
            a, m = self.attn, self.mlp
            y = window_attention(_linear(self, a.qkv, _norm(self, self.norm1, x)), a.qkv.bias, a.relative_position_bias_table, H, W, a.num_heads,
                                 self.ws, self.shift, a.scale)
            x = _linear(self, a.proj, y, None, x)
            return _linear(self, m.fc2, _linear(self, m.fc1, _norm(self, self.norm2, x), 'gelu'), None, x)
        fused = self.fused_attention(x)
        if fused is not None:
            # qkv and proj are per-token linears: both run on the un-padded, un-rolled tokens, the kernel does the index arithmetic
            a = self.attn
            y = fused(a.qkv(_norm(self, self.norm1, x)), a.qkv.bias, a.relative_position_bias_table, H, W, a.num_heads, self.ws, self.shift, a.scale)
            x = x + self.drop_path(a.proj_drop(a.proj(y)))
            return x + self.drop_path(self.mlp(_norm(self, self.norm2, x)))
        B, L, C = x.shape
        ws = self.ws
        y = _norm(self, self.norm1, x).view(B, H, W, C)
        pr, pb = (ws - W % ws) % ws, (ws - H % ws) % ws                        # pad to whole windows (bottom / right)
        if pr or pb:
            y = F.pad(y, (0, 0, 0, pr, 0, pb))
        Hp, Wp = H + pb, W + pr
        if self.shift:
            y = torch.roll(y, shifts=(-self.shift, -self.shift), dims=(1, 2))
        y = self.attn(to_windows(y, ws), shift_mask if self.shift else None)
        y = from_windows(y, ws, Hp, Wp)
        if self.shift:
            y = torch.roll(y, shifts=(self.shift, self.shift), dims=(1, 2))
        if pr or pb:
            y = y[:, :H, :W, :]
        x = x + self.drop_path(y.reshape(B, L, C))
        return x + self.drop_path(self.mlp(_norm(self, self.norm2, x)))


class PatchMerging(nn.Module):
    """2 x 2 neighbourhoods concatenated (4C), normalised, projected to 2C."""

    def __init__(self, dim):
        super().__init__()
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(4 * dim)
        self.fuse_token_norm, self.force_token_norm = None, False

    def forward(self, x, H, W):
        B, L, C = x.shape
        x = _norm(self, self.norm, x.view(B, H, W, C), 'merge')       # pad, cat of the 2 x 2 neighbourhood, norm: [B, L/4, 4C]
        if not self.training and switches.of(self, 'fuse_token_linear', 'SWIN_LINEAR_FUSE'):
            return _linear(self, self.reduction, x)       # (fp32 inference on CUDA tokens, where routed; else the module as written)
        return self.reduction(x)


class SwinStage(nn.Module):
    def __init__(self, dim, depth, num_heads, window_size, mlp_ratio, qkv_bias, qk_scale, drop, attn_drop, drop_path,
                 downsample, use_checkpoint):
        super().__init__()
        self.ws, self.shift, self.use_checkpoint = window_size, window_size // 2, use_checkpoint
        self.blocks = nn.ModuleList([
            SwinBlock(dim, num_heads, window_size, 0 if i % 2 == 0 else window_size // 2, mlp_ratio, qkv_bias, qk_scale,
                      drop, attn_drop, drop_path[i]) for i in range(depth)])
        self.downsample = PatchMerging(dim) if downsample else None
        self._masks = {}

    def shift_mask(self, H, W, device):
        """[nW, N, N]: 0 where two positions of a shifted window come from the same image region, -100 otherwise."""
        ws, s = self.ws, self.shift
        Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
        key = (Hp, Wp, device)
        m = self._masks.get(key)
        if m is None:
            region = torch.zeros(Hp, Wp, device=device)
            bands = (slice(0, -ws), slice(-ws, -s), slice(-s, None))
            for a, hs in enumerate(bands):
                for b, wsl in enumerate(bands):
                    region[hs, wsl] = 3 * a + b
            r = to_windows(region.view(1, Hp, Wp, 1), ws).squeeze(-1)          # [nW, N]
            m = (r[:, None, :] != r[:, :, None]).float() * -100.0
            if len(self._masks) > 8:
                self._masks.clear()
            self._masks[key] = m
        return m

    def forward(self, x, H, W):
        # (no block that takes the fused route reads the mask: it is not evaluated for them)
        fused = all(blk.fused_attention(x) is not None for blk in self.blocks if blk.shift)
        mask = None if fused else self.shift_mask(H, W, x.device)
        for blk in self.blocks:
            if self.use_checkpoint and x.requires_grad:
                x = cp.checkpoint(blk, x, H, W, mask, use_reentrant=False)
            else:
                x = blk(x, H, W, mask)
        if self.downsample is not None:
            return x, self.downsample(x, H, W), (H + 1) // 2, (W + 1) // 2
        return x, x, H, W


class PatchEmbed(nn.Module):
    def __init__(self, patch_size=4, in_chans=3, embed_dim=96, norm=True):
        super().__init__()
        self.patch_size = patch_size
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = nn.LayerNorm(embed_dim) if norm else None
        self.fuse_token_norm, self.force_token_norm = None, False

    def forward(self, x):
        p = self.patch_size
        H, W = x.shape[2:]
        if W % p or H % p:
            x = F.pad(x, (0, (p - W % p) % p, 0, (p - H % p) % p))
        x = self.proj(x)                                                       # [B, C, Wh, Ww]
        if self.norm is not None:
            Wh, Ww = x.shape[2:]
            x = _norm(self, self.norm, x.flatten(2), 'from_nchw').transpose(1, 2).reshape(x.size(0), -1, Wh, Ww)
        return x


@BACKBONES.register_module
class SwinTransformer(nn.Module):
    def __init__(self, pretrain_img_size=224, patch_size=4, in_chans=3, embed_dim=96, depths=(2, 2, 6, 2),
                 num_heads=(3, 6, 12, 24), window_size=7, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0.,
                 attn_drop_rate=0., drop_path_rate=0.2, norm_layer=nn.LayerNorm, ape=False, patch_norm=True,
                 out_indices=(0, 1, 2, 3), frozen_stages=-1, use_checkpoint=False):
        super().__init__()
        assert norm_layer is nn.LayerNorm
        self.num_layers, self.embed_dim, self.ape = len(depths), embed_dim, ape
        self.out_indices, self.frozen_stages = tuple(out_indices), frozen_stages
        self.patch_embed = PatchEmbed(patch_size, in_chans, embed_dim, patch_norm)
        if ape:
            side = pretrain_img_size if isinstance(pretrain_img_size, int) else pretrain_img_size[0]
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, embed_dim, side // patch_size, side // patch_size))
            nn.init.trunc_normal_(self.absolute_pos_embed, std=.02)
        self.pos_drop = nn.Dropout(p=drop_rate)
        rates = torch.linspace(0, drop_path_rate, sum(depths)).tolist()        # stochastic depth grows linearly with depth
        self.layers = nn.ModuleList()
        for i, depth in enumerate(depths):
            self.layers.append(SwinStage(embed_dim * 2 ** i, depth, num_heads[i], window_size, mlp_ratio, qkv_bias, qk_scale,
                                         drop_rate, attn_drop_rate, rates[sum(depths[:i]):sum(depths[:i + 1])],
                                         i < self.num_layers - 1, use_checkpoint))
        self.num_features = [embed_dim * 2 ** i for i in range(self.num_layers)]
        for i in self.out_indices:
            self.add_module('norm%d' % i, nn.LayerNorm(self.num_features[i]))
        self.fuse_token_norm, self.force_token_norm = None, False     # (the output norms)
        self._freeze_stages()

    def _freeze_stages(self):
        frozen = []
        if self.frozen_stages >= 0:
            frozen.append(self.patch_embed)
        if self.frozen_stages >= 1:
            frozen.append(self.pos_drop)
            if self.ape:
                self.absolute_pos_embed.requires_grad = False
            frozen += list(self.layers[:self.frozen_stages - 1])
        for m in frozen:
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

    def init_weights(self, pretrained=None):
        """`pretrained`: a local checkpoint (state dict, or {'model': ...} / {'state_dict': ...}); no network here."""
        if isinstance(pretrained, str):
            import os
            import warnings
            if os.path.isfile(pretrained):
                sd = torch.load(pretrained, map_location='cpu')
                sd = sd.get('model', sd.get('state_dict', sd))
                sd = {k[len('backbone.'):] if k.startswith('backbone.') else k: v for k, v in sd.items()}
                missing, unexpected = self.load_state_dict(sd, strict=False)
                unexpected = [k for k in unexpected if not (k.startswith('head.') or k.startswith('norm.') or 'attn_mask' in k)]
                if missing or unexpected:
                    warnings.warn('SwinTransformer.init_weights(%r): missing %s, unexpected %s'
                                  % (pretrained, list(missing)[:8], unexpected[:8]))
                return
            warnings.warn('SwinTransformer.init_weights: pretrained=%r was NOT loaded (no such file); random initialisation'
                          % pretrained)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)

    def forward(self, x):
        x = self.patch_embed(x)
        H, W = x.shape[2:]
        if self.ape:
            x = x + F.interpolate(self.absolute_pos_embed, size=(H, W), mode='bicubic')
        x = self.pos_drop(x.flatten(2).transpose(1, 2))
        outs = []
        for i, layer in enumerate(self.layers):
            out, x, Hn, Wn = layer(x, H, W)
            if i in self.out_indices:
                outs.append(_norm(self, getattr(self, 'norm%d' % i), out, 'to_nchw', (H, W)))
            H, W = Hn, Wn
        return tuple(outs)

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        return self
