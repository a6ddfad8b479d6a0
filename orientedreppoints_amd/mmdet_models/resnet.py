"""ResNet backbone on stock PyTorch-ROCm (mmdet/models/backbones/resnet.py:306-520 interface: depth, num_stages,
out_indices, frozen_stages, norm_cfg, style, norm_eval).  Parameter names follow torchvision / the released
checkpoints (conv1, bn1, layer{1..4}.{i}.conv{1,2,3}, bn{1,2,3}, downsample.{0,1}).  Out of the HIP hot path: this
is the part BASELINE.json says stays stock."""
import functools

import torch
import torch.nn as nn

from .. import switches
from .layers import build_conv_layer, build_norm_layer, constant_init, kaiming_init
from .registry import BACKBONES


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style='pytorch',
                 norm_cfg=dict(type='BN'), dcn=None):
        super(Bottleneck, self).__init__()
        assert style in ['pytorch', 'caffe']
        assert dcn is None or isinstance(dcn, dict)
        if style == 'pytorch':
            conv1_stride, conv2_stride = 1, stride
        else:
            conv1_stride, conv2_stride = stride, 1
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, stride=conv1_stride, bias=False)
        self.add_module('bn1', build_norm_layer(norm_cfg, planes)[1])
        # dcn = dict(type='DCN' | 'DCNv2', deformable_groups=1, fallback_on_stride=False) turns conv2 into the
        # offset-predicting deformable convolution (mmdet/models/backbones/resnet.py:140-170); its parameters are
        # conv2.weight and conv2.conv_offset.{weight,bias}, as in the released DCN checkpoints
        self.with_dcn = dcn is not None
        fallback_on_stride = False
        if self.with_dcn:
            # as the reference does it (resnet.py:145-148): the flag is POPPED from the dict the backbone hands to every block
            # of every stage, so only the first block built from it sees the flag -- which decides the set of
            # conv2.conv_offset keys a reference-trained checkpoint has -- and a set flag means a plain conv2 whatever its stride
            fallback_on_stride = dcn.pop('fallback_on_stride', False)
            dcn = dict(dcn)
            if 'modulated' in dcn:                                   # the older spelling of the same choice
                dcn.setdefault('type', 'DCNv2' if dcn.pop('modulated') else 'DCN')
            dcn.setdefault('type', 'DCN')
        use_dcn = self.with_dcn and not fallback_on_stride
        self.conv2 = build_conv_layer(dcn if use_dcn else None, planes, planes, kernel_size=3, stride=conv2_stride,
                                      padding=dilation, dilation=dilation, bias=False)
        self.conv2_is_dcn = use_dcn
        self.add_module('bn2', build_norm_layer(norm_cfg, planes)[1])
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.add_module('bn3', build_norm_layer(norm_cfg, planes * self.expansion)[1])
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def _fused_ok(self, x):
        # inference only: eval-mode BatchNorm is a per-channel affine -> one fused HIP pass with the ReLU / residual add
        return (not torch.is_grad_enabled()) and x.is_cuda and x.dtype == torch.float32 and \
            isinstance(self.bn1, nn.BatchNorm2d) and not self.bn1.training and not self.bn3.training

    def _norms_are_eval_bn(self):
        """bn1 / bn2 / bn3 and the downsample norm (where the identity branch has one: then it is exactly Sequential(Conv2d, BatchNorm2d))
        are eval-mode BatchNorm2d"""
        return all(isinstance(bn, nn.BatchNorm2d) and not bn.training for bn in (self.bn1, self.bn2, self.bn3)) and \
            (self.downsample is None or self._downsample_is_conv_norm())

    def _frozen_ok(self, x):
        """training with this block frozen (`frozen_stages`): gradients are enabled, but no parameter of the block and not its input
        requires one, so nothing here needs autograd and the block runs the inference route as it is, under that route's switches
        (`fuse_bn_frozen` attribute, or ORP_BN_FROZEN_FUSE=0 for A/B timing: off gives the stock modules).  Not under autocast."""
        return torch.is_grad_enabled() and not torch.is_autocast_enabled() and x.is_cuda and x.dtype == torch.float32 and \
            not x.requires_grad and not getattr(self, 'with_cp', False) and \
            isinstance(self.bn1, nn.BatchNorm2d) and not self.bn1.training and not self.bn3.training and \
            switches.of(self, 'fuse_bn_frozen', 'BN_FROZEN_FUSE') and not any(p.requires_grad for p in self.parameters())

    def _train_fused_ok(self, x):
        """training with this block trainable and its norms frozen statistics (`norm_eval`): each BatchNorm (+ residual) + ReLU behind a
        convolution is one differentiable pass (`bn_act_train`) on contiguous fp32 CUDA tensors (`fuse_bn_train` attribute, or
        ORP_BN_TRAIN_FUSE=0 for A/B timing: off gives the stock modules).  Not under autocast (16-bit convolution outputs), not with
        checkpointing."""
        return torch.is_grad_enabled() and not torch.is_autocast_enabled() and x.is_cuda and x.dtype == torch.float32 and \
            x.dim() == 4 and x.is_contiguous() and not getattr(self, 'with_cp', False) and self._norms_are_eval_bn() and \
            switches.of(self, 'fuse_bn_train', 'BN_TRAIN_FUSE')

    def route(self, x):
        """the route `forward` takes for x: 'fused' (inference kernels, gradients disabled), 'frozen' (the same, in a training step's
        frozen stage), 'train' (differentiable fused passes) or 'stock' (the modules as written)"""
        if self._fused_ok(x):
            return 'fused'
        if self._frozen_ok(x):
            return 'frozen'
        if self._train_fused_ok(x):
            return 'train'
        return 'stock'

    def _forward_train_fused(self, x):
        from ..mmdet_ops.fused_norm import bn_act_train
        out = bn_act_train(self.conv1(x).contiguous(), self.bn1, relu=True)
        out = bn_act_train(self.conv2(out).contiguous(), self.bn2, relu=True)
        out = self.conv3(out).contiguous()
        ds = self.downsample
        if ds is not None:
            # the downsample BatchNorm rides in the block's last pass, forward and backward
            return bn_act_train(out, self.bn3, residual=ds[0](x).contiguous(), residual_bn=ds[1], relu=True)
        return bn_act_train(out, self.bn3, residual=x, relu=True)

    def _downsample_norm_fusable(self):
        """the identity branch is exactly Sequential(Conv2d, eval-mode BatchNorm2d) and the fusion is not switched off
        (`fuse_downsample_norm` attribute, or ORP_BN_DOWNSAMPLE_FUSE=0 for A/B timing)"""
        return switches.of(self, 'fuse_downsample_norm', 'BN_DOWNSAMPLE_FUSE') and self._downsample_is_conv_norm()

    def _downsample_is_conv_norm(self):
        ds = self.downsample
        return isinstance(ds, nn.Sequential) and len(ds) == 2 and isinstance(ds[0], nn.Conv2d) and \
            isinstance(ds[1], nn.BatchNorm2d) and not ds[1].training

    def _conv1x1_fusable(self):
        """conv1 / conv3 may run with their BatchNorm (+ residual) + ReLU in the convolution's epilogue where that was measured
        faster (`fuse_conv1x1` attribute, or ORP_BN_CONV1X1_FUSE=0 for A/B timing); the shapes are decided by
        `conv1x1_bn_act` (`orp_conv1x1_bn_act_pays`)"""
        return switches.of(self, 'fuse_conv1x1', 'BN_CONV1X1_FUSE')

    def _conv1x1_pieces_on(self):
        """where conv1 / conv3 run fused, the bf16-pieces kernel may take them at the shapes `orp_conv1x1_bn_act_pieces_pays` lists
        (`fuse_conv1x1_pieces` attribute, or ORP_BN_CONV1X1_PIECES=0 for A/B timing: off gives the launches of before)"""
        return switches.of(self, 'fuse_conv1x1_pieces', 'BN_CONV1X1_PIECES')

    def _downsample_conv_fusable(self):
        """where conv3 runs on the bf16-pieces kernel, the downsample convolution (and with it its BatchNorm, whatever
        `_downsample_norm_fusable` says: the launch has no form without it) may be contracted inside that launch at the shapes
        `orp_conv1x1_bn_act_pieces_dual_pays` lists (`fuse_downsample_conv` attribute, or ORP_BN_DOWNSAMPLE_CONV_FUSE=0 for A/B
        timing: off gives the launches and bits of before)"""
        return switches.of(self, 'fuse_downsample_conv', 'BN_DOWNSAMPLE_CONV_FUSE')

    def _conv3x3_fusable(self, kind='act'):
        """conv2 may run on the fused fp16-pieces kernel `kind` of `fused_norm.CONV3X3_KERNELS` -- bn2 + ReLU in its epilogue -- where
        that was measured faster: the kernel's block attribute (`fuse_conv3x3`, `fuse_conv3x3_deep`, `fuse_conv3x3_s2`) or its switch
        (ORP_BN_CONV3X3_FUSE / _DEEP_FUSE / _S2_FUSE = 0 for A/B timing: off gives the launches and bits of before).  The shapes are
        decided by the kernel's `ok` / `pays`; its force attribute (`force_conv3x3`..., tests) routes every supported shape.  One
        kernel's attributes do not touch another's."""
        from ..mmdet_ops.fused_norm import conv3x3_kernel
        k = conv3x3_kernel(kind)
        return switches.of(self, k.fuse_attr, k.switch) and not self.conv2_is_dcn and \
            isinstance(self.bn2, nn.BatchNorm2d) and not self.bn2.training

    _conv3x3_deep_fusable = functools.partialmethod(_conv3x3_fusable, 'deep')
    _conv3x3_s2_fusable = functools.partialmethod(_conv3x3_fusable, 's2')

    def _conv3x3_forced(self, kind):
        from ..mmdet_ops.fused_norm import conv3x3_kernel
        return bool(getattr(self, conv3x3_kernel(kind).force_attr, False))

    def _forward_fused(self, x):
        from ..mmdet_ops.fused_norm import bn_act, conv1x1_bn_act, conv3x3_bn_route, _conv3x3_launch, conv1x1_bn_act_dual, \
            conv1x1_bn_act_dual_routed
        fuse = self._conv1x1_fusable()
        pieces = None if self._conv1x1_pieces_on() else False       # (None: conv1x1_bn_act asks its table)

        def conv_bn_act(t, conv, bn, **kw):
            # conv1 / conv3: where the fused kernel pays, the raw convolution output is never written; everywhere else (and with
            # the switch off) the library's convolution and the pass.  conv2 stays on the library where its own kernel does not pay.
            if fuse:
                return conv1x1_bn_act(t, conv, bn, pieces=pieces, **kw)
            return bn_act(conv(t).contiguous(), bn, **kw)
        kind = None
        if tuple(self.conv1.stride) == (1, 1):
            # conv2's kernel -- the first of the table that says yes -- is decided in front of conv1 (whose output has x's positions),
            # so that conv1's kernel leaves the range word conv2 reads
            kind = conv3x3_bn_route(x, self.conv2, self.bn2, (x.size(0), self.conv1.out_channels, x.size(2), x.size(3)),
                                    self._conv3x3_fusable, self._conv3x3_forced)
        if kind is not None:
            out, bits = conv_bn_act(x, self.conv1, self.bn1, relu=True, want_range=True)
            out = _conv3x3_launch(kind, out, self.conv2, self.bn2, relu=True, force=self._conv3x3_forced(kind), range_bits=bits)
        else:
            out = conv_bn_act(x, self.conv1, self.bn1, relu=True)
            out = bn_act(self.conv2(out).contiguous(), self.bn2, relu=True)
        ds = self.downsample
        if fuse and pieces is None and self._downsample_conv_fusable() and self._downsample_is_conv_norm() and \
                conv1x1_bn_act_dual_routed(out, self.conv3, self.bn3, x, ds[0], ds[1]):
            # where it was measured faster the whole identity branch rides in conv3's launch: the downsample convolution is
            # contracted in front of conv3 by the same workgroups, its output never written.  Not under ORP_BN_DOWNSAMPLE_FUSE: with
            # that switch on or off the block has the same bits, as it had before this launch existed
            return conv1x1_bn_act_dual(out, self.conv3, self.bn3, x, ds[0], ds[1], relu=True)
        if self._downsample_norm_fusable():
            # the downsample BatchNorm rides in the block's last pass: no read-modify-write pass of its own over the identity
            residual, residual_bn = ds[0](x).contiguous(), ds[1]
        elif ds is not None:
            residual, residual_bn = bn_act(ds[0](x).contiguous(), ds[1], relu=False), None
        else:
            residual, residual_bn = x.contiguous(), None
        return conv_bn_act(out, self.conv3, self.bn3, residual=residual, residual_bn=residual_bn, relu=True)

    def forward(self, x):
        route = self.route(x)
        if route == 'fused':
            return self._forward_fused(x)
        if route == 'frozen':
            with torch.no_grad():       # nothing here has a gradient: the result requires none, as on the stock route
                return self._forward_fused(x)
        if route == 'train':
            return self._forward_train_fused(x)
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


@BACKBONES.register_module
class ResNet(nn.Module):
    arch_settings = {50: (Bottleneck, (3, 4, 6, 3)), 101: (Bottleneck, (3, 4, 23, 3)), 152: (Bottleneck, (3, 8, 36, 3))}

    def __init__(self, depth, in_channels=3, num_stages=4, strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1),
                 out_indices=(0, 1, 2, 3), style='pytorch', frozen_stages=-1, conv_cfg=None,
                 norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), gcb=None, stage_with_gcb=None, gen_attention=None,
                 stage_with_gen_attention=None, with_cp=False, zero_init_residual=True):
        super(ResNet, self).__init__()
        if depth not in self.arch_settings:
            raise KeyError('invalid depth {} for resnet'.format(depth))
        assert gcb is None and gen_attention is None, 'context / attention blocks are not part of the DOTA configs'
        assert conv_cfg is None, 'the backbone convolutions are stock nn.Conv2d (dcn= selects the deformable conv2)'
        # one private copy per model build: the blocks pop 'fallback_on_stride' from the dict they share (the reference's pop-once
        # semantics, which decide the checkpoint's conv_offset key set) -- the CALLER's config object is left as it was, so a second
        # backbone built from the same config sees the flag again (round-5 advisor)
        self.dcn = dict(dcn) if dcn is not None else None
        self.stage_with_dcn = tuple(stage_with_dcn) if stage_with_dcn is not None else (False,) * num_stages
        if dcn is not None:
            assert len(self.stage_with_dcn) == num_stages
        self.depth, self.num_stages, self.out_indices = depth, num_stages, out_indices
        self.frozen_stages, self.norm_eval = frozen_stages, norm_eval
        self.zero_init_residual = zero_init_residual
        block, stage_blocks = self.arch_settings[depth]
        self.conv1 = nn.Conv2d(in_channels, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.add_module('bn1', build_norm_layer(norm_cfg, 64)[1])
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        inplanes = 64
        self.res_layers = []
        for i, num_blocks in enumerate(stage_blocks[:num_stages]):
            planes = 64 * 2 ** i
            stride, dilation = strides[i], dilations[i]
            downsample = None
            if stride != 1 or inplanes != planes * block.expansion:
                downsample = nn.Sequential(
                    nn.Conv2d(inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                    build_norm_layer(norm_cfg, planes * block.expansion)[1])
            stage_dcn = self.dcn if (self.dcn is not None and self.stage_with_dcn[i]) else None
            layers = [block(inplanes, planes, stride, dilation, downsample, style, norm_cfg, stage_dcn)]
            inplanes = planes * block.expansion
            for _ in range(1, num_blocks):
                layers.append(block(inplanes, planes, 1, dilation, None, style, norm_cfg, stage_dcn))
            name = 'layer{}'.format(i + 1)
            self.add_module(name, nn.Sequential(*layers))
            self.res_layers.append(name)
        self._freeze_stages()
        self.feat_dim = inplanes

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.bn1.eval()
            for m in [self.conv1, self.bn1]:
                for param in m.parameters():
                    param.requires_grad = False
        for i in range(1, self.frozen_stages + 1):
            m = getattr(self, 'layer{}'.format(i))
            m.eval()
            for param in m.parameters():
                param.requires_grad = False

    def init_weights(self, pretrained=None):
        """`pretrained`: a local checkpoint file, or a model-zoo URI of the reference configs ('torchvision://resnet50',
        'open-mmlab://...').  There is no network here: a URI is resolved through the environment variable
        ORP_PRETRAINED_DIR (<dir>/<name>.pth) and, when no such file exists, a warning says that the backbone -- whose
        stem and layer1 the DOTA configs FREEZE -- stays at its random initialisation."""
        if isinstance(pretrained, str):
            import os
            import warnings
            path = pretrained
            if '://' in pretrained:
                name = pretrained.split('://', 1)[1].replace('/', '_')
                root = os.environ.get('ORP_PRETRAINED_DIR', '')
                path = os.path.join(root, name + '.pth') if root else ''
            if path and os.path.isfile(path):
                sd = torch.load(path, map_location='cpu')
                sd = sd.get('state_dict', sd)
                missing, unexpected = self.load_state_dict(sd, strict=False)
                unexpected = [k for k in unexpected if not k.startswith('fc.')]      # the classifier head is not part of it
                if missing or unexpected:
                    warnings.warn('ResNet.init_weights(%r): missing keys %s, unexpected keys %s'
                                  % (pretrained, list(missing)[:8], unexpected[:8]))
                return
            warnings.warn('ResNet.init_weights: pretrained=%r was NOT loaded (no such file%s); the backbone keeps its '
                          'random initialisation, frozen_stages=%d of it frozen'
                          % (pretrained, '' if '://' not in pretrained else '; set ORP_PRETRAINED_DIR', self.frozen_stages))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                kaiming_init(m)
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                constant_init(m, 1)
        if self.dcn is not None:                                      # resnet.py:478-482: offsets (and masks) start at zero
            for m in self.modules():
                if isinstance(m, Bottleneck) and hasattr(m.conv2, 'conv_offset'):
                    constant_init(m.conv2.conv_offset, 0)
        if self.zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    constant_init(m.bn3, 0)

    def _stem_pool_fusable(self):
        """`maxpool` is exactly MaxPool2d(3, 2, 1) -- dilation 1, floor mode, no indices -- and the fusion is not switched off
        (`fuse_stem_pool` attribute, or ORP_STEM_POOL_FUSE=0 for A/B timing)"""
        from ..mmdet_ops.fused_norm import is_maxpool_3_2_1
        return switches.of(self, 'fuse_stem_pool', 'STEM_POOL_FUSE') and is_maxpool_3_2_1(self.maxpool)

    def stem_route(self, x):
        """the route `forward` takes through the stem for x: 'fused' (inference kernels, gradients disabled), 'frozen' (the same in a
        training step whose stem is frozen -- neither conv1 / bn1 nor the image requires a gradient; `fuse_bn_frozen` attribute, or
        ORP_BN_FROZEN_FUSE=0 for A/B timing; not under autocast) or 'stock'"""
        if not (x.is_cuda and x.dtype == torch.float32 and isinstance(self.bn1, nn.BatchNorm2d) and not self.bn1.training):
            return 'stock'
        if not torch.is_grad_enabled():
            return 'fused'
        if not torch.is_autocast_enabled() and not x.requires_grad and switches.of(self, 'fuse_bn_frozen', 'BN_FROZEN_FUSE') and \
                not any(p.requires_grad for m in (self.conv1, self.bn1) for p in m.parameters()):
            return 'frozen'
        return 'stock'

    def _forward_stem_fused(self, x):
        from ..mmdet_ops.fused_norm import bn_act, bn_relu_maxpool, stem_conv_bn_relu_maxpool, stem_conv_routed
        # the whole stem as one launch (`fuse_stem_conv` attribute, or ORP_STEM_CONV_FUSE=0 for A/B timing) at the shapes where it was
        # measured faster; `force_stem_conv` (attribute, tests) routes every supported shape
        if switches.of(self, 'fuse_stem_conv', 'STEM_CONV_FUSE') and \
                stem_conv_routed(x, self.conv1, self.bn1, self.maxpool, bool(getattr(self, 'force_stem_conv', False))):
            return stem_conv_bn_relu_maxpool(x, self.conv1, self.bn1)
        if self._stem_pool_fusable():
            return bn_relu_maxpool(self.conv1(x).contiguous(), self.bn1)      # BatchNorm + ReLU applied while pooling
        return self.maxpool(bn_act(self.conv1(x).contiguous(), self.bn1, relu=True))

    def forward(self, x):
        route = self.stem_route(x)
        if route == 'fused':
            x = self._forward_stem_fused(x)
        elif route == 'frozen':
            with torch.no_grad():       # nothing in the stem has a gradient: the result requires none, as on the stock route
                x = self._forward_stem_fused(x)
        else:
            x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        outs = []
        for i, name in enumerate(self.res_layers):
            x = getattr(self, name)(x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)

    def train(self, mode=True):
        super(ResNet, self).train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, nn.modules.batchnorm._BatchNorm):
                    m.eval()
