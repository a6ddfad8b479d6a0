"""GPU: the glue passes fused away in the backbone and the FPN compute the bits of the launch sequences they replace.

Three launches -- the block-final pass with the downsample BatchNorm folded in (orp_affine2_act), the stem's BatchNorm + ReLU inside
its max-pool (orp_affine_relu_maxpool), the FPN's lateral GroupNorm + top-down sum + transposition (orp_fpn_topdown_nhwc) -- each
against the separate launches on the same inputs, as int32 views (NaN positions count); the call sites' fall-backs; and the whole
R-50 detector with all three switches off against all three on."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()            # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _bn(c, dev, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.3)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.5)
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.3)
    return bn.to(dev).eval()


def _salt(x, seed):
    """+-inf, NaN, zeros of both signs and magnitudes that underflow to a signed zero behind a scale, at scattered positions"""
    g = torch.Generator().manual_seed(seed)
    flat = x.view(-1)
    vals = [float('inf'), float('-inf'), float('nan'), 0.0, -0.0, 1e-45, -1e-45, -1e-38, 3e38, -3e38]
    idx = torch.randperm(flat.numel(), generator=g)[:50 * len(vals)].to(x.device)
    for k, v in enumerate(vals):
        flat[idx[k::len(vals)]] = v
    return x


# the backbone's planes at a 1024 x 1024 image (B = 1): stage outputs, i.e. what a stage's first block ends in
R50_STAGE_PLANES = [(1, 256, 256, 256), (1, 512, 128, 128), (1, 1024, 64, 64), (1, 2048, 32, 32)]


@pytest.mark.parametrize("shape,salted", [(s, False) for s in R50_STAGE_PLANES] +
                         [((2, 24, 7, 9), False), ((2, 24, 7, 9), True), ((1, 64, 40, 36), True), ((3, 5, 1, 1), True)])
@pytest.mark.parametrize("relu", [True, False])
def test_block_final_pass_with_downsample_affine(dev, shape, salted, relu):
    """bn_act(out, bn3, residual=raw, residual_bn=bn_ds) == bn_act(raw, bn_ds, relu=False) then bn_act(out, bn3, residual=.)"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act
    torch.manual_seed(11)
    x = torch.randn(shape, device=dev) * 2
    r = torch.randn(shape, device=dev) * 2 + 0.5
    if salted:
        _salt(x, 1); _salt(r, 2)
    bn3, bnd = _bn(shape[1], dev, 3), _bn(shape[1], dev, 4)
    if salted:
        with torch.no_grad():
            bnd.bias.copy_(bnd.running_mean * bnd.weight * torch.rsqrt(bnd.running_var + bnd.eps))   # shift ~ 0: tiny products survive
    with torch.no_grad():
        identity = bn_act(r.clone(), bnd, relu=False)
        want = bn_act(x.clone(), bn3, residual=identity, relu=relu)
        got = bn_act(x.clone(), bn3, residual=r.clone(), residual_bn=bnd, relu=relu)
    assert _same_bits(got, want)
    if not salted:
        with torch.no_grad():
            ref = bn3(x) + bnd(r)
            ref = torch.relu(ref) if relu else ref
        assert float((got - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))


def _bottleneck(dev, downsample, inplanes=64, planes=32):
    from orientedreppoints_amd.mmdet_models.resnet import Bottleneck
    torch.manual_seed(5)
    blk = Bottleneck(inplanes, planes, stride=2, downsample=downsample).to(dev).eval()
    for i, m in enumerate(m for m in blk.modules() if isinstance(m, torch.nn.BatchNorm2d)):
        src = _bn(m.num_features, dev, 20 + i)
        m.load_state_dict(src.state_dict())
    return blk


def test_bottleneck_switch_and_fallback(dev):
    """Bottleneck.forward with the fusion off and on: the same bits; a downsample branch that is not exactly conv + BatchNorm keeps
    the two passes (and matches as well)."""
    nn = torch.nn
    x = torch.randn(2, 64, 30, 22, device=dev)
    plain = nn.Sequential(nn.Conv2d(64, 128, 1, stride=2, bias=False), nn.BatchNorm2d(128))
    resnet_d = nn.Sequential(nn.Sequential(nn.AvgPool2d(2, 2), nn.Conv2d(64, 128, 1, bias=False)), nn.BatchNorm2d(128))
    for ds, fusable in ((plain, True), (resnet_d, False)):
        blk = _bottleneck(dev, ds)
        outs = {}
        with torch.no_grad():
            for flag in (False, True):
                blk.fuse_downsample_norm = flag
                assert blk._downsample_norm_fusable() == (flag and fusable)
                outs[flag] = blk(x.clone())
            del blk.fuse_downsample_norm
            assert blk._downsample_norm_fusable() == fusable            # default: on
            with torch.enable_grad():
                stock = blk(x.clone())                                  # autograd on: the unfused module path
        assert _same_bits(outs[True], outs[False])
        assert float((outs[True] - stock).abs().max()) <= 1e-4 * max(1.0, float(stock.abs().max()))


@pytest.mark.parametrize("shape,salted", [((1, 64, 512, 512), False), ((1, 64, 512, 512), True), ((2, 5, 37, 41), True),
                                          ((2, 3, 16, 18), True), ((1, 4, 9, 8), True), ((1, 2, 1, 1), True), ((1, 2, 2, 5), True),
                                          ((1, 3, 64, 2048), False)])
def test_stem_affine_relu_maxpool(dev, shape, salted):
    """bn_relu_maxpool(x, bn) == MaxPool2d(3, 2, 1)(bn_act(x, bn, relu=True)): the stem plane at 1024 x 1024, odd H and W, W that is
    not a multiple of 4, maps smaller than a window, inputs salted with +-inf / NaN / signed zeros."""
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act, bn_relu_maxpool
    torch.manual_seed(12)
    x = torch.randn(shape, device=dev) * 2
    if salted:
        _salt(x, 6)
    bn = _bn(shape[1], dev, 7)
    if salted:
        with torch.no_grad():
            bn.bias.copy_(bn.running_mean * bn.weight * torch.rsqrt(bn.running_var + bn.eps))       # shift ~ 0
    keep = x.clone()
    with torch.no_grad():
        want = torch.nn.MaxPool2d(3, 2, 1)(bn_act(x.clone(), bn, relu=True))
        got = bn_relu_maxpool(x, bn)
    assert _same_bits(x, keep), "the input is left as it was"
    assert got.is_contiguous() and _same_bits(got, want)


def test_stem_switch_and_fallback(dev):
    """ResNet.forward with the stem fusion off and on: the same bits; a max-pool that is not MaxPool2d(3, 2, 1) in floor mode
    (ceil_mode=True) keeps the two launches, also at an input where ceil mode changes the output size."""
    from orientedreppoints_amd.mmdet_models.resnet import ResNet
    torch.manual_seed(8)
    net = ResNet(50, num_stages=1, out_indices=(0,)).to(dev)
    net.eval()
    net.bn1.load_state_dict(_bn(64, dev, 9).state_dict())
    x = torch.randn(1, 3, 76, 68, device=dev)              # conv1 output 38 x 34: floor mode 19 x 17, ceil mode 20 x 18
    with torch.no_grad():
        outs = {}
        for flag in (False, True):
            net.fuse_stem_pool = flag
            assert net._stem_pool_fusable() == flag
            outs[flag] = net(x)[0]
        assert _same_bits(outs[True], outs[False])
        net.maxpool = torch.nn.MaxPool2d(3, 2, 1, ceil_mode=True)
        ceil = {}
        for flag in (False, True):
            net.fuse_stem_pool = flag
            assert not net._stem_pool_fusable()
            ceil[flag] = net(x)[0]
        assert _same_bits(ceil[True], ceil[False]) and ceil[True].shape != outs[True].shape


def _gn(c, dev, seed):
    g = torch.Generator().manual_seed(seed)
    gn = torch.nn.GroupNorm(32, c)
    with torch.no_grad():
        gn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        gn.bias.copy_(torch.randn(c, generator=g) * 0.3)
    return gn.to(dev)


def _topdown_parent(raws, gns):
    """the launch sequence fpn_topdown_cl replaces"""
    import torch.nn.functional as F
    from orientedreppoints_amd.mmdet_ops.fused_norm import group_norm_act_multi, to_channels_last_multi
    lat = group_norm_act_multi([r.clone() for r in raws], gns, relu=False, inplace=True)
    for i in range(len(lat) - 1, 0, -1):
        lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode='nearest')
    return to_channels_last_multi(lat, amax_slots=[0] * len(lat))


@pytest.mark.parametrize("batch,sizes", [(1, ((128, 128), (64, 64), (32, 32))), (2, ((40, 56), (20, 28), (10, 14))),
                                         (2, ((12, 8), (6, 4), (3, 2))), (1, ((24, 16), (12, 8), (6, 4), (3, 2))), (2, ((36, 20), (18, 10))),
                                         (1, ((5, 7),))])
def test_fpn_topdown_launch(dev, batch, sizes):
    """fpn_topdown_cl == GroupNorm of every lateral, interpolate + add from the coarsest level down, transposition: the output
    bits of every level and the range word; the R-50 levels at 1024 x 1024, three levels with batch 2, tiles that hang over."""
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.fused_norm import fpn_topdown_cl, fpn_topdown_ok
    torch.manual_seed(13)
    raws = [torch.randn(batch, 256, h, w, device=dev) * (1.5 + i) + 0.25 * i for i, (h, w) in enumerate(sizes)]
    gns = [_gn(256, dev, 30 + i) for i in range(len(sizes))]
    keep = [r.clone() for r in raws]
    with torch.no_grad():
        want, want_bits = _topdown_parent(raws, gns)
        assert fpn_topdown_ok(raws, gns)
        got, got_bits = fpn_topdown_cl(raws, gns)
    for r, k in zip(raws, keep):
        assert _same_bits(r, k), "the raw laterals are left as they were"
    for g, w in zip(got, want):
        assert g.is_contiguous(memory_format=torch.channels_last) and g.shape == w.shape
        assert np.array_equal(_bits(g.permute(0, 2, 3, 1)), _bits(w.permute(0, 2, 3, 1)))
    assert _lib.lib().orp_dcn_get_split_mode() != 3 or want_bits is not None
    assert (got_bits is None) == (want_bits is None)
    if want_bits is not None:
        assert np.array_equal(got_bits.cpu().numpy(), want_bits.cpu().numpy())
        assert float(got_bits.view(torch.float32)[0]) == max(float(g.abs().max()) for g in got)


def _neck(dev):
    from orientedreppoints_amd.dota_configs import r50_model
    from orientedreppoints_amd.mmdet_models import ConfigDict
    from orientedreppoints_amd.mmdet_models.registry import build_neck
    torch.manual_seed(14)
    neck = build_neck(ConfigDict(r50_model['neck'])).to(dev).eval()
    neck.init_weights()
    for i, m in enumerate(m for m in neck.modules() if isinstance(m, torch.nn.GroupNorm)):
        m.load_state_dict(_gn(m.num_channels, dev, 40 + i).state_dict())
    return neck


@pytest.mark.parametrize("batch,sizes,fusable", [(1, (256, 128, 64, 32), True), (2, (48, 24, 12, 6), True), (2, (50, 25, 13, 7), False)])
def test_fpn_switch_and_fallback(dev, batch, sizes, fusable):
    """FPN.forward with the top-down fusion off and on: every output level and the range hand-over are the same bits; levels that
    are not exactly twice the next (25 -> 13 -> 7) keep the separate launches."""
    neck = _neck(dev)
    torch.manual_seed(15)
    feats = [torch.randn(batch, c, n, n, device=dev) for c, n in zip((256, 512, 1024, 2048), sizes)]
    res = {}
    with torch.no_grad():
        raw = [lc.conv(feats[i + neck.start_level]) for i, lc in enumerate(neck.lateral_convs)]
        for flag in (False, True):
            neck.fuse_topdown = flag
            assert neck._topdown_ok(raw) == (flag and fusable)
            res[flag] = neck([f.clone() for f in feats])
        del neck.fuse_topdown
        assert neck._topdown_ok(raw) == fusable                        # default: on
    assert len(res[True]) == len(res[False]) == 5
    for a, b in zip(res[True], res[False]):
        assert a.shape == b.shape and a.stride() == b.stride()
        assert np.array_equal(_bits(a.permute(0, 2, 3, 1)), _bits(b.permute(0, 2, 3, 1)))
    assert (res[True].orp_amax is None) == (res[False].orp_amax is None)
    if res[True].orp_amax is not None:
        assert np.array_equal(res[True].orp_amax.cpu().numpy(), res[False].orp_amax.cpu().numpy())


def test_detector_at_1024_is_unchanged_by_the_three_fusions(dev):
    """build_detector(r50_model) in eval mode on a seeded 1024 x 1024 image, all three switches off against all three on: backbone
    outputs and FPN outputs bit for bit, simple_test detections array_equal -- under torch.backends.cudnn.deterministic so that
    the stock convolutions are themselves reproducible."""
    from orientedreppoints_amd import switches
    from orientedreppoints_amd.dota_configs import r50_model, test_cfg
    from orientedreppoints_amd.mmdet_models import ConfigDict, build_detector
    torch.manual_seed(0)
    model = build_detector(ConfigDict(r50_model), train_cfg=None, test_cfg=ConfigDict(test_cfg)).to(dev).eval()
    head = model.bbox_head
    with torch.no_grad():
        head.reppoints_cls_out.weight.normal_(0, 0.05)
        head.reppoints_cls_out.bias.fill_(-3.0)
    for i, m in enumerate(m for m in model.backbone.modules() if isinstance(m, torch.nn.BatchNorm2d)):
        m.load_state_dict(_bn(m.num_features, dev, 100 + i).state_dict())
    img = torch.randn(1, 3, 1024, 1024, device=dev)
    metas = [dict(img_shape=(1024, 1024, 3), pad_shape=(1024, 1024, 3), scale_factor=1.0, flip=False)]
    names = ('BN_DOWNSAMPLE_FUSE', 'STEM_POOL_FUSE', 'FPN_TOPDOWN_FUSE')
    saved = {n: getattr(switches, n) for n in names}
    saved_det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    res = {}
    try:
        with torch.no_grad():
            for flag in (False, True):
                for n in names:
                    setattr(switches, n, flag)
                c = model.backbone(img)
                p = model.neck(c)
                res[flag] = ([t.clone() for t in c], [t.clone() for t in p], model.simple_test(img, metas))
    finally:
        torch.backends.cudnn.deterministic = saved_det
        for n in names:
            setattr(switches, n, saved[n])
    assert all(saved.values()), "the three fusions are on by default"
    for a, b in zip(res[True][0], res[False][0]):
        assert _same_bits(a, b)
    for a, b in zip(res[True][1], res[False][1]):
        assert a.shape == b.shape and np.array_equal(_bits(a.permute(0, 2, 3, 1)), _bits(b.permute(0, 2, 3, 1)))
    assert sum(len(d) for d in res[True][2]) > 100
    for a, b in zip(res[True][2], res[False][2]):
        assert a.shape == b.shape and np.array_equal(a, b)
