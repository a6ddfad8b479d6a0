"""GPU (MI355X): the backbone's training route -- `orp_affine_act_backward` / `orp_affine2_act_backward`, `bn_act_train`, the
differentiable and the frozen route of `Bottleneck` / `ResNet` -- against the float64 statement of tests/bn_train_cases.py.

The elementwise outputs are one multiply or a copy: equal to the statement rounded once.  The channel sums are held two ways: exactly
(integer data: a dropped, doubled or misindexed element shows whatever the order of summation) and on N(0, 1) data around means of up
to +-50 against the stock route's own error on the same tensors.  The backward launches the forward's grid, so the shapes are the
forward's edges (bn_train_cases.SHAPES).  Measured on MI355X (profiles/r27_gputest_bn_train.log has every line the tests report)."""
import copy
import ctypes
import types

import numpy as np
import pytest

import bn_train_cases as K
import conftest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
F = torch.nn.functional

SENTINEL = 7.25
FLOOR = 8 * 2.0 ** -24           # a few roundings of the result


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()            # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _guarded(shape, dev):
    """an output of this shape filled with a sentinel, with 64 sentinel floats behind it: (view, whole buffer)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), SENTINEL, dtype=torch.float32, device=dev)
    return buf[:n].view(shape), buf


def _tail_intact(buf, n):
    return bool((buf[n:] == SENTINEL).all())


def _raw_backward(dev, d, relu, res, want, alias, hw=None, ws_bytes=None, drop=()):
    """one call of the C entry on the arrays of a case; returns (rc, outputs as numpy, every guarded buffer intact behind its end).
    hw / ws_bytes / drop (argument names passed as NULL) override what is passed: the refused-argument cases."""
    from orientedreppoints_amd import _lib
    L = _lib.lib()
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    shape = tuple(t['grad_y'].shape)
    B, C, H, W = shape
    n = B * C * H * W
    two = res == 'affine2'
    outs, bufs = {}, {}

    def out(name, shp):
        outs[name], bufs[name] = _guarded(shp, dev)
        return outs[name]
    gy = t['grad_y'].clone()
    gx = out('grad_x', shape)
    gx2 = out('grad_x2', shape) if two else None
    gres = None
    if res == 'plain':
        gres = gy if alias else out('grad_res', shape)
    dw = out('dweight', (C,)) if want else None
    db = out('dbias', (C,)) if want else None
    dw2 = out('dweight2', (C,)) if (want and two) else None
    db2 = out('dbias2', (C,)) if (want and two) else None
    nbytes = L.orp_affine_act_backward_workspace_bytes(B, C, H * W) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    a = dict(grad_y=gy, y=t['y'] if relu else None, x=t['x'] if want else None, scale=t['scale'], mean=t['mean'], rstd=t['rstd'],
             x2=t['x2'] if (want and two) else None, scale2=t['scale2'] if two else None, mean2=t['mean2'] if two else None,
             rstd2=t['rstd2'] if two else None, grad_x=gx, grad_x2=gx2, grad_res=gres, dweight=dw, dbias=db, dweight2=dw2, dbias2=db2)
    for k in drop:
        a[k] = None
    p = {k: _lib.ptr(v) for k, v in a.items()}
    dims = (B, C, H * W if hw is None else hw, _lib.ptr(ws), ctypes.c_size_t(nbytes), _lib.stream_of(gy))
    with torch.cuda.device(dev):
        if two:
            rc = L.orp_affine2_act_backward(p['grad_y'], p['y'], p['x'], p['scale'], p['mean'], p['rstd'], p['x2'], p['scale2'], p['mean2'],
                                            p['rstd2'], p['grad_x'], p['grad_x2'], p['grad_res'], p['dweight'], p['dbias'], p['dweight2'],
                                            p['dbias2'], *dims)
        else:
            rc = L.orp_affine_act_backward(p['grad_y'], p['y'], p['x'], p['scale'], p['mean'], p['rstd'], p['grad_x'], p['grad_res'],
                                           p['dweight'], p['dbias'], *dims)
    torch.cuda.synchronize()
    intact = all(_tail_intact(bufs[k], outs[k].numel()) for k in outs)
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    if res == 'plain' and alias:
        got['grad_res'] = gy.cpu().numpy()
    return rc, got, intact


def _round32(a):
    return np.asarray(a, np.float64).astype(np.float32)


@pytest.mark.parametrize("shape", K.SHAPES)
def test_backward_exact(dev, shape):
    """integer data: every elementwise output equals the statement rounded once, every channel sum equals it exactly, the call twice
    gives the same bits, nothing is written behind an output -- for every (ReLU, residual form, dweight wanted, aliasing) case"""
    d = K.exact_case(shape, 3)
    for relu, res, want, alias in K.op_cases():
        two = res == 'affine2'
        rc, got, intact = _raw_backward(dev, d, relu, res, want, alias)
        assert rc == 0 and intact, (relu, res, want, alias, rc)
        w = K.backward_f64(d['grad_y'], d['scale'], y=d['y'] if relu else None, x=d['x'], mean=d['mean'], rstd=d['rstd'],
                           scale2=d['scale2'] if two else None, x2=d['x2'] if two else None, mean2=d['mean2'], rstd2=d['rstd2'])
        names = ['grad_x'] + (['grad_res'] if res == 'plain' else []) + (['grad_x2'] if two else [])
        if want:
            names += ['dweight', 'dbias'] + (['dweight2', 'dbias2'] if two else [])
        assert sorted(names) == sorted(got)
        for k in names:
            exp = _round32(w['dbias'] if k == 'dbias2' else w[k])
            assert np.array_equal(got[k], exp), (relu, res, want, alias, k, float(np.max(np.abs(got[k] - exp))))
        rc2, again, _ = _raw_backward(dev, d, relu, res, want, alias)
        assert rc2 == 0 and all(np.array_equal(got[k].view(np.int32), again[k].view(np.int32)) for k in names)


def _bn_of(d, s, dev, trainable):
    C = d['weight' + s].shape[0]
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(d['weight' + s])); bn.bias.copy_(torch.from_numpy(d['bias' + s]))
        bn.running_mean.copy_(torch.from_numpy(d['running_mean' + s])); bn.running_var.copy_(torch.from_numpy(d['running_var' + s]))
    bn = bn.to(dev).eval()
    for p in bn.parameters():
        p.requires_grad = trainable
    return bn


def _grads(y, gy, leaves):
    gs = torch.autograd.grad(y, [t for t in leaves if t is not None], gy, retain_graph=True, allow_unused=True)
    it = iter(gs)
    return [next(it) if t is not None else None for t in leaves]


@pytest.mark.parametrize("shape", K.SHAPES)
def test_bn_act_train_random(dev, shape):
    """N(0, 1) data around channel means of up to +-50 through `bn_act_train`: the forward is `bn_act` on a copy bit for bit; grad_x /
    grad_res / grad_x2 equal the statement rounded once; |dweight - statement| / sum |terms| (and dbias's) stay within twice the same
    figure of torch's eval-mode batch_norm backward on the same GPU tensors, or 8 * 2^-24 (a few roundings of the result), whichever is
    larger -- both are fp32 reductions of the same terms in different orders: equally good, not equal; the backward twice gives equal
    bits; a BatchNorm whose parameters want no gradient returns none."""
    from orientedreppoints_amd.mmdet_ops.fused_norm import _bn_affine_stats, bn_act, bn_act_train
    d = K.random_case(shape, 5)
    worst = {}
    for relu, res, want, alias in K.op_cases():
        if alias:                    # (aliasing is the C entry's business: test_backward_exact)
            continue
        two = res == 'affine2'
        bn, bn2 = _bn_of(d, '', dev, want), _bn_of(d, '2', dev, want)
        gy = torch.from_numpy(d['grad_y']).to(dev)
        x = torch.from_numpy(d['x']).to(dev).requires_grad_()
        r = None if res == 'none' else torch.from_numpy(d['x2'] if two else d['residual']).to(dev).requires_grad_()
        y = bn_act_train(x, bn, residual=r, relu=relu, residual_bn=bn2 if two else None)
        with torch.no_grad():
            ref = bn_act(x.detach().clone(), bn, residual=None if r is None else r.detach(), relu=relu, residual_bn=bn2 if two else None)
        assert torch.equal(y, ref) and y.data_ptr() != x.data_ptr()
        leaves = [x, r, bn.weight if want else None, bn.bias if want else None,
                  bn2.weight if (want and two) else None, bn2.bias if (want and two) else None]
        g = _grads(y, gy, leaves)
        g2 = _grads(y, gy, leaves)
        for u, v in zip(g, g2):
            assert (u is None) == (v is None) and (u is None or torch.equal(u.view(torch.int32), v.view(torch.int32)))
        # the stock route on the same tensors
        xs = x.detach().clone().requires_grad_()
        rs = None if r is None else r.detach().clone().requires_grad_()
        ys = F.batch_norm(xs, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0., bn.eps)
        if res == 'plain':
            ys = ys + rs
        elif two:
            ys = ys + F.batch_norm(rs, bn2.running_mean, bn2.running_var, bn2.weight, bn2.bias, False, 0., bn2.eps)
        if relu:
            ys = torch.relu(ys)
        gs = _grads(ys, gy, [xs, rs] + leaves[2:])
        scale, _shift, mean, rstd = [t.cpu().numpy() for t in _bn_affine_stats(bn)]
        scale2 = _bn_affine_stats(bn2)[0].cpu().numpy()
        rstd64 = 1. / np.sqrt(d['running_var'].astype(np.float64) + bn.eps)
        rstd64_2 = 1. / np.sqrt(d['running_var2'].astype(np.float64) + bn2.eps)

        def statement(yy):
            return K.backward_f64(d['grad_y'], scale, y=yy.detach().cpu().numpy() if relu else None, x=d['x'], mean=d['running_mean'],
                                  rstd=rstd64, scale2=scale2 if two else None, x2=d['x2'] if two else None, mean2=d['running_mean2'],
                                  rstd2=rstd64_2)
        w, wst = statement(y), statement(ys)
        assert np.array_equal(g[0].cpu().numpy(), _round32(w['grad_x']))
        if res == 'plain':
            assert np.array_equal(g[1].cpu().numpy(), _round32(w['grad_res']))
        if two:
            assert np.array_equal(g[1].cpu().numpy(), _round32(w['grad_x2']))
        if not want:
            continue
        for idx, key, absk in ((2, 'dweight', 'dweight_abs'), (3, 'dbias', 'dbias_abs')) + \
                (((4, 'dweight2', 'dweight2_abs'), (5, 'dbias', 'dbias_abs')) if two else ()):
            def rel(got, st):
                return float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - st[key]) / np.maximum(st[absk], 1e-300)))
            new, stock = rel(g[idx], w), rel(gs[idx], wst)
            name = key + ('' if idx < 5 else '2')
            pair = worst.get(name, (0., 0.))
            if new / max(2 * stock, FLOOR) >= pair[0] / max(2 * pair[1], FLOOR):
                worst[name] = (new, stock)
            print("bn_act_train %s relu=%d %s %s: |d| / sum |terms| fused %.3g, stock %.3g" % (shape, relu, res, name, new, stock))
            assert new <= max(2 * stock, FLOOR), (shape, relu, res, name, new, stock)
    conftest.REPORT.append("bn_act_train %s: worst |d| / sum |terms| (fused, stock) %s; floor %.3g"
                           % (shape, ", ".join("%s (%.3g, %.3g)" % (k, v[0], v[1]) for k, v in sorted(worst.items())), FLOOR))


def test_refused_arguments_raise_and_launch_nothing(dev):
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act_train
    d = K.exact_case((2, 3, 5, 7), 1)
    for kw in (dict(hw=0), dict(hw=-4), dict(ws_bytes=16), dict(drop=('x',)), dict(drop=('dbias',)), dict(drop=('mean',)),
               dict(drop=('grad_x',)), dict(drop=('scale',))):
        rc, got, intact = _raw_backward(dev, d, True, 'plain', True, False, **kw)
        assert rc == _lib.ORP_EINVAL, (kw, rc)
        assert intact and all(bool((v == SENTINEL).all()) for v in got.values()), kw      # nothing was launched
        with pytest.raises(_lib.OrpHipError):
            _lib.check(rc, "orp_affine_act_backward")
    rc, got, intact = _raw_backward(dev, d, True, 'affine2', True, False, drop=('x2',))
    assert rc == _lib.ORP_EINVAL and all(bool((v == SENTINEL).all()) for v in got.values())
    # without a dweight neither x nor a workspace is needed
    rc, got, intact = _raw_backward(dev, d, True, 'plain', False, False, ws_bytes=0)
    assert rc == 0 and intact
    # the Python entry: what it was not written for is a ValueError, not another route
    bn = torch.nn.BatchNorm2d(3).to(dev).eval()
    x = torch.randn(2, 3, 5, 7, device=dev)
    cl = x.to(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    for bad in (x.half(), x.bfloat16(), cl, x[:, :, ::2], x.cpu(), x[0]):
        with pytest.raises(ValueError):
            bn_act_train(bad, bn)
    with pytest.raises(ValueError):
        bn_act_train(x.double(), copy.deepcopy(bn).double())
    with pytest.raises(ValueError):
        bn_act_train(x, copy.deepcopy(bn).train())
    with pytest.raises(ValueError):
        bn_act_train(x, bn, residual=x[:, :, :4])
    with pytest.raises(ValueError):
        bn_act_train(x, bn, residual_bn=bn)
    with pytest.raises(ValueError):
        bn_act_train(x, torch.nn.BatchNorm2d(4).to(dev).eval())


# ---- module level ---------------------------------------------------------------------------------------------------------------

def _randomise_norms(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.weight.copy_(torch.rand(c, generator=g) + 0.5); m.bias.copy_(torch.randn(c, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(c, generator=g) * 0.3); m.running_var.copy_(torch.rand(c, generator=g) + 0.5)


def _set_switches(net, train, frozen):
    for m in net.modules():
        m.fuse_bn_train, m.fuse_bn_frozen = train, frozen


def _block_run(blk, x, gy):
    """(output, gradient of the input and of every parameter by name) of one forward + backward"""
    x = x.detach().clone().requires_grad_()
    for p in blk.parameters():
        p.grad = None
    y = blk(x)
    y.backward(gy)
    out = {'out': y.detach(), 'grad_input': x.grad}
    out.update({'grad ' + n: p.grad for n, p in blk.named_parameters()})
    return out


def _held_to_double(new, stock, ref, what):
    """per tensor: the new route's error against the float64 copy is within twice the stock route's, or 1e-6 of the tensor's max"""
    lines = []
    for k in ref:
        r = ref[k].double()
        en, es = float((new[k].double() - r).abs().max()), float((stock[k].double() - r).abs().max())
        floor = 1e-6 * float(r.abs().max())
        lines.append((k, en, es, floor))
        print("%s %s: max |err| fused %.3g, stock %.3g, floor %.3g" % (what, k, en, es, floor))
    for k, en, es, floor in lines:
        assert en <= max(2 * es, floor), (what, k, en, es, floor)
    k, en, es, floor = max(lines, key=lambda t: t[1] / max(2 * t[2], t[3], 1e-300))
    conftest.REPORT.append("%s: %d tensors; nearest its bound: %s, max |err| fused %.3g, stock %.3g, floor %.3g"
                           % (what, len(lines), k, en, es, floor))


@pytest.mark.parametrize("downsample", [False, True])
def test_bottleneck_train_route(dev, downsample):
    """one Bottleneck in train mode with eval-mode norms, 2 x C x 12 x 20 (planes 8; 32 input channels on the identity form, whose
    residual has the block's 4 * planes channels; 16 and a stride-2 downsample branch on the other): output and every gradient on the
    new route and on the stock route (attribute off), both against a float64 copy"""
    from orientedreppoints_amd.mmdet_models.resnet import Bottleneck
    torch.manual_seed(3)
    cin = 16 if downsample else 32
    ds = None
    if downsample:
        ds = torch.nn.Sequential(torch.nn.Conv2d(16, 32, 1, stride=2, bias=False), torch.nn.BatchNorm2d(32))
    blk = Bottleneck(cin, 8, stride=2 if downsample else 1, downsample=ds)
    _randomise_norms(blk, 4)
    blk = blk.to(dev).train()
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.eval()
    x = torch.randn(2, cin, 12, 20, device=dev)
    ref_blk = copy.deepcopy(blk).double()
    blk.fuse_bn_train, ref_blk.fuse_bn_train = True, False
    assert blk.route(x.requires_grad_()) == 'train'
    y = blk(x)
    gy = torch.randn_like(y)
    new = _block_run(blk, x, gy)
    blk.fuse_bn_train = False
    assert blk.route(x) == 'stock'
    stock = _block_run(blk, x, gy)
    ref = _block_run(ref_blk, x.double(), gy.double())
    assert sorted(new) == sorted(ref) and len(ref) == 2 + (12 if downsample else 9)
    _held_to_double(new, stock, ref, "Bottleneck%s" % (" + downsample" if downsample else ""))


@pytest.fixture(scope="module")
def r50(dev):
    from orientedreppoints_amd.mmdet_models.resnet import ResNet
    torch.manual_seed(5)
    net = ResNet(50, frozen_stages=1, norm_eval=True)
    _randomise_norms(net, 6)
    net = net.to(dev)
    net.train()
    g = torch.Generator().manual_seed(8)
    return net, torch.randn(2, 3, 64, 64, generator=g).to(dev)


def _net_run(net, img):
    """(stage outputs, layer1's output as the hook saw it, gradient by parameter name) of sum(outs).backward()"""
    seen = []
    h = net.layer1.register_forward_hook(lambda m, i, o: seen.append(o))
    for p in net.parameters():
        p.grad = None
    outs = net(img)
    h.remove()
    sum(o.sum() for o in outs).backward()
    return outs, seen[0], {n: p.grad for n, p in net.named_parameters()}


def test_resnet_frozen_and_trained_stages(dev, r50):
    net, img = r50
    _set_switches(net, True, True)
    assert net.stem_route(img) == 'frozen' and net.layer1[0].route(img) == 'frozen' and net.layer2[0].route(img) == 'train'
    outs, l1, grads = _net_run(net, img)
    net.eval()
    with torch.no_grad():
        want_l1 = net(img)[0]
    net.train()
    assert torch.equal(l1, want_l1) and not l1.requires_grad and outs[1].requires_grad
    trained = [n for n, p in net.named_parameters() if p.requires_grad]
    assert trained and all(n.startswith(('layer2', 'layer3', 'layer4')) for n in trained)
    assert all(grads[n] is not None for n in trained)
    assert all(grads[n] is None for n, p in net.named_parameters() if not p.requires_grad)
    # the stock route and its float64 copy
    _set_switches(net, False, False)
    assert net.stem_route(img) == 'stock' and net.layer1[0].route(img) == 'stock' and net.layer2[0].route(img) == 'stock'
    _o, _l, stock = _net_run(net, img)
    ref_net = copy.deepcopy(net).double()
    ref_net.train()
    _o, _l, ref = _net_run(ref_net, img.double())
    _set_switches(net, True, True)
    _held_to_double({n: grads[n] for n in trained}, {n: stock[n] for n in trained}, {n: ref[n] for n in trained},
                    "ResNet-50 frozen_stages=1, gradients of stages 2-4")


def _stock_forward(net, x):
    """the modules as written: what a training step ran before the routes existed"""
    x = net.maxpool(net.relu(net.bn1(net.conv1(x))))
    outs = []
    for i, name in enumerate(net.res_layers):
        for blk in getattr(net, name):
            identity = x
            out = blk.relu(blk.bn1(blk.conv1(x)))
            out = blk.relu(blk.bn2(blk.conv2(out)))
            out = blk.bn3(blk.conv3(out))
            if blk.downsample is not None:
                identity = blk.downsample(x)
            out += identity
            x = blk.relu(out)
        if i in net.out_indices:
            outs.append(x)
    return tuple(outs)


def test_resnet_switches_off_is_the_stock_route(dev, r50):
    """both switches off: the outputs and every gradient are the bits of the stock modules run by hand"""
    net, img = r50
    _set_switches(net, False, False)
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True        # (the library's convolution backward, the same algorithm on both sides)
    try:
        outs, _l1, grads = _net_run(net, img)
        for p in net.parameters():
            p.grad = None
        want = _stock_forward(net, img)
        sum(o.sum() for o in want).backward()
        assert len(outs) == len(want) and all(torch.equal(a, b) for a, b in zip(outs, want))
        for n, p in net.named_parameters():
            assert (p.grad is None) == (grads[n] is None) and (p.grad is None or torch.equal(p.grad, grads[n])), n
    finally:
        torch.backends.cudnn.deterministic = was
        _set_switches(net, True, True)


def test_resnet_graphed_training_steps_match_eager(dev, r50):
    """three SGD steps with the backbone's forward and backward replayed as graphs (dist_utils.graph_backbone) leave the weights of
    three eager steps on the new route, as tests/test_gpu_train_graph.py holds the stock route"""
    from orientedreppoints_amd import dist_utils as D
    net0, img = r50
    _set_switches(net0, True, True)

    def run(graph):
        net = copy.deepcopy(net0)
        net.train()
        holder = types.SimpleNamespace(backbone=net)
        opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=1e-3, momentum=0.9)
        if graph:
            assert D.graph_backbone(holder, img)
        for _ in range(3):
            opt.zero_grad(set_to_none=True)
            outs = holder.backbone(img)
            sum((o * o).mean() for o in outs).backward()
            opt.step()
        return {n: p.detach().clone() for n, p in net.named_parameters()}
    eager, graphed = run(False), run(True)
    moved = 0
    for n, p in net0.named_parameters():
        if p.requires_grad:
            moved += int(not torch.equal(eager[n], p))
            assert float((eager[n] - graphed[n]).abs().max()) <= 1e-5 * max(float(eager[n].abs().max()), 1e-3), n
        else:
            assert torch.equal(eager[n], p) and torch.equal(graphed[n], p)
    assert moved > 100, "the optimiser must move the trained stages' weights (BatchNorm weight / bias among them)"
