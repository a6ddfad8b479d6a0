"""CPU: the float64 statement of the fused BatchNorm backward (tests/bn_train_cases.py) is torch's own autograd of the stock modules,
its exact cases are exact, and the backbone's routing predicates send every combination of gradient mode, frozen parameters,
BatchNorm mode, dtype, checkpointing and switches where the README says they go."""
import contextlib

import numpy as np
import pytest

import bn_train_cases as K

torch = pytest.importorskip("torch")
F = torch.nn.functional


@pytest.mark.parametrize("shape", [s for s in K.SHAPES if s[2] * s[3] <= 5000])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("res", K.RESIDUALS)
def test_float64_statement_is_torch_autograd(shape, relu, res):
    """relu?(F.batch_norm(x, mean, var, w, b, False, 0., eps) (+ r | + F.batch_norm(x2, ...))) in float64 on the CPU: its gradients are
    the statement's, to float64 rounding"""
    d = K.random_case(shape, 5)
    eps = 1e-5
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=k in ('x', 'x2', 'residual', 'weight', 'bias', 'weight2', 'bias2'))
         for k, v in d.items()}
    y = F.batch_norm(t['x'], t['running_mean'], t['running_var'], t['weight'], t['bias'], False, 0., eps)
    if res == 'plain':
        y = y + t['residual']
    elif res == 'affine2':
        y = y + F.batch_norm(t['x2'], t['running_mean2'], t['running_var2'], t['weight2'], t['bias2'], False, 0., eps)
    if relu:
        y = torch.relu(y)
    y.backward(t['grad_y'])

    rstd = 1. / np.sqrt(d['running_var'].astype(np.float64) + eps)
    rstd2 = 1. / np.sqrt(d['running_var2'].astype(np.float64) + eps)
    a, a2 = d['weight'].astype(np.float64) * rstd, d['weight2'].astype(np.float64) * rstd2
    two = res == 'affine2'
    want = K.backward_f64(d['grad_y'], a, y=y.detach().numpy() if relu else None, x=d['x'], mean=d['running_mean'], rstd=rstd,
                          scale2=a2 if two else None, x2=d['x2'] if two else None, mean2=d['running_mean2'], rstd2=rstd2)
    # the statement's own forward gives the mask torch's forward gave
    b = d['bias'].astype(np.float64) - d['running_mean'].astype(np.float64) * a
    b2 = d['bias2'].astype(np.float64) - d['running_mean2'].astype(np.float64) * a2
    yf = K.forward_f64(d['x'], a, b, relu, residual=None if res == 'none' else (d['x2'] if two else d['residual']),
                       scale2=a2 if two else None, shift2=b2 if two else None)
    np.testing.assert_allclose(yf, y.detach().numpy(), rtol=1e-12, atol=1e-12)

    def close(got, exp, scale):
        assert np.max(np.abs(got.numpy() - exp)) <= 1e-12 * max(1., float(np.max(scale)))
    close(t['x'].grad, want['grad_x'], np.abs(want['grad_x']))
    close(t['weight'].grad, want['dweight'], want['dweight_abs'])
    close(t['bias'].grad, want['dbias'], want['dbias_abs'])
    if res == 'plain':
        close(t['residual'].grad, want['grad_res'], np.abs(want['g']))
    if two:
        close(t['x2'].grad, want['grad_x2'], np.abs(want['grad_x2']))
        close(t['weight2'].grad, want['dweight2'], want['dweight2_abs'])
        close(t['bias2'].grad, want['dbias'], want['dbias_abs'])


@pytest.mark.parametrize("shape", K.SHAPES)
def test_exact_cases_are_exact(shape):
    """the exact cases' terms are integers and sum |terms| stays below 2^24 per channel, so every partial sum of an fp32 reduction
    is exact in any order -- and the mask has zeros of both signs, the weights a negative and a zero"""
    d = K.exact_case(shape, 3)
    for relu in (True, False):
        w = K.backward_f64(d['grad_y'], d['scale'], y=d['y'] if relu else None, x=d['x'], mean=d['mean'], rstd=d['rstd'],
                           scale2=d['scale2'], x2=d['x2'], mean2=d['mean2'], rstd2=d['rstd2'])
        for s in ('', '2'):
            xhat = (d['x' + s].astype(np.float64) - K._bc(d['mean' + s])) * K._bc(d['rstd' + s])
            assert np.array_equal(xhat, np.round(xhat)) and np.max(np.abs(xhat)) <= 8
            assert np.max(w['dweight' + s + '_abs']) < 2 ** 24
            assert np.array_equal(w['dweight' + s], np.round(w['dweight' + s]))
        assert np.array_equal(w['g'], np.round(w['g'])) and np.max(w['dbias_abs']) < 2 ** 24
        # one rounding to fp32 changes nothing: the products g a are exact too
        assert np.array_equal(w['grad_x'].astype(np.float32).astype(np.float64), w['grad_x'])
    assert d['scale'][0] < 0 and (shape[1] < 2 or d['scale'][1] == 0)
    if d['y'].size >= 64:
        assert np.any((d['y'] == 0) & np.signbit(d['y'])) and np.any((d['y'] == 0) & ~np.signbit(d['y'])) and np.any(d['y'] < 0)


class _Described(object):
    """what the routing predicates ask of a tensor, for devices this machine does not have"""

    def __init__(self, is_cuda, dtype, requires_grad=False, contiguous=True):
        self.is_cuda, self.dtype, self.requires_grad, self._contiguous = is_cuda, dtype, requires_grad, contiguous

    def dim(self):
        return 4

    def is_contiguous(self):
        return self._contiguous


@contextlib.contextmanager
def _cuda_autocast():
    """the CUDA autocast flag as the predicates read it, set without a device (torch.autocast('cuda') disables itself without one)"""
    was = torch.is_autocast_enabled()
    torch.set_autocast_enabled(True)
    try:
        yield
    finally:
        torch.set_autocast_enabled(was)


def _block(frozen, bn_training, with_cp, train_fuse, frozen_fuse, downsample=False):
    from orientedreppoints_amd.mmdet_models.resnet import Bottleneck
    ds = None
    if downsample:
        ds = torch.nn.Sequential(torch.nn.Conv2d(16, 32, 1, stride=2, bias=False), torch.nn.BatchNorm2d(32))
    # (without a downsample branch the identity has the block's 4 * planes output channels)
    blk = Bottleneck(16 if downsample else 32, 8, stride=2 if downsample else 1, downsample=ds).train()
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.train(bn_training)
    for p in blk.parameters():
        p.requires_grad = not frozen
    blk.with_cp, blk.fuse_bn_train, blk.fuse_bn_frozen = with_cp, train_fuse, frozen_fuse
    return blk


@pytest.mark.parametrize("downsample", [False, True])
def test_bottleneck_routes(downsample):
    for case in K.routing_cases():
        grad, frozen, bn_training, dtype, with_cp, train_fuse, frozen_fuse = case
        blk = _block(frozen, bn_training, with_cp, train_fuse, frozen_fuse, downsample)
        with torch.set_grad_enabled(grad):
            got = blk.route(_Described(True, getattr(torch, dtype)))
            assert got == K.expected_route(*case), (case, got)
            # a CPU tensor: always the stock modules
            assert blk.route(_Described(False, getattr(torch, dtype))) == 'stock'
            assert blk.route(torch.zeros(1, 32, 4, 4, dtype=getattr(torch, dtype))) == 'stock'


def test_bottleneck_route_edges():
    """what the table does not enumerate: an input that requires a gradient is never 'frozen'; a non-contiguous input and autocast
    keep the stock modules in training; the environment switches are what an unset attribute falls back to"""
    from orientedreppoints_amd import switches
    x32 = dict(is_cuda=True, dtype=torch.float32)
    blk = _block(True, False, False, True, True)
    assert blk.route(_Described(requires_grad=True, **x32)) == 'train'
    assert blk.route(_Described(requires_grad=False, **x32)) == 'frozen'
    blk = _block(False, False, False, True, True)
    assert blk.route(_Described(contiguous=False, **x32)) == 'stock'
    with _cuda_autocast():
        assert blk.route(_Described(**x32)) == 'stock'
        assert _block(True, False, False, True, True).route(_Described(**x32)) == 'stock'
    blk.fuse_bn_train = blk.fuse_bn_frozen = None
    assert blk.route(_Described(**x32)) == ('train' if switches.BN_TRAIN_FUSE else 'stock')
    # one norm that is not a BatchNorm2d in eval mode keeps the whole block stock
    blk = _block(False, False, False, True, True)
    blk.bn2.train()
    assert blk.route(_Described(**x32)) == 'stock'
    blk = _block(False, False, False, True, True, downsample=True)
    blk.downsample[1].train()
    assert blk.route(_Described(**x32)) == 'stock'


def test_stem_routes():
    from orientedreppoints_amd.mmdet_models.resnet import ResNet
    x32 = dict(is_cuda=True, dtype=torch.float32)
    for frozen_stages, fuse, want in ((1, True, 'frozen'), (1, False, 'stock'), (0, True, 'frozen'), (-1, True, 'stock')):
        net = ResNet(50, frozen_stages=frozen_stages, norm_eval=True)
        net.train()
        net.fuse_bn_frozen = fuse
        for b in net.layer1:
            b.fuse_bn_frozen = fuse
        assert net.stem_route(_Described(**x32)) == want
        assert net.stem_route(_Described(requires_grad=True, **x32)) == 'stock'
        assert net.stem_route(_Described(is_cuda=True, dtype=torch.float16)) == 'stock'
        assert net.stem_route(_Described(is_cuda=False, dtype=torch.float32)) == 'stock'
        with _cuda_autocast():
            assert net.stem_route(_Described(**x32)) == 'stock'
        with torch.no_grad():
            assert net.stem_route(_Described(**x32)) == 'fused'
        # which blocks of a training step take which route
        routes = [b.route(_Described(**x32)) for b in net.layer1] + [net.layer2[1].route(_Described(requires_grad=True, **x32))]
        assert routes == ['frozen' if (frozen_stages >= 1 and fuse) else 'train'] * 3 + ['train']


def test_cpu_tensors_take_the_stock_route_with_unchanged_results():
    """a CPU block computes what the modules as written compute, bit for bit, in training and under no_grad, whatever the switches"""
    torch.manual_seed(0)
    for downsample in (False, True):
        blk = _block(False, False, False, True, True, downsample)
        with torch.no_grad():
            for bn in [m for m in blk.modules() if isinstance(m, torch.nn.BatchNorm2d)]:
                bn.running_mean.normal_(); bn.running_var.uniform_(0.5, 2.); bn.weight.normal_(); bn.bias.normal_()
        x = torch.randn(2, 16 if downsample else 32, 6, 10)
        for grad in (True, False):
            with torch.set_grad_enabled(grad):
                got = blk(x)
                out = torch.relu(blk.bn1(blk.conv1(x)))
                out = torch.relu(blk.bn2(blk.conv2(out)))
                out = blk.bn3(blk.conv3(out)) + (blk.downsample(x) if downsample else x)
                want = torch.relu(out)
            assert torch.equal(got, want) and got.requires_grad == grad


def test_bn_act_train_refuses_what_it_does_not_take():
    """CPU tensors, and with them every dtype / layout / BatchNorm mode it was not written for, are a ValueError, never a fall-back"""
    from orientedreppoints_amd.mmdet_ops.fused_norm import bn_act_train, bn_act_train_ok
    bn = torch.nn.BatchNorm2d(4).eval()
    x = torch.randn(2, 4, 3, 3)
    assert not bn_act_train_ok(x, bn)
    with pytest.raises(ValueError):
        bn_act_train(x, bn)
    with pytest.raises(ValueError):
        bn_act_train(x, torch.nn.GroupNorm(2, 4))
