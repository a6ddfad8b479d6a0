"""The backward of the backbone's fused eval-mode BatchNorm passes, stated in float64 numpy, and the cases the tests hold the
kernels to (tests/test_bn_train_cases.py on the CPU, tests/test_gpu_bn_train.py on the GPU).

Forward (include/orp_hip.h, orp_affine_act / orp_affine2_act):  y = relu?(x a[c] + b[c] (+ r | + x2 a2[c] + b2[c])),
a = weight rstd, b = bias - mean a, rstd = rsqrt(running_var + eps).  Backward (orp_affine_act_backward / orp_affine2_act_backward):
g = grad_y where y > 0 (no ReLU: g = grad_y), grad_x = g a, grad_x2 = g a2, grad_res = g, dbias = sum g,
dweight = sum g (x - mean) rstd, sums over images and positions."""
import numpy as np

# (B, C, H, W): the smallest shapes at which the pass can go wrong.  The backward launches the forward's grid (256 threads, about four
# float4s or scalars per thread, at most 64 workgroups per plane), so it has the forward's edges and no others.
SHAPES = [
    (1, 1, 1, 1),        # a single element
    (2, 3, 5, 7),        # odd hw: the scalar path
    (1, 2, 1, 4),        # one float4
    (3, 5, 16, 20),      # several images and channels, less than one workgroup per plane
    (1, 2, 4, 1025),     # hw % 4 == 0, one float4 past a workgroup's 1 024
    (1, 1, 513, 512),    # past the cap of 64 workgroups per plane: the stride loop strides
]
RESIDUALS = ('none', 'plain', 'affine2')


def _bc(v, ndim=4):
    """a per-channel vector against [B, C, ...]"""
    return np.asarray(v, np.float64).reshape((1, -1) + (1,) * (ndim - 2))


def forward_f64(x, scale, shift, relu, residual=None, scale2=None, shift2=None):
    y = np.asarray(x, np.float64) * _bc(scale) + _bc(shift)
    if residual is not None:
        r = np.asarray(residual, np.float64)
        y = y + (r * _bc(scale2) + _bc(shift2) if scale2 is not None else r)
    return np.maximum(y, 0.) if relu else y


def backward_f64(grad_y, scale, y=None, x=None, mean=None, rstd=None, scale2=None, x2=None, mean2=None, rstd2=None):
    """every output of the backward in float64 from the arrays the kernel reads (y: the forward's output = the ReLU mask, None = no
    ReLU; x / x2 None = that dweight is not formed).  `dweight_abs` / `dbias_abs` are sum |terms|: what a summation error is held
    against."""
    g = np.asarray(grad_y, np.float64)
    if y is not None:
        g = np.where(np.asarray(y) > 0, g, 0.)
    out = dict(g=g, grad_res=g, grad_x=g * _bc(scale), dbias=g.sum(axis=(0, 2, 3)), dbias_abs=np.abs(g).sum(axis=(0, 2, 3)))
    if scale2 is not None:
        out['grad_x2'] = g * _bc(scale2)
    for key, xx, m, r in (('dweight', x, mean, rstd), ('dweight2', x2, mean2, rstd2)):
        if xx is not None:
            t = g * ((np.asarray(xx, np.float64) - _bc(m)) * _bc(r))
            out[key] = t.sum(axis=(0, 2, 3))
            out[key + '_abs'] = np.abs(t).sum(axis=(0, 2, 3))
    return out


def exact_case(shape, seed):
    """fp32 arrays whose every partial sum of g and of g xhat is an integer below 2^24 in any order: grad_y integer in [-3, 3], mean
    integer, x - mean integer in [-2, 2], rstd in {1, 2, 4} (|g xhat| <= 24; 24 * 513 * 512 < 2^24).  y holds the mask: about a
    quarter exactly 0 (of both signs) and a quarter negative.  The weight is negative in one channel and zero in another where there
    are that many (scale = weight rstd: the kernel's `scale`)."""
    B, C, H, W = shape
    rng = np.random.RandomState(seed)
    d = dict(grad_y=rng.randint(-3, 4, size=shape).astype(np.float32))
    for s in ('', '2'):
        mean = rng.randint(-5, 6, size=C).astype(np.float32)
        rstd = np.asarray([1., 2., 4.], np.float32)[rng.randint(0, 3, size=C)]
        weight = rng.randint(1, 4, size=C).astype(np.float32)
        weight[0] = -2.
        if C > 1:
            weight[1] = 0.
        d['x' + s] = (mean.reshape(1, C, 1, 1) + rng.randint(-2, 3, size=shape)).astype(np.float32)
        d['mean' + s], d['rstd' + s], d['scale' + s] = mean, rstd, weight * rstd
    y = rng.normal(size=shape).astype(np.float32)
    u = rng.rand(*shape)
    y[u < 0.25] = 0.
    y[u < 0.08] = -0.
    d['y'] = y
    return d


def random_case(shape, seed):
    """N(0, 1) data around channel means of up to +-50 (x sits far from zero in some channels), BatchNorm parameters with a
    negative and a zero weight: (x, x2, residual, grad_y, and per BatchNorm: weight, bias, running_mean, running_var)"""
    B, C, H, W = shape
    rng = np.random.RandomState(seed)
    d = dict(grad_y=rng.normal(size=shape).astype(np.float32), residual=rng.normal(size=shape).astype(np.float32))
    for s in ('', '2'):
        mean = rng.uniform(-50, 50, size=C).astype(np.float32)
        var = rng.uniform(0.3, 1.5, size=C).astype(np.float32)
        weight = rng.uniform(0.5, 1.5, size=C).astype(np.float32)
        weight[0] = -0.7
        if C > 1:
            weight[1] = 0.
        d['x' + s] = (mean.reshape(1, C, 1, 1) + np.sqrt(var).reshape(1, C, 1, 1) * rng.normal(size=shape)).astype(np.float32)
        d['weight' + s], d['bias' + s] = weight, rng.normal(0, 0.3, size=C).astype(np.float32)
        d['running_mean' + s], d['running_var' + s] = mean, var
    return d


def op_cases():
    """(relu, residual form, dweight wanted, grad_res aliases grad_y) of the operator tests; aliasing only where there is a grad_res"""
    out = []
    for relu in (True, False):
        for res in RESIDUALS:
            for want in (True, False):
                for alias in ((False, True) if res == 'plain' else (False,)):
                    out.append((relu, res, want, alias))
    return out


def routing_cases():
    """every combination the routing predicates decide on: (grad enabled, parameters frozen, bn.training, dtype name, with_cp,
    ORP_BN_TRAIN_FUSE as the block sees it, ORP_BN_FROZEN_FUSE as the block sees it)"""
    import itertools
    return list(itertools.product((True, False), (True, False), (False, True), ('float32', 'float64', 'float16'), (False, True),
                                  (True, False), (True, False)))


def expected_route(grad, frozen, bn_training, dtype, with_cp, train_fuse, frozen_fuse, on_gpu=True):
    """the route `Bottleneck.route` must report for a contiguous tensor that does not itself require a gradient"""
    if not on_gpu or dtype != 'float32' or bn_training:
        return 'stock'
    if not grad:
        return 'fused'
    if with_cp:
        return 'stock'
    if frozen and frozen_fuse:
        return 'frozen'
    return 'train' if train_fuse else 'stock'
