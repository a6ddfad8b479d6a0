"""The training image half on the MI355X: `orp_train_images` against the numpy oracle of tests/train_pipeline_oracle.py bit for
bit (resize, flips, rotation, both orders of Pad and Normalize, the collate's zeros, per-sample geometry inside one launch),
the behaviour of the launch (every element written, twice the same, under graph capture, refused arguments), and
`DeviceTrainPipeline` end to end for the R-50 and the Swin-T train pipelines."""
import ctypes

import numpy as np
import pytest

from train_pipeline_oracle import R50, SWIN, batch_oracle, rotation_inverse, same_value, seeded, small_train_pipeline, write_dataset

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
SALT_MEAN, SALT_STD = (0.1, 300.7, 127.5), (0.3, 255.0, 1.7)                # no round numbers, a mean above 255


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from orientedreppoints_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def image(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def sample(src, new, flip=None, angle=None, pad=None):
    """A plan entry; src, new and pad are (w, h) as in the issue's tables.  The default pad shape is the resized one rounded
    up to a multiple of 4 plus 4 columns and 3 rows, so that all three padding regions exist inside a batch."""
    (sw, sh), (nw, nh) = src, new
    pw, ph = pad if pad is not None else (-(-nw // 4) * 4 + 4, nh + 3)
    return dict(src=(sh, sw), new=(nh, nw), pad=(ph, pw), flip=flip, inv=None if angle is None else rotation_inverse(nw, nh, angle))


def launch(dev, images, plans, mean=MEAN, std=STD, to_rgb=True, pad_first=False, out_hw=None):
    from orientedreppoints_amd.mmdet_ops.train_image_ops import TrainImagePlan, train_images
    plan = TrainImagePlan(plans, mean, std, to_rgb, pad_first)
    packed = plan.pack_images(images)
    imgs, table = torch.from_numpy(packed).to(dev), torch.from_numpy(plan.table).to(dev)
    H, W = out_hw if out_hw is not None else plan.out_shape[2:]
    out = torch.full((len(images), 3, H, W), float('nan'), dtype=torch.float32, device=dev)
    assert train_images(imgs, table, plan, out) is out
    assert np.array_equal(imgs.cpu().numpy(), packed), "the source buffer must be unchanged"
    return out.cpu().numpy()


def check(dev, images, plans, mean=MEAN, std=STD, to_rgb=True, pad_first=False, out_hw=None):
    got = launch(dev, images, plans, mean, std, to_rgb, pad_first, out_hw)
    want = batch_oracle(images, plans, mean, std, to_rgb, pad_first, out_hw)
    assert got.shape == want.shape and not np.isnan(got).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), [(p['src'], p['new'], p['flip'], p['inv'] is not None) for p in plans]
    return got


# ---- bit for bit against the oracle -------------------------------------------------------------------------------------------
SIZES = [((1, 1), (1, 1)), ((3, 5), (4, 7)), ((40, 24), (33, 17)), ((24, 40), (61, 97)), ((97, 61), (24, 40)),
         ((300, 10), (257, 9)), ((10, 300), (9, 257))]          # 257 columns / 9 rows: one past a block's 256 x 8


@pytest.mark.parametrize("src,new", SIZES)
def test_resize_and_rotation_sizes(dev, src, new):
    """Each pair of sizes alone, without and with the rotation (stage B), to_rgb on and off."""
    img = image(src[0], src[1], 11 * src[0] + new[0])
    for to_rgb in (True, False):
        check(dev, [img], [sample(src, new)], to_rgb=to_rgb)
        check(dev, [img], [sample(src, new, angle=37.3)], to_rgb=to_rgb)


@pytest.mark.parametrize("pad_first", [False, True])
def test_three_samples_in_one_launch_and_alone(dev, pad_first):
    """Three samples of three source, resized and pad sizes (one flips, one rotates) in one launch, and each alone in a batch
    of the same shape: a sample's values do not depend on its neighbours.  The three padding regions, checked one by one."""
    from orientedreppoints_amd.mmdet_datasets.imops import imnormalize
    images = [image(90, 70, 1), image(64, 96, 2), image(77, 83, 3)]
    plans = [sample((90, 70), (123, 96), flip='horizontal', pad=(128, 96)), sample((64, 96), (80, 120), angle=-151.9, pad=(96, 128)),
             sample((77, 83), (59, 64), flip='vertical', angle=37.3, pad=(64, 64))]
    together = check(dev, images, plans, SALT_MEAN, SALT_STD, pad_first=pad_first)
    assert together.shape == (3, 3, 128, 128)
    for b in range(3):
        alone = check(dev, images[b:b + 1], plans[b:b + 1], SALT_MEAN, SALT_STD, pad_first=pad_first, out_hw=(128, 128))
        assert np.array_equal(alone[0].view(np.uint32), together[b].view(np.uint32))
    fill = imnormalize(np.zeros((1, 1, 3), np.uint8), SALT_MEAN, SALT_STD, True).reshape(3) if pad_first else np.zeros(3, np.float32)
    assert fill.all() == pad_first
    for b, p in enumerate(plans):
        (nh, nw), (ph, pw) = p['new'], p['pad']
        got = together[b]
        assert np.isfinite(got).all()
        for c in range(3):
            assert np.all(got[c, nh:ph, :pw] == fill[c]) and np.all(got[c, :ph, nw:pw] == fill[c])       # Pad's region
        assert not got[:, ph:, :].any() and not got[:, :, pw:].any()                                     # the collate's region
        if p['inv'] is not None:                    # the rotation's border: source zeros, always normalised, never the pad fill
            want = imnormalize(np.zeros((1, 1, 3), np.uint8), SALT_MEAN, SALT_STD, True).reshape(3)
            assert np.array_equal(got[:, 0, 0], want) and want.all()


@pytest.mark.parametrize("flip", [None, 'horizontal', 'vertical'])
def test_flips_with_and_without_rotation(dev, flip):
    img = image(41, 35, 4)
    plain = check(dev, [img], [sample((41, 35), (66, 57), flip=None, pad=(68, 57))])[0]
    got = check(dev, [img], [sample((41, 35), (66, 57), flip=flip, pad=(68, 57))])[0]
    inside = plain[:, :57, :66]                      # mirrored inside the resized size: every value is the unflipped kernel's
    mirror = {None: inside, 'horizontal': inside[:, :, ::-1], 'vertical': inside[:, ::-1]}[flip]
    assert np.array_equal(got[:, :57, :66], mirror) and np.array_equal(got[:, :, 66:], plain[:, :, 66:])
    check(dev, [img], [sample((41, 35), (66, 57), flip=flip, angle=37.3, pad=(68, 57))])


@pytest.mark.parametrize("angle", [0, 90, 180, 37.3, -151.9])
def test_rotation_angles(dev, angle):
    """Rotation by 0 goes through stage B and equals the unrotated sample (the identity the pipeline relies on when it skips
    stage B for a sample that drew no rotation)."""
    for (w, h) in ((64, 64), (131, 97)):
        img = image(w, h, 5)
        got = check(dev, [img], [sample((w, h), (w, h), angle=angle)])
        if angle == 0:
            assert np.array_equal(got, check(dev, [img], [sample((w, h), (w, h))]))


def test_ties_and_constant_images(dev):
    """The 2x up-sampling of columns 0, 2, 1, 3 (blends on exact halves: rint's ties to even), an all-255 and an all-0 image,
    through both stages."""
    row = np.array([0, 2, 1, 3], np.uint8)
    ties = np.repeat(np.tile(row[None, :, None], (3, 1, 3)), 1, 0)
    ties[1] += 1
    for img in (ties, np.full((3, 4, 3), 255, np.uint8), np.zeros((3, 4, 3), np.uint8)):
        for angle in (None, 37.3):
            check(dev, [img], [sample((4, 3), (8, 6), angle=angle)])
            check(dev, [img], [sample((4, 3), (8, 6), angle=angle)], SALT_MEAN, SALT_STD, to_rgb=False, pad_first=True)
    from test_scene_resize import resize_oracle
    up = resize_oracle(ties, 8, 6)
    assert set(np.unique(up[0, :, 0])) >= {0, 1, 2}                      # (0.5 -> 0, 1.5 -> 2: the ties do occur and go to even)


# ---- behaviour of the launch ----------------------------------------------------------------------------------------------------
def _staged(dev, images, plans, pad_first=True):
    from orientedreppoints_amd.mmdet_ops.train_image_ops import TrainImagePlan
    plan = TrainImagePlan(plans, MEAN, STD, True, pad_first)
    imgs, table = torch.from_numpy(plan.pack_images(images)).to(dev), torch.from_numpy(plan.table).to(dev)
    return plan, imgs, table


def test_same_launch_twice_and_captured_graph(dev):
    from orientedreppoints_amd.mmdet_ops.train_image_ops import train_images
    plans = [sample((90, 70), (123, 96), flip='vertical', pad=(128, 96)), sample((64, 96), (80, 120), angle=37.3, pad=(96, 128))]
    first, second = [image(90, 70, 1), image(64, 96, 2)], [image(90, 70, 8), image(64, 96, 9)]
    plan, imgs, table = _staged(dev, first, plans)
    a = train_images(imgs, table, plan, torch.full(plan.out_shape, float('nan'), device=dev))
    b = train_images(imgs, table, plan, torch.full(plan.out_shape, 7.0, device=dev))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    static_out = torch.full(plan.out_shape, float('nan'), device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        train_images(imgs, table, plan, static_out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        train_images(imgs, table, plan, static_out)
    imgs.copy_(torch.from_numpy(plan.pack_images(second)).to(dev))
    static_out.fill_(float('nan'))
    graph.replay()
    eager = train_images(imgs, table, plan, torch.full(plan.out_shape, float('nan'), device=dev))
    assert torch.equal(static_out.view(torch.int32), eager.view(torch.int32))
    want = batch_oracle(second, plans, MEAN, STD, True, True)
    assert np.array_equal(static_out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert not torch.equal(eager, a)


def test_refused_arguments(dev):
    from orientedreppoints_amd import _lib
    from orientedreppoints_amd.mmdet_ops.train_image_ops import TrainImagePlan, train_images
    images = [image(40, 24, 1), image(24, 40, 2)]
    plans = [sample((40, 24), (33, 17), pad=(36, 20)), sample((24, 40), (30, 50), angle=90, pad=(32, 52))]
    plan, imgs, table = _staged(dev, images, plans)
    out = torch.zeros(plan.out_shape, device=dev)
    scratch = torch.zeros(plan.scratch_bytes, dtype=torch.uint8, device=dev)
    train_images(imgs, table, plan, out, scratch=scratch)
    # the wrapper
    with pytest.raises(TypeError):
        train_images(imgs.cpu(), table, plan, out)
    with pytest.raises(ValueError, match="images"):
        train_images(imgs[:-16], table, plan, out)
    with pytest.raises(ValueError, match="table"):
        train_images(imgs, table[:-16], plan, out)
    with pytest.raises(ValueError, match="out must be"):
        train_images(imgs, table, plan, out.double())
    with pytest.raises(ValueError, match="multiple of 4"):
        train_images(imgs, table, plan, torch.zeros((2, 3, 52, 38), device=dev))
    with pytest.raises(ValueError, match="smaller than a sample's pad shape"):
        train_images(imgs, table, plan, torch.zeros((2, 3, 48, 36), device=dev))
    with pytest.raises(ValueError, match="scratch"):
        train_images(imgs, table, plan, out, scratch=scratch[:-4])
    with pytest.raises(ValueError, match="smaller than the resized"):
        TrainImagePlan([sample((40, 24), (33, 17), pad=(32, 20))], MEAN, STD)
    with pytest.raises(ValueError, match="flip"):
        TrainImagePlan([sample((40, 24), (33, 17), flip='diagonal')], MEAN, STD)

    # the entry point itself: every refusal comes before any launch
    L = _lib.lib()
    m, s = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
    at = lambda name: table.data_ptr() + plan.sections[name][0]                                      # noqa: E731

    def call(**kw):
        a = dict(images=imgs.data_ptr(), images_bytes=imgs.numel(), desc_host=plan.desc.ctypes.data, desc=at('desc'), n=2,
                 inv=at('inv'), i0=at('axis_i0'), w1=at('axis_w1'), axis_len=plan.axis_len, mean=m, std=s, to_rgb=1, pad_first=0,
                 out=out.data_ptr(), out_h=out.size(2), out_w=out.size(3), scratch=scratch.data_ptr(), scratch_bytes=scratch.numel())
        a.update(kw)
        p = lambda v: ctypes.c_void_p(v) if isinstance(v, int) else v                               # noqa: E731
        return L.orp_train_images(p(a['images']), a['images_bytes'], p(a['desc_host']), p(a['desc']), a['n'], p(a['inv']), p(a['i0']),
                                  p(a['w1']), a['axis_len'], a['mean'], a['std'], a['to_rgb'], a['pad_first'], p(a['out']), a['out_h'],
                                  a['out_w'], p(a['scratch']), a['scratch_bytes'], _lib.stream_of(out))
    assert call() == _lib.ORP_OK
    for name in ('images', 'desc_host', 'desc', 'inv', 'i0', 'w1', 'mean', 'std', 'out', 'scratch'):
        assert call(**{name: None}) == _lib.ORP_EINVAL, name
    assert call(out_w=out.size(3) - 2) == _lib.ORP_EINVAL                       # out_w % 4 != 0
    assert call(out_w=out.size(3) - 4) == _lib.ORP_EINVAL                       # a pad shape wider than the batch
    assert call(out_h=out.size(2) - 1) == _lib.ORP_EINVAL                       # ... and higher
    assert call(scratch_bytes=scratch.numel() - 256) == _lib.ORP_EINVAL         # scratch too small
    assert call(images_bytes=imgs.numel() - 64) == _lib.ORP_EINVAL              # an image outside the buffer
    assert call(axis_len=plan.axis_len - 1) == _lib.ORP_EINVAL                  # a table outside the buffer
    assert call(n=65536) == _lib.ORP_EINVAL and call(n=-1) == _lib.ORP_EINVAL
    small = plan.desc.copy()
    small['pad_w'][0] = small['new_w'][0] - 1                                   # a pad shape smaller than the resized shape
    assert call(desc_host=small.ctypes.data) == _lib.ORP_EINVAL
    bad_flip = plan.desc.copy()
    bad_flip['flip'][1] = 3
    assert call(desc_host=bad_flip.ctypes.data) == _lib.ORP_EINVAL
    torch.cuda.synchronize()
    assert L.orp_train_images_scratch_bytes(30, 50) == ((3 * 30 + 3) // 4 * 4 * 50 + 255) // 256 * 256 == plan.scratch_bytes
    assert L.orp_train_images_scratch_bytes(0, 5) == 0


# ---- DeviceTrainPipeline end to end ---------------------------------------------------------------------------------------------
def _pipelines(tmp_path, cfg, dev):
    from orientedreppoints_amd.mmdet_datasets import DeviceTrainPipeline, DotaDataset
    ann_file, arrays = write_dataset(str(tmp_path))
    steps = small_train_pipeline(cfg)
    host = DotaDataset(ann_file=ann_file, img_prefix=str(tmp_path), pipeline=steps)
    dp = DeviceTrainPipeline.from_config(steps, device=dev)
    return host, DotaDataset(ann_file=ann_file, img_prefix=str(tmp_path), pipeline=[dp.host]), dp


# (config, [(image index, seed)]): the Swin-T pair holds a vertical flip without and one with a rotation
BATCHES = [(R50, [(2, 2), (0, 0)]), (SWIN, [(1, 16), (2, 17)])]


@pytest.mark.parametrize("name,picks", BATCHES)
def test_device_train_pipeline_end_to_end(dev, tmp_path, reference_configs, name, picks):
    """A seeded batch of two: the collated image bit for bit the oracle's, boxes, labels and metas the host pipeline's; the
    device half of `collate` (after the uploads) does not synchronise; for R-50 one training step on the batch has a finite loss."""
    host, dev_ds, dp = _pipelines(tmp_path, reference_configs[name], dev)
    want = [seeded(host, i, s) for i, s in picks]
    samples = [seeded(dev_ds, i, s) for i, s in picks]
    assert all(w is not None for w in want) and all(s is not None for s in samples)
    if name == SWIN:
        assert [s['plan']['inv'] is not None for s in samples] == [False, True] and samples[0]['plan']['flip'] == 'vertical'
    staged = dp.upload(samples)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        batch = dp.run(staged)
        with pytest.raises(RuntimeError):                        # (the mode is live: a D2H copy of a device tensor raises)
            batch['img'][0, 0, 0, 0].item()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    img = batch['img']
    H, W = max(s['plan']['pad'][0] for s in samples), max(s['plan']['pad'][1] for s in samples)
    assert img.is_cuda and img.dtype == torch.float32 and tuple(img.shape) == (2, 3, H, W)
    oracle = batch_oracle([s['img'] for s in samples], [s['plan'] for s in samples], dp.mean, dp.std, dp.to_rgb, dp.pad_before_normalize)
    assert np.array_equal(img.cpu().numpy().view(np.uint32), oracle.view(np.uint32))
    for k in range(2):
        assert same_value(batch['img_metas'][k], want[k]['img_meta'])
        assert batch['gt_bboxes'][k].is_cuda and batch['gt_bboxes'][k].dtype == torch.float32
        assert batch['gt_labels'][k].is_cuda and batch['gt_labels'][k].dtype == torch.int64
        assert torch.equal(batch['gt_bboxes'][k].cpu(), want[k]['gt_bboxes']) and torch.equal(batch['gt_labels'][k].cpu(), want[k]['gt_labels'])
        ph, pw = samples[k]['plan']['pad']
        close = (img[k, :, :ph, :pw].cpu() - want[k]['img']).abs().max()
        assert float(close) <= 2 / min(STD) + 1e-6                # (the host image: the CPU test holds the oracle to it)
    again = dp.collate(samples)
    assert torch.equal(again['img'].view(torch.int32), img.view(torch.int32))
    if name != R50:
        return
    from orientedreppoints_amd import dist_utils as D
    from orientedreppoints_amd.dota_configs import r50_model, test_cfg, train_cfg
    from orientedreppoints_amd.mmdet_models import ConfigDict, build_detector
    torch.manual_seed(0)
    model = build_detector(ConfigDict(r50_model), train_cfg=ConfigDict(train_cfg), test_cfg=ConfigDict(test_cfg)).to(dev).train()
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=1e-3, momentum=0.9)
    hook = D.DistOptimizerHook(grad_clip=dict(max_norm=35, norm_type=2), overlap=True, scaler=None)
    data = dict(img=batch['img'], img_meta=batch['img_metas'], gt_bboxes=batch['gt_bboxes'], gt_labels=batch['gt_labels'])
    loss = float(D.train_step(model, opt, data, hook)['loss'])
    assert np.isfinite(loss)
