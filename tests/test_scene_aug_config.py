"""`SceneInference(views=...)` without a GPU: `from_config(..., aug=True)` reads the flip flag and the scale list of the test
pipeline into views in `MultiScaleFlipAug`'s own order (for each scale: plain, then flipped); without `aug=True` such a pipeline
is refused as before; malformed views raise; the per-view planning of a scene."""
import copy

import pytest

from test_gpu_scene_inference import stub_model


def edited(reference_configs, **changes):
    from orientedreppoints_amd.mmdet_models import Config
    cfg = copy.deepcopy(dict(reference_configs['orientedrepoints_r101_demo.py']._cfg_dict))
    aug = cfg['data']['test']['pipeline'][1]
    assert aug['type'] == 'MultiScaleFlipAug' and aug['transforms'][0]['type'] == 'RotateResize'
    for k, v in changes.items():
        if k in ('flip', 'img_scale'):
            aug[k] = v
        elif k == 'pad_size':
            [t for t in aug['transforms'] if t['type'] == 'Pad'][0]['size'] = v
        else:
            aug['transforms'][0][k] = v
    return Config(cfg)


def test_from_config_aug_gives_the_views_in_pipeline_order(reference_configs):
    from orientedreppoints_amd.mmdet_models import SceneInference
    two = [(1333, 960), (1333, 1024)]
    cases = [(dict(), [((1333, 960), False)]),
             (dict(flip=True), [((1333, 960), False), ((1333, 960), True)]),
             (dict(img_scale=two), [((1333, 960), False), ((1333, 1024), False)]),
             (dict(img_scale=two, flip=True), [((1333, 960), False), ((1333, 960), True), ((1333, 1024), False), ((1333, 1024), True)])]
    for changes, views in cases:
        si = SceneInference.from_config(stub_model(), edited(reference_configs, **changes), aug=True, batch=2)
        assert si.views == views and si.img_scale is None and si.size_divisor == 32 and si.to_rgb is True and si.batch == 2


def test_without_aug_the_pipeline_is_refused_as_before(reference_configs):
    from orientedreppoints_amd.mmdet_models import SceneInference
    with pytest.raises(ValueError, match="flip"):
        SceneInference.from_config(stub_model(), edited(reference_configs, flip=True))
    with pytest.raises(ValueError, match="scales"):
        SceneInference.from_config(stub_model(), edited(reference_configs, img_scale=[(1333, 960), (1333, 1024)]))
    for aug in (False, True):                          # what stays refused with aug=True too
        with pytest.raises(ValueError, match="keep_ratio"):
            SceneInference.from_config(stub_model(), edited(reference_configs, flip=aug, keep_ratio=False), aug=aug)
        with pytest.raises(ValueError, match="interpolation"):
            SceneInference.from_config(stub_model(), edited(reference_configs, flip=aug, interpolation='bicubic'), aug=aug)
        with pytest.raises(ValueError, match="Pad"):
            SceneInference.from_config(stub_model(), edited(reference_configs, flip=aug, pad_size=(1024, 1024)), aug=aug)


@pytest.mark.parametrize("views", [[], "flip", [((1333, 960), False)] * 9, [(1333, 960)], [((1333, 960), 1)], [((1333, 960), None)],
                                   [((1333,), False)], [((1333, 0), True)], [((1333.5, 960), True)], [(960, False)],
                                   [((1333, 960), False, True)]])
def test_malformed_views_raise(views):
    from orientedreppoints_amd.mmdet_models import SceneInference
    with pytest.raises(ValueError, match="view"):
        SceneInference(stub_model(), views=views)


def test_views_and_img_scale_do_not_combine_and_the_default_is_untouched():
    from orientedreppoints_amd.mmdet_models import SceneInference
    with pytest.raises(ValueError, match="views"):
        SceneInference(stub_model(), views=[(None, True)], img_scale=(1333, 960))
    si = SceneInference(stub_model())
    assert si.views is None
    (_, shape), = si.tile_shapes(4096, 4096)
    assert shape is None                               # the single-view native route, as before


def test_views_plan_one_shape_per_scale():
    """Every rate runs all views; the views of one scale share a `_Shape`; a native-size view refuses a scene smaller than a tile."""
    from orientedreppoints_amd.mmdet_models import SceneInference
    views = [(None, False), (None, True), ((1333, 960), False), ((1333, 960), True)]
    si = SceneInference(stub_model(), rates=(1.0, 0.5), views=views, batch=2)
    planned = si.tile_shapes(4096, 4096)
    assert len(planned) == 2 and planned[0][1] is planned[1][1]           # 2048^2 at rate 0.5: the same 1024^2 patches
    aug = planned[0][1]
    assert [f for _, f in aug.views] == [False, True, False, True]
    assert aug.views[0][0] is aug.views[1][0] and aug.views[2][0] is aug.views[3][0]
    assert aug.views[0][0].native and aug.views[0][0].scale_factor == 1.0
    assert aug.views[2][0].new == aug.views[2][0].pad == (960, 960) and aug.views[2][0].scale_factor == 0.9375
    assert [[m['flip'] for m in ms] for ms in aug.metas] == [[False] * 2, [True] * 2, [False] * 2, [True] * 2]
    assert aug.metas[3][0]['scale_factor'] == 0.9375 and aug.metas[3][0]['img_shape'] == (960, 960, 3)
    with pytest.raises(ValueError, match="smaller"):
        si.tile_shapes(4000, 1023)
    assert SceneInference(stub_model(), views=views[2:]).tile_shapes(4000, 1023)[0][1].views[0][0].src == (1024, 1023)
