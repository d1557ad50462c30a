"""Segmentation heads without a GPU: what build_model returns for `masks: true`, the state-dict keys
against the reference's (tests/golden/segm_*.keys.txt), the refusals, and the C ABI's argument
checks (csrc/segm.hip returns KINET_ERR_ARG before it touches a device)."""
import os

import pytest
import torch
import yaml

import segm_refs as R
from kinet_amd import _native as N
from kinet_amd.models import build_model
from kinet_amd.models.config import load_args


@pytest.fixture(scope='module')
def built():
    torch.manual_seed(0)
    return {tag: build_model(R.case_args(tag)) for tag in R.CASES}


def test_build_model_returns_segm_classes(built):
    from kinet_amd.models import (DeformableDETR, DeformableDETRSegm, DeformableDETRSegmTracking, DeformablePostProcess,
                                  PostProcessSegm)
    from kinet_amd.models.detr_tracking import DETRTrackingBase
    from kinet_amd.models.segmentation import DETRSegmBase
    assert type(built['a'][0]) is DeformableDETRSegm
    assert type(built['b'][0]) is DeformableDETRSegmTracking and type(built['c'][0]) is DeformableDETRSegmTracking
    # the reference's MRO (detr_segmentation.py:81, :94)
    assert DeformableDETRSegm.__mro__[:3] == (DeformableDETRSegm, DETRSegmBase, DeformableDETR)
    assert DeformableDETRSegmTracking.__mro__[:4] == (DeformableDETRSegmTracking, DETRSegmBase, DETRTrackingBase,
                                                      DeformableDETR)
    for tag in R.CASES:
        model, criterion, post = built[tag]
        assert type(post['segm']) is PostProcessSegm and post['segm'].threshold == 0.5
        assert type(post['bbox']) is DeformablePostProcess and set(post) == {'bbox', 'segm'}
        assert not any('mask' in k or 'dice' in k for k in criterion.weight_dict)      # no mask losses
        assert model.backbone.num_channels == [256, 512, 1024, 2048] and model.fpn_channels == [1024, 512, 256]
    assert built['c'][0].multi_frame_attention


@pytest.mark.parametrize('tag', list(R.CASES))
def test_state_dict_matches_reference_keys(built, golden_dir, tag):
    want = R.key_shapes(golden_dir, tag)
    got = {k: list(v.shape) for k, v in built[tag][0].state_dict().items()}
    assert sorted(got) == sorted(want)
    assert got == want
    head = {k: v for k, v in got.items() if k.startswith(('bbox_attention.', 'mask_head.'))}
    assert len(head) == 32
    assert head['mask_head.lay1.weight'] == [264, 264, 3, 3] and head['mask_head.adapter1.weight'] == [128, 1024, 1, 1]
    assert head['mask_head.out_lay.weight'] == [1, 16, 3, 3] and head['bbox_attention.k_linear.weight'] == [256, 256]


def test_head_init_is_the_references(built):
    """kaiming_uniform(a=1) weights and zero biases for every conv of the head, xavier + zero bias for q / k."""
    model = built['a'][0]
    for name, m in model.mask_head.named_modules():
        if isinstance(m, torch.nn.Conv2d):
            fan_in = m.in_channels * m.kernel_size[0] * m.kernel_size[1]
            assert float(m.weight.detach().abs().max()) <= (3.0 / fan_in) ** 0.5 + 1e-6, name
            assert float(m.bias.detach().abs().max()) == 0.0
    att = model.bbox_attention
    assert float(att.q_linear.bias.detach().abs().max()) == 0.0 and float(att.k_linear.bias.detach().abs().max()) == 0.0
    assert att.num_heads == 8 and att.normalize_fact == 32 ** -0.5


def test_freeze_detr_freezes_the_detector_only():
    model = build_model(R.case_args('a', freeze_detr=True))[0]
    for n, p in model.named_parameters():
        assert p.requires_grad == n.startswith(('bbox_attention.', 'mask_head.')), n


def test_shipped_masks_configs(golden_dir):
    """The reference's two masks configs (copied settings files) build the Segm classes."""
    from kinet_amd.models import DeformableDETRSegm, DeformableDETRSegmTracking
    for name, cls, extra in (('train_coco_person_masks', DeformableDETRSegm, ()),
                             ('train_mots20', DeformableDETRSegmTracking, ('train_tracking',))):
        with open(os.path.join(golden_dir, 'cfgs', name + '.yaml')) as f:
            cfg = yaml.safe_load(f)
        assert cfg['masks'] is True
        known = {k: v for k, v in cfg.items() if k in vars(load_args())}
        model, _, post = build_model(load_args('train_deformable', *extra, **known))
        assert type(model) is cls and 'segm' in post
        named = load_args('train_deformable', *extra, name)          # the same settings as a named config
        assert all(getattr(named, k) == v for k, v in known.items() if k != 'resume') and named.masks


@pytest.mark.parametrize('over,match', [
    (dict(deformable=False), 'vanilla'),
    (dict(two_stage=True), 'two_stage'),
    (dict(dataset='coco_panoptic'), 'Panoptic'),
])
def test_refusals(over, match):
    with pytest.raises(NotImplementedError, match=match):
        build_model(load_args('train_deformable', masks=True, **over))


def test_vanilla_masks_with_train_detr_raises():
    with pytest.raises(NotImplementedError):
        build_model(load_args('train_detr', masks=True))
    with pytest.raises(NotImplementedError):
        build_model(load_args(masks=True))


def test_tracker_refuses_masks(built):
    from kinet_amd.models.config import TRACKER_CFG
    from kinet_amd.tracker import Tracker
    model, _, post = built['b']
    with pytest.raises(NotImplementedError, match='masks'):
        Tracker(model, post, dict(TRACKER_CFG))
    Tracker(model, {'bbox': post['bbox']}, dict(TRACKER_CFG))


def test_training_forward_raises(built):
    """With autograd on (train or eval mode) the forward names what is missing, before any kernel."""
    model = built['a'][0]
    for mode in (True, False):
        model.train(mode)
        with pytest.raises(NotImplementedError, match='inference'):
            model([torch.zeros(3, 64, 64)])
    model.eval()


def test_criterion_is_unchanged_by_masks(built):
    plain = build_model(load_args('train_deformable', num_queries=R.N_QUERIES))[1]
    assert built['a'][1].weight_dict == plain.weight_dict and built['a'][1].losses == plain.losses


# --------------------------------------------------------------------------- the C ABI's argument checks
def _err(name, *args):
    with pytest.raises(RuntimeError) as e:
        N.call(name, *args)
    return str(e.value)


def test_abi_rejects_bad_arguments_before_any_launch():
    """Null pointers throughout: every call must fail on its arguments, not reach a launch."""
    z = None
    assert 'dtype' in _err('kinet_segm_attention', z, z, z, z, 1, 1, 4, 8, 256, 0.1, 3, z)            # f64
    assert 'heads' in _err('kinet_segm_attention', z, z, z, z, 1, 1, 4, 6, 252, 0.1, 0, z)
    assert 'multiple of heads' in _err('kinet_segm_attention', z, z, z, z, 1, 1, 4, 8, 252, 0.1, 0, z)
    assert 'geometry' in _err('kinet_segm_attention', z, z, z, z, 1, 1, 0, 8, 256, 0.1, 0, z)
    assert 'null' in _err('kinet_segm_attention', z, z, z, z, 1, 1, 4, 8, 256, 0.1, 0, z)
    assert '8 attention channels' in _err('kinet_segm_lay1', z, z, z, z, 1, 0, 1, 1, 4, 4, 16, 264, 0, z)
    assert 'Cout' in _err('kinet_segm_lay1', z, z, z, z, 1, 0, 1, 1, 4, 4, 8, 2048, 0, z)
    assert 'outside' in _err('kinet_segm_lay1', z, z, z, z, 2, 5, 3, 2, 4, 4, 8, 264, 0, z)         # rows 5..6 of 6
    assert 'null' in _err('kinet_segm_lay1', z, z, z, z, 1, 0, 1, 1, 4, 4, 8, 264, 0, z)
    assert 'multiple of groups' in _err('kinet_segm_gn_relu_up_add', z, z, z, z, z, 1, 0, 1, 1, 4, 4, 4, 4, 260, 8, 1e-5, 0, z, z)
    assert 'multiple of groups and of 8' in _err('kinet_segm_gn_relu_up_add', z, z, z, z, z, 1, 0, 1, 1, 4, 4, 4, 4, 36, 4, 1e-5, 0, z, z)
    assert 'aligned' in _err('kinet_segm_gn_relu_up_add', 16, 8, 8, z, 24, 1, 0, 1, 1, 4, 4, 4, 4, 16, 8, 1e-5, 0, 8, z)
    assert 'output has the input' in _err('kinet_segm_gn_relu_up_add', z, z, z, z, z, 1, 0, 1, 1, 4, 4, 8, 8, 16, 8, 1e-5, 0, z, z)
    assert 'outside' in _err('kinet_segm_gn_relu_up_add', z, z, z, z, z, 4, 3, 3, 2, 4, 4, 4, 4, 16, 8, 1e-5, 0, z, z)
    assert 'workspace' in _err('kinet_segm_gn_relu_up_add', 8, 8, 8, z, 8, 1, 0, 1, 1, 4, 4, 4, 4, 16, 8, 1e-5, 0, z, z)
    assert 'C must' in _err('kinet_segm_out_conv', z, z, z, z, 1, 4, 4, 128, 0, z)
    assert 'null' in _err('kinet_segm_out_conv', z, z, z, z, 1, 4, 4, 16, 0, z)
    assert 'inside' in _err('kinet_segm_postprocess', z, z, 1, 4, 4, 16, 16, 17, 16, 32, 32, 0.5, 0, z)
    assert 'geometry' in _err('kinet_segm_postprocess', z, z, 1, 4, 4, 16, 16, 16, 16, 0, 32, 0.5, 0, z)
    assert 'null' in _err('kinet_segm_postprocess', z, z, 1, 4, 4, 16, 16, 16, 16, 32, 32, 0.5, 0, z)


def test_abi_empty_calls_are_no_ops():
    z = None
    assert N.call('kinet_segm_attention', z, z, z, z, 2, 0, 4, 8, 256, 0.1, 0, z) == 0
    assert N.call('kinet_segm_lay1', z, z, z, z, 0, 0, 1, 1, 4, 4, 8, 264, 0, z) == 0
    assert N.call('kinet_segm_gn_relu_up_add', z, z, z, z, z, 0, 0, 1, 1, 4, 4, 4, 4, 16, 8, 1e-5, 0, z, z) == 0
    assert N.call('kinet_segm_out_conv', z, z, z, z, 0, 4, 4, 16, 0, z) == 0
    assert N.call('kinet_segm_postprocess', z, z, 0, 4, 4, 16, 16, 16, 16, 32, 32, 0.5, 0, z) == 0


def test_gn_workspace_size():
    L = N.lib()
    assert L.kinet_segm_gn_workspace(6, 91, 8) == 6 * 8 * (3 + 2 * 1)
    assert L.kinet_segm_gn_workspace(3, 257, 8) == 3 * 8 * (3 + 2 * 2)
    assert L.kinet_segm_gn_workspace(0, 91, 8) == 0
