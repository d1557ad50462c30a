"""Vanilla DETR (config 1, the reference's default `deformable: false`) builds through
build_model with the reference's module names and shapes.  Host only; the key files come from
the reference model (tests/golden/make_golden_detr.py)."""
import os

import pytest
import torch
from torch import nn

from kinet_amd.models import build_model
from kinet_amd.models.config import load_args


def _keys(golden_dir, name):
    out = []
    for ln in open(os.path.join(golden_dir, name)):
        k, *s = ln.split()
        out.append((k, tuple(int(x) for x in s)))
    return out


@pytest.fixture(scope='module')
def built():
    return {'a': build_model(load_args()),
            'b': build_model(load_args('train_detr')),
            'c': build_model(load_args('train_detr', tracking=True))}


def test_build_model_constructs_vanilla_detr(built):
    from kinet_amd.models.detr import DETR
    from kinet_amd.models.detr_tracking import DETRTracking, DETRTrackingBase
    from kinet_amd.models.transformer import Transformer
    for tag in 'abc':
        model, criterion, post = built[tag]
        assert isinstance(model, DETR) and isinstance(model.transformer, Transformer)
        assert criterion is not None
    assert type(built['a'][0]) is DETR and type(built['b'][0]) is DETR
    assert type(built['c'][0]) is DETRTracking and isinstance(built['c'][0], DETRTrackingBase)
    assert built['a'][0].hidden_dim == 256 and built['a'][0].num_queries == 100
    assert built['b'][0].hidden_dim == 288 and built['b'][0].num_queries == 500


@pytest.mark.parametrize('tag,keyfile', [('a', 'detr_vanilla_a.keys.txt'), ('b', 'detr_vanilla_b.keys.txt'),
                                         ('c', 'detr_vanilla_b.keys.txt')])
def test_state_dict_matches_reference(built, golden_dir, tag, keyfile):
    """Same keys, same order, same shapes as the reference DETR / DETRTracking."""
    ref = _keys(golden_dir, keyfile)
    got = [(k, tuple(v.shape)) for k, v in built[tag][0].state_dict().items()]
    assert [k for k, _ in got] == [k for k, _ in ref]
    assert got == ref
    names = {k for k, _ in got}
    for k in ('transformer.encoder.layers.5.self_attn.in_proj_weight',
              'transformer.decoder.layers.5.multihead_attn.out_proj.bias', 'transformer.decoder.norm.weight',
              'class_embed.weight', 'bbox_embed.layers.2.bias', 'query_embed.weight', 'input_proj.weight',
              'backbone.0.body.layer4.2.conv3.weight'):
        assert k in names, k


def test_input_proj_is_bare_conv(built):
    for tag in 'abc':
        proj = built[tag][0].input_proj
        assert isinstance(proj, nn.Conv2d) and proj.kernel_size == (1, 1) and proj.in_channels == 2048


def test_postprocessor_is_softmax_postprocess(built):
    from kinet_amd.models import DeformablePostProcess, PostProcess
    for tag in 'abc':
        assert type(built[tag][2]['bbox']) is PostProcess
    assert type(build_model(load_args(focal_loss=True))[2]['bbox']) is DeformablePostProcess


def test_num_classes_follow_focal_loss():
    assert build_model(load_args())[0].class_embed.out_features == 92
    assert build_model(load_args(focal_loss=True))[0].class_embed.out_features == 91


@pytest.mark.parametrize('over', [dict(masks=True), dict(pre_norm=True), dict(activation='gelu'),
                                  dict(track_attention=True)])
def test_unbuilt_variants_still_raise(over):
    with pytest.raises(NotImplementedError):
        build_model(load_args(**over))
    with pytest.raises(NotImplementedError):
        build_model(load_args('train_detr', **over))


def test_broken_reference_multi_frame_branch_raises():
    """detr.py:120-123 calls .flatten on a list; build_model never passes the flags (as the
    reference's does not), the class raises for the pair."""
    from kinet_amd.models.backbone import build_backbone
    from kinet_amd.models.detr import DETR
    from kinet_amd.models.transformer import build_transformer
    args = load_args()
    assert args.multi_frame_encoding and not build_model(args)[0].multi_frame_encoding
    with pytest.raises(NotImplementedError):
        DETR(build_backbone(args), build_transformer(args), 91, 100, multi_frame_encoding=True,
             multi_frame_attention=True)


def test_training_forward_raises_clearly(built):
    """Training config 1 is not built: with autograd on the forward names that, before any kernel."""
    model = built['a'][0]
    with pytest.raises(NotImplementedError, match='inference'):
        model([torch.zeros(3, 64, 64)])


def test_named_config_train_detr():
    a = load_args('train_detr')
    assert (a.deformable, a.multi_frame_encoding, a.num_queries, a.hidden_dim, a.activation) == \
        (False, False, 500, 288, 'relu')
