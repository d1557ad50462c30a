"""Two-stage Deformable DETR without a GPU: the model builds with the reference's state_dict
(tests/golden/two_stage_{a,b}.keys.txt, written by make_golden_two_stage.py from the reference
model), the unsupported combinations are refused when the model is built, and the C ABI of
csrc/two_stage.hip rejects bad arguments before any device work."""
import ctypes
import os

import pytest
import torch


def _args(**over):
    from kinet_amd.models.config import load_args
    return load_args('train_deformable', **dict(dict(two_stage=True, num_queries=100), **over))


def _keys(golden_dir, name):
    return [(k, tuple(int(x) for x in s)) for k, *s in (ln.split() for ln in open(os.path.join(golden_dir, name)))]


@pytest.mark.parametrize('tag,refine', [('a', True), ('b', False)])
def test_two_stage_state_dict_equals_the_reference(golden_dir, tag, refine):
    from kinet_amd.models import build_model
    model, _, _ = build_model(_args(with_box_refine=refine))
    got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert got == _keys(golden_dir, f'two_stage_{tag}.keys.txt')
    names = dict(got)
    assert 'transformer.reference_points.weight' not in names
    assert names['transformer.enc_output.weight'] == (256, 256)
    assert names['transformer.pos_trans.weight'] == (512, 512)
    assert names['transformer.pos_trans_norm.weight'] == (512,)
    # one head pair more than decoder layers: the proposal generator's
    assert len(model.class_embed) == len(model.bbox_embed) == 7
    assert model.transformer.decoder.class_embed is model.class_embed
    if refine:
        assert model.transformer.decoder.bbox_embed is model.bbox_embed
        assert len({id(m) for m in model.bbox_embed}) == 7
    else:
        assert model.transformer.decoder.bbox_embed is None
        assert len({id(m) for m in model.bbox_embed}) == 1
    # deformable_detr.py:112-113: every box head's w / h bias back to 0
    for m in model.bbox_embed:
        assert not m.layers[-1].bias.data[2:].any()
    # the DETR base's d-wide embedding the reference keeps (and never reads) when two_stage
    assert names['query_embed.weight'] == (100, 256)


def test_one_stage_model_is_unchanged(golden_dir):
    from kinet_amd.models import build_model
    from kinet_amd.models.config import load_args
    model, _, _ = build_model(load_args('train_deformable'))
    got = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert got == dict(_keys(golden_dir, 'detr_config2_small.keys.txt'))
    assert got['query_embed.weight'] == (300, 512)
    assert not hasattr(model.transformer, 'enc_output')


def test_two_stage_refusals():
    from kinet_amd.models import build_model
    with pytest.raises(NotImplementedError, match='hidden_dim 256'):
        build_model(_args(hidden_dim=288))
    with pytest.raises(NotImplementedError, match='tracking'):
        build_model(_args(tracking=True))
    with pytest.raises(NotImplementedError, match='multi_frame_attention'):
        build_model(_args(multi_frame_attention=True))
    with pytest.raises(NotImplementedError, match='1024'):
        build_model(_args(num_queries=1025))


def test_two_stage_training_forward_raises():
    from kinet_amd.models import build_model
    model, _, _ = build_model(_args())
    frames = [torch.zeros(3, 64, 64)]
    with pytest.raises(NotImplementedError, match='inference'):
        model(frames)                      # autograd enabled
    model.train()
    with pytest.raises(NotImplementedError, match='inference'), torch.no_grad():
        model(frames)                      # train mode (active dropout)
    with pytest.raises(NotImplementedError, match='inference'):
        model.transformer.forward_flat(None, None, None)


def test_two_stage_entry_points_validate_arguments():
    """include/kinet_two_stage.h: KINET_ERR_ARG and a message before touching the device."""
    from kinet_amd import _native
    L = _native.lib()
    fake = 4096   # never dereferenced: every call below fails validation first

    def err(rc):
        assert rc != 0
        return L.kinet_last_error().decode()

    # top-k
    assert 'k 1025 not in [1, 1024]' in err(L.kinet_topk_rows(fake, 4096, 1, 2, 4096, 1025, fake, None))
    assert 'k 0 not in' in err(L.kinet_topk_rows(fake, 4096, 1, 2, 4096, 0, fake, None))
    assert 'S 99 must be in [k = 100' in err(L.kinet_topk_rows(fake, 99, 1, 2, 99, 100, fake, None))
    assert 'null pointer' in err(L.kinet_topk_rows(None, 4096, 1, 2, 4096, 100, fake, None))
    assert 'null pointer' in err(L.kinet_topk_rows(fake, 4096, 1, 2, 4096, 100, None, None))
    assert 'strides' in err(L.kinet_topk_rows(fake, 4096, 0, 2, 4096, 100, fake, None))
    # proposals
    hw = (ctypes.c_int * 4)(4, 6, 2, 3)
    assert 'null pointer' in err(L.kinet_two_stage_proposals(None, 2, None, fake, fake, 1, 30, None))
    assert 'null pointer' in err(L.kinet_two_stage_proposals(hw, 2, None, None, fake, 1, 30, None))
    assert 'null pointer' in err(L.kinet_two_stage_proposals(hw, 2, None, fake, None, 1, 30, None))
    assert 'cover 30 tokens, S is 31' in err(L.kinet_two_stage_proposals(hw, 2, None, fake, fake, 1, 31, None))
    assert 'levels 17 not in' in err(L.kinet_two_stage_proposals(hw, 17, None, fake, fake, 1, 30, None))
    bad = (ctypes.c_int * 4)(4, 0, 2, 3)
    assert 'bad level 0 shape' in err(L.kinet_two_stage_proposals(bad, 2, None, fake, fake, 1, 30, None))
    # queries
    assert 'null pointer' in err(L.kinet_two_stage_queries(fake, None, fake, fake, fake, 1, 400, 100, 0, None))
    assert 'k 1025' in err(L.kinet_two_stage_queries(fake, fake, fake, fake, fake, 1, 4000, 1025, 0, None))
    assert 'k <= S' in err(L.kinet_two_stage_queries(fake, fake, fake, fake, fake, 1, 50, 100, 0, None))
    assert 'unsupported dtype 3' in err(L.kinet_two_stage_queries(fake, fake, fake, fake, fake, 1, 400, 100, 3, None))
    # glue
    assert 'null pointer' in err(L.kinet_two_stage_fill_rows(fake, None, fake, 10, 256, 1, None))
    assert 'multiple of 16' in err(L.kinet_two_stage_fill_rows(fake, fake, fake, 10, 257, 0, None))
    assert '16-byte aligned' in err(L.kinet_two_stage_fill_rows(fake + 4, fake, fake, 10, 256, 0, None))
    assert 'null pointer' in err(L.kinet_two_stage_boxes(fake, fake, None, fake, 10, None))
    assert '16-byte aligned' in err(L.kinet_two_stage_boxes(fake, fake + 8, fake, fake, 10, None))


def test_two_stage_wrappers_refuse_cpu_tensors():
    from kinet_amd import kernels as K
    with pytest.raises(RuntimeError, match='GPU only'):
        K.topk_rows(torch.zeros(2, 300), 100)
    with pytest.raises(RuntimeError, match='GPU only'):
        K.two_stage_queries(torch.zeros(1, 300, 4), torch.zeros(1, 100, dtype=torch.int64), torch.float32)
