"""Tracker masks without a GPU: the argument checks of kinet_segm_track_resolve (csrc/segm.hip returns
KINET_ERR_ARG before it touches a device), the wrapper's host checks, and the tracker's opt-in."""
import pytest
import torch

from kinet_amd import _native as N
from kinet_amd import kernels as K

GEO = (26, 50, 104, 200, 88, 136, 131, 203)     # h, w, max_h, max_w, img_h, img_w, oh, ow


def _err(*args):
    with pytest.raises(RuntimeError) as e:
        N.call('kinet_segm_track_resolve', *args)
    return str(e.value)


def test_exported():
    assert N.exported('kinet_segm_track_resolve')


def test_abi_rejects_bad_arguments_before_any_launch():
    """Null pointers throughout: every call must fail on its arguments, not reach a launch."""
    z = None
    assert '32767' in _err(z, z, z, z, 32768, 1, *GEO, 0.5, z)
    assert 'inside' in _err(z, z, z, z, 2, 1, 26, 50, 104, 200, 105, 136, 131, 203, 0.5, z)     # crop taller than max
    assert 'inside' in _err(z, z, z, z, 2, 1, 26, 50, 104, 200, 88, 201, 131, 203, 0.5, z)      # crop wider than max
    assert 'inside' in _err(z, z, z, z, 2, 1, 26, 50, 104, 200, 0, 136, 131, 203, 0.5, z)
    for bad in ((0, 50, 104, 200, 88, 136, 131, 203), (26, 50, 104, 200, 88, 136, 0, 203),
                (26, 50, 104, 200, 88, 136, 131, -1), (26, 50, 0, 200, 88, 136, 131, 203)):
        assert 'geometry' in _err(z, z, z, z, 2, 1, *bad, 0.5, z)
    assert 'geometry' in _err(z, z, z, z, -1, 1, *GEO, 0.5, z)
    assert 'geometry' in _err(z, z, z, z, 2, -1, *GEO, 0.5, z)
    assert 'null pointer (labels)' in _err(z, z, z, z, 2, 1, *GEO, 0.5, z)
    assert 'null pointer (src)' in _err(z, z, z, 64, 2, 1, *GEO, 0.5, z)
    assert 'null pointer (logits)' in _err(z, 64, z, 64, 2, 1, *GEO, 0.5, z)
    assert 'two buffers' in _err(64, 64, 128, 128, 2, 1, *GEO, 0.5, z)


def test_abi_empty_operands_need_no_pointer():
    """T == 0 needs no src and n == 0 no logits: with neither, the one operand still asked for is the label
    map, which every call writes whole (T == 0 writes -1 everywhere: tests/test_mots_direct_gpu.py)."""
    z = None
    assert 'null pointer (labels)' in _err(z, z, z, z, 0, 0, *GEO, 0.5, z)
    assert 'null pointer (labels)' in _err(z, z, z, z, 0, 5, *GEO, 0.5, z)
    assert 'null pointer (src)' in _err(z, z, z, 64, 3, 0, *GEO, 0.5, z)          # n == 0: past the logits check


def test_wrapper_needs_a_gpu_tensor():
    with pytest.raises(RuntimeError, match='GPU only'):
        K.segm_track_resolve(torch.zeros(1, 26, 50), [0], None, (104, 200), (88, 136), (131, 203))


def _tracker(cfg_over, post_keys=('bbox', 'segm'), cls=None):
    from fake_mask_detector import FakeMaskDetector
    from fake_detector import TRACKER_CFGS
    from kinet_amd.models import DeformablePostProcess, PostProcessSegm
    from kinet_amd.tracker import Tracker
    post = {'bbox': DeformablePostProcess(), 'segm': PostProcessSegm()}
    return (cls or Tracker)(FakeMaskDetector(), {k: post[k] for k in post_keys}, dict(TRACKER_CFGS['default'], **cfg_over))


def test_tracker_with_masks_is_constructible():
    t = _tracker({'masks': True})
    assert t.masks
    t.reset()
    assert t.tracks == [] and t.get_results() == {}


def test_tracker_masks_are_opt_in():
    from kinet_amd.models.config import TRACKER_CFG
    assert 'masks' not in TRACKER_CFG
    with pytest.raises(NotImplementedError, match=r"masks.*tracker_cfg\['masks'\]"):
        _tracker({})
    with pytest.raises(NotImplementedError, match='masks'):
        _tracker({'masks': False})
    assert not _tracker({}, post_keys=('bbox',)).masks
    with pytest.raises(ValueError, match='segm'):
        _tracker({'masks': True}, post_keys=('bbox',))


def test_tracker_masks_refuse_a_blob_without_size():
    from fake_mask_detector import mask_blobs
    t = _tracker({'masks': True})
    t.reset()
    blob = mask_blobs(0, 1)[0]
    del blob['size']
    with pytest.raises(ValueError, match='size'):
        t.step(blob)


def test_tracker_kinematic_keeps_refusing_masks():
    from fake_detector import KINEMATIC_CFGS, FakeKinetDetector, kinematic_args
    from kinet_amd.models import DeformablePostProcess, PostProcessSegm
    from kinet_amd.tracker import TrackerKinematic
    post = {'bbox': DeformablePostProcess(), 'segm': PostProcessSegm()}
    for cfg in (dict(KINEMATIC_CFGS['kinet'], masks=True), KINEMATIC_CFGS['kinet']):
        with pytest.raises(NotImplementedError, match='masks'):
            TrackerKinematic(FakeKinetDetector(), post, cfg, kinematic_args())


def test_fake_mask_detector_keeps_the_box_stream():
    """The masks come from a separate generator: boxes, logits and embeddings are FakeDetector's."""
    from fake_detector import FakeDetector
    from fake_mask_detector import MASK_HW, FakeMaskDetector
    a, b = FakeDetector(seed=1), FakeMaskDetector(seed=1)
    tq = {'track_query_boxes': torch.rand(3, 4), 'track_query_hs_embeds': torch.randn(3, 16)}
    for targets in (None, [tq]):
        oa, ob = a(None, targets)[0], b(None, targets)[0]
        for k in oa:
            assert torch.equal(oa[k], ob[k]), k
        n = oa['pred_boxes'].shape[1]
        assert ob['pred_masks'].shape == (1, n) + MASK_HW and float(ob['pred_masks'].abs().max()) < 8
