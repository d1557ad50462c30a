"""kinet_amd.tracker.MultiTracker: several sequences in lock-step on one batched detector forward
must track exactly as one Tracker per sequence does.  On the fixtures' fake detector (batched and ragged
through multi_track_refs.BatchedFakeDetector, whose placeholder rows are NaN) every sequence reproduces
tests/golden/tracker.npz under test_tracker_matches_reference's assertions; on the real small Deformable
tracking model S = 1 reproduces Tracker.  Also: retire(), the device -> host sync budget and what the class
refuses."""
import os

import numpy as np
import pytest
import torch

import multi_track_refs as R

pytestmark = pytest.mark.gpu

CFGS = ['default', 'reid_lsa', 'public_iou', 'reid_greedy']
FRAMES = 20


def _multi(name, seeds, **kw):
    from fake_detector import TRACKER_CFGS
    from kinet_amd.models import DeformablePostProcess
    from kinet_amd.tracker import MultiTracker
    det = R.BatchedFakeDetector(seeds).cuda()
    return MultiTracker(det, {'bbox': DeformablePostProcess()}, TRACKER_CFGS[name], len(seeds), **kw), det


def _assert_fixture(d, name, seq, results, q=None, frames=None):
    from fake_detector import flatten_results
    ids, vals = flatten_results(results)
    want_ids, want_vals = d[f'{name}_{seq}_ids'], d[f'{name}_{seq}_vals']
    if frames is not None:
        sel = want_ids[:, 0] < frames
        want_ids, want_vals = want_ids[sel], want_vals[sel]
    np.testing.assert_array_equal(ids.numpy(), want_ids)
    np.testing.assert_allclose(vals.numpy(), want_vals, rtol=1e-5, atol=1e-3)
    if q is not None:
        assert q.num_reids == int(d[f'{name}_{seq}_reids'])
        assert q.track_num == int(d[f'{name}_{seq}_tracks'])


@pytest.mark.parametrize('name', CFGS)
def test_two_sequences_match_the_fixture(golden_dir, name):
    d = np.load(os.path.join(golden_dir, 'tracker.npz'))
    tracker, det = _multi(name, [0, 1])
    R.run_multi(tracker, det, [0, 1], FRAMES)
    # the sequences hold different track counts, so placeholder (NaN) rows occurred
    assert any(len(set(ks)) > 1 for ks in det.calls)
    res = tracker.get_results()
    for seq in (0, 1):
        _assert_fixture(d, name, seq, res[seq], tracker.sequence(seq))
        assert tracker.sequence(seq).frame_index == FRAMES


@pytest.mark.parametrize('name', CFGS)
def test_three_slots_two_equal(golden_dir, name):
    from fake_detector import flatten_results
    d = np.load(os.path.join(golden_dir, 'tracker.npz'))
    tracker, det = _multi(name, [1, 0, 1])
    R.run_multi(tracker, det, [1, 0, 1], FRAMES)
    res = tracker.get_results()
    a, b = flatten_results(res[0]), flatten_results(res[2])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _assert_fixture(d, name, 1, res[0], tracker.sequence(0))
    _assert_fixture(d, name, 0, res[1], tracker.sequence(1))


@pytest.mark.parametrize('name', ['default', 'reid_lsa'])
def test_retire(golden_dir, name):
    d = np.load(os.path.join(golden_dir, 'tracker.npz'))
    tracker, det = _multi(name, [0, 1])
    R.run_multi(tracker, det, [0, 1], FRAMES, retire_at=(1, 10))
    res = tracker.get_results()
    _assert_fixture(d, name, 0, res[0], tracker.sequence(0))
    _assert_fixture(d, name, 1, res[1], frames=10)
    assert tracker.live_sequences() == [0] and tracker.sequence(1).frame_index == 10
    with pytest.raises(ValueError):
        tracker.retire(1)


def test_retire_drops_the_cached_feature_rows():
    from fake_detector import TRACKER_CFGS
    from kinet_amd.models import DeformablePostProcess
    from kinet_amd.models.misc import NestedTensor
    from kinet_amd.tracker import MultiTracker
    tracker = MultiTracker(R.BatchedFakeDetector([0, 1, 2]).cuda(), {'bbox': DeformablePostProcess()},
                           TRACKER_CFGS['default'], 3)
    t = torch.arange(3 * 2 * 4 * 5, dtype=torch.float32, device='cuda').view(3, 2, 4, 5)
    m = torch.zeros(3, 4, 5, dtype=torch.bool, device='cuda')
    m[1, :, 3:] = True
    tracker._prev_features.append([NestedTensor(t.clone(), m.clone(), ((4, 5), (4, 3), (4, 5)))])
    tracker.retire(1)
    f = tracker._prev_features[0][0]
    assert torch.equal(f.tensors, t[[0, 2]]) and torch.equal(f.mask, m[[0, 2]]) and f.sizes == ((4, 5), (4, 5))
    tracker.retire(0)
    assert torch.equal(f.tensors, t[[2]]) and f.sizes == ((4, 5),)


def test_sync_budget():
    tracker, det = _multi('reid_lsa', [0, 1])
    two = R.run_multi(tracker, det, [0, 1], FRAMES)
    tracker, det = _multi('reid_lsa', [0, 1, 0, 1])
    four = R.run_multi(tracker, det, [0, 1, 0, 1], FRAMES)
    assert max(two) <= 4 and two == four, (two, four)
    assert max(two) == 4          # the cfg re-identifies by embedding distance: every transfer occurs
    tracker, det = _multi('default', [0, 1])
    default = R.run_multi(tracker, det, [0, 1], FRAMES)
    assert max(default) <= 3, default       # no inactive tracks (inactive_patience -1): no distances
    assert tracker.sync_count == sum(default)


# ---------------------------------------------------------------------------------- real detector
@pytest.fixture(scope='module')
def real(golden_dir):
    """The small Deformable tracking model of test_model_gpu.py's tracking tests, f32, its class bias
    calibrated on frame 0 so that about ten queries pass the detection threshold as persons."""
    import math
    from kinet_amd.models import DeformablePostProcess
    from kinet_amd.models.config import TRACKER_CFG
    d = dict(np.load(os.path.join(golden_dir, 'detr_tracking_mf_small.npz')))
    model = R.small_tracking_model(golden_dir)
    model.set_compute_dtype(torch.float32)
    frames = [torch.from_numpy(d['frame0']).cuda(), torch.from_numpy(d['frame1']).cuda()]
    with torch.no_grad():
        for ce in model.class_embed:
            ce.bias.fill_(-20.0)
            ce.bias[0] = 0.0
        logits = model([frames[0]])[0]['pred_logits'][0, :, 0].float()
        thr = math.log(TRACKER_CFG['detection_obj_score_thresh'] / (1 - TRACKER_CFG['detection_obj_score_thresh']))
        b = thr - torch.sort(logits, descending=True)[0][10].item()
        for ce in model.class_embed:
            ce.bias[0] = b
    h, w = frames[0].shape[-2:]
    blobs = [{'img': frames[f % 2][None], 'orig_size': torch.tensor([[h * 4, w * 4]], device='cuda'),
              'dets': [torch.zeros(0, 4)]} for f in range(6)]
    cfg = dict(TRACKER_CFG, track_nms_thresh=0.7, detection_nms_thresh=0.7)
    return model, {'bbox': DeformablePostProcess()}, cfg, blobs


def test_real_detector_one_sequence_matches_tracker(real):
    from fake_detector import flatten_results
    from kinet_amd.tracker import MultiTracker, Tracker
    model, post, cfg, blobs = real
    one = Tracker(model, post, cfg)
    one.reset()
    for blob in blobs:
        one.step(blob)
    multi = MultiTracker(model, post, cfg, 1)
    for blob in blobs:
        multi.step([blob])
    ids, vals = flatten_results(one.get_results())
    mids, mvals = flatten_results(multi.get_results()[0])
    assert len(ids) >= 6                                   # the calibration let queries pass
    assert len({int(t) for t in ids[:, 1]}) >= 2
    np.testing.assert_array_equal(mids.numpy(), ids.numpy())
    np.testing.assert_allclose(mvals.numpy(), vals.numpy(), rtol=1e-5, atol=1e-3)
    assert multi.sequence(0).track_num == one.track_num and multi.sequence(0).num_reids == one.num_reids


def test_real_detector_two_equal_slots(real):
    from fake_detector import flatten_results
    from kinet_amd.tracker import MultiTracker
    model, post, cfg, blobs = real
    multi = MultiTracker(model, post, cfg, 2)
    for blob in blobs:
        multi.step([blob, blob])
    a, b = (flatten_results(r) for r in multi.get_results())
    assert len(a[0]) >= 6
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------- refusals
def test_refusals():
    from fake_detector import KINEMATIC_CFGS, TRACKER_CFGS
    from kinet_amd.models import DeformablePostProcess, build_model
    from kinet_amd.models.config import load_args
    from kinet_amd.models.deformable_detr import PostProcess
    from kinet_amd.tracker import MultiTracker
    det = R.BatchedFakeDetector([0]).cuda()
    post, cfg = {'bbox': DeformablePostProcess()}, TRACKER_CFGS['default']
    with pytest.raises(NotImplementedError):
        MultiTracker(det, post, dict(cfg, masks=True), 1)
    with pytest.raises(NotImplementedError):
        MultiTracker(det, dict(post, segm=object()), cfg, 1)
    with pytest.raises(NotImplementedError):
        MultiTracker(det, {'bbox': PostProcess()}, cfg, 1)
    with pytest.raises(NotImplementedError):
        MultiTracker(det, post, cfg, 1, generate_attention_maps=True)
    kinet, _, kpost = build_model(load_args('train_kinet', tracking=True, device='cuda'))
    with pytest.raises(NotImplementedError):
        MultiTracker(kinet, {'bbox': DeformablePostProcess()}, KINEMATIC_CFGS['kinet'], 1)
    MultiTracker(det, post, cfg, 1)        # (the plain construction passes)


def test_vanilla_detr_refuses_ragged_track_queries():
    from kinet_amd.models.detr import DETR
    t = [{'track_query_hs_embeds': torch.zeros(1, 4), 'track_query_boxes': torch.zeros(1, 4),
          'track_queries_placeholder_mask': torch.zeros(3, dtype=torch.bool)}]
    with pytest.raises(NotImplementedError):
        DETR.forward(None, [torch.zeros(3, 8, 8)], t)
