"""kinet_amd.tracker.MultiTracker with segmentation masks (tracker_cfg['masks'], MOTS): several sequences in
lock-step must carry exactly the masks one Tracker per sequence carries.

  * on the fixtures' fake detector with masks (multi_mots_refs.BatchedFakeMaskDetector, NaN placeholder rows)
    every sequence reproduces tests/golden/tracker_masks.npz under test_tracker_masks_match_reference's
    assertions, and every mask bit of a Tracker with masks run beside it on the plain FakeMaskDetector (both
    run the same segm_prob); `reid_lsa` terminates after two missed frames, so stale slots occur;
  * the device -> host sync budget (five per step, whatever S is), retire();
  * the real masks model (segm_refs case b): S = 1 against Tracker, two equal slots, ragged frame orders
    through mask_logits_rows against the full pred_masks, and what mask_logits_rows is asked for;
  * what the class still refuses.
"""
import numpy as np
import pytest
import torch

import multi_mots_refs as M
import segm_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def single(golden_dir):
    """Tracker's own results per (cfg, sequence), computed once."""
    d = M.load_fixture(golden_dir)
    cache = {}

    def get(name, seq):
        if (name, seq) not in cache:
            cache[name, seq] = M.run_single(name, int(d['mask_seed']), seq, int(d['frames']))
        return cache[name, seq]
    return get


def _assert_equals_tracker(ids, got, res_single):
    from fake_detector import flatten_results
    sid, _ = flatten_results(res_single)
    assert torch.equal(sid, ids)
    for (f, t, _), m in zip(ids.tolist(), got):
        assert np.array_equal(m, res_single[t][f]['mask']), (f, t)


@pytest.mark.parametrize('name', ['default', 'reid_lsa'])
@pytest.mark.parametrize('seeds', [[0, 1], [1, 0, 1]])
def test_sequences_match_the_fixture_and_tracker(golden_dir, single, name, seeds):
    d = M.load_fixture(golden_dir)
    frames = int(d['frames'])
    tracker, det = M.multi(name, int(d['mask_seed']), seeds)
    M.run_multi(tracker, det, seeds, frames)
    # the sequences hold different track counts, so placeholder (NaN) rows occurred
    assert any(len(set(ks)) > 1 for ks in det.calls)
    res = tracker.get_results()
    for slot, seq in enumerate(seeds):
        ids, got = M.assert_fixture(d, name, seq, res[slot], tracker.sequence(slot))
        assert tracker.sequence(slot).frame_index == frames
        _assert_equals_tracker(ids, got, single(name, seq))


def test_sync_budget(golden_dir):
    d = M.load_fixture(golden_dir)
    frames, ms = int(d['frames']), int(d['mask_seed'])
    tracker, det = M.multi('reid_lsa', ms, [0, 1])
    two = M.run_multi(tracker, det, [0, 1], frames)
    tracker, det = M.multi('reid_lsa', ms, [0, 1, 0, 1])
    four = M.run_multi(tracker, det, [0, 1, 0, 1], frames)
    assert max(two) <= 5 and two == four, (two, four)
    assert max(two) == 5            # the cfg re-identifies by embedding distance: every transfer occurs
    assert tracker.sync_count == sum(four)


@pytest.mark.parametrize('name', ['default', 'reid_lsa'])
def test_retire(golden_dir, name):
    d = M.load_fixture(golden_dir)
    tracker, det = M.multi(name, int(d['mask_seed']), [0, 1])
    M.run_multi(tracker, det, [0, 1], int(d['frames']), retire_at=(1, 7))
    res = tracker.get_results()
    M.assert_fixture(d, name, 0, res[0], tracker.sequence(0))
    M.assert_fixture(d, name, 1, res[1], frames=7)
    assert tracker.live_sequences() == [0] and tracker.sequence(1).frame_index == 7
    assert tracker.sequence(1).map_off is None


def test_a_frame_without_tracks_launches_and_copies_nothing(golden_dir):
    from fake_detector import TRACKER_CFGS
    from fake_mask_detector import mask_blobs
    from kinet_amd import _native as N
    from kinet_amd.models import DeformablePostProcess, PostProcessSegm
    from kinet_amd.tracker import MultiTracker
    det = M.BatchedFakeMaskDetector(0, [0, 1]).cuda()
    cfg = dict(TRACKER_CFGS['default'], masks=True, detection_obj_score_thresh=2.0)     # no score passes
    tracker = MultiTracker(det, {'bbox': DeformablePostProcess(), 'segm': PostProcessSegm()}, cfg, 2)
    blobs = [mask_blobs(s, 1, device='cuda')[0] for s in (0, 1)]
    N.trace_begin()
    tracker.step(blobs)
    names = [t[0] for t in N.trace_end()]
    assert tracker.sync_count == 1 and not any('segm' in n for n in names), names
    assert tracker.get_results() == [{}, {}]


# ---------------------------------------------------------------------------------- real model
NET_HW, ORIG_HW = (104, 200), (157, 301)


class _FullMasks(torch.nn.Module):
    """The masks model as a detector that returns pred_masks itself (no mask_logits_rows attribute)."""

    def __init__(self, model):
        super().__init__()
        self.model = model
        self.num_queries, self.overflow_boxes = model.num_queries, model.overflow_boxes

    def forward(self, img, targets=None, prev_features=None):
        return self.model(img, targets, prev_features)


@pytest.fixture(scope='module')
def real(golden_dir):
    """Case b's model with the other classes silenced and the threshold that lets about six queries pass on
    the first frame (test_mots_gpu.test_tracker_over_segm_model's choices); the biases are put back after."""
    import os
    from fake_detector import TRACKER_CFGS
    d = np.load(os.path.join(golden_dir, 'segm_b.npz'))
    model, post = R.build_case(golden_dir, 'b', int(d['seed']))
    model = model.cuda()
    model.tracking()
    g = torch.Generator().manual_seed(4201)
    frames = [torch.randn(1, 3, *NET_HW, generator=g).cuda() for _ in range(4)]
    biases = [ce.bias.detach().clone() for ce in model.class_embed]
    with torch.no_grad():
        for ce in model.class_embed:
            ce.bias.fill_(-20.0)
            ce.bias[0] = 0.0
        r0 = post['bbox'](model(frames[0])[0], torch.tensor([ORIG_HW], device='cuda'))[0]
    s = torch.sort(r0['scores'][r0['labels'] == 0], descending=True)[0]
    assert len(s) >= 8
    thr = float((s[5] + s[6]) / 2)
    cfg = dict(TRACKER_CFGS['reid_lsa'], detection_obj_score_thresh=thr, track_obj_score_thresh=thr,
               reid_score_thresh=thr, detection_nms_thresh=0.9, track_nms_thresh=0.9, masks=True)
    blobs = [{'img': f, 'orig_size': torch.tensor([ORIG_HW]), 'size': torch.tensor([NET_HW]),
              'dets': [torch.zeros(0, 4)]} for f in frames]
    yield model, post, cfg, blobs
    with torch.no_grad():
        for ce, b in zip(model.class_embed, biases):
            ce.bias.copy_(b)


def _run_multi(det, post, cfg, orders):
    """orders[s]: the blobs of slot s, frame by frame -> (results, per step the slots' tracks alive)."""
    from kinet_amd.tracker import MultiTracker
    tracker = MultiTracker(det, post, cfg, len(orders))
    alive = []
    for step in zip(*orders):
        tracker.step(list(step))
        alive.append(tuple(len(tracker.sequence(s).tracks) for s in range(len(orders))))
    return tracker.get_results(), alive


def _assert_same_results(a, b, min_rows=6):
    from fake_detector import flatten_results
    ia, va = flatten_results(a)
    ib, vb = flatten_results(b)
    assert torch.equal(ia, ib) and len(ia) >= min_rows
    np.testing.assert_allclose(va.numpy(), vb.numpy(), rtol=1e-5, atol=1e-3)
    owned = 0
    for f, t, _ in ia.tolist():
        ma, mb = a[t][f]['mask'], b[t][f]['mask']
        assert ma.dtype == np.bool_ and ma.shape == ORIG_HW and np.array_equal(ma, mb), (f, t)
        owned += int(ma.sum())
    assert owned > 0


def test_real_model_one_sequence_matches_tracker(real):
    from kinet_amd.tracker import Tracker
    model, post, cfg, blobs = real
    one = Tracker(model, post, cfg)
    one.reset()
    for blob in blobs:
        one.step(blob)
    res, alive = _run_multi(model, post, cfg, [blobs])
    assert 4 <= alive[0][0] <= 6
    _assert_same_results(res[0], one.get_results())
    assert not model.defer_masks


def test_real_model_two_equal_slots(real):
    model, post, cfg, blobs = real
    res, _ = _run_multi(model, post, cfg, [blobs, blobs])
    _assert_same_results(res[0], res[1])


def test_real_model_ragged_rows_against_the_full_head(real):
    model, post, cfg, blobs = real
    orders = [blobs, [blobs[i] for i in (2, 0, 3, 1)], [blobs[1]] * 4]       # the slots' K differ
    asked, switch = [], []
    genuine = model.mask_logits_rows

    def spy(rows, frames):
        asked.append(int(rows.numel()))
        switch.append(model.defer_masks)
        return genuine(rows, frames)
    model.mask_logits_rows = spy
    try:
        res_rows, alive = _run_multi(model, post, cfg, orders)
    finally:
        del model.mask_logits_rows
    assert not model.defer_masks                        # the tracker leaves the switch as it found it
    res_full, alive_full = _run_multi(_FullMasks(model), post, cfg, orders)
    assert alive == alive_full and sum(alive[0]) >= 8
    assert any(len(set(a)) > 1 for a in alive)          # the slots' track counts differ: ragged K
    total = [sum(a) for a in alive]
    assert len(asked) == sum(a > 0 for a in total)      # at most once per step
    assert all(n <= a for n, a in zip(asked, [a for a in total if a > 0])), (asked, alive)
    assert not any(switch)                              # restored before the head runs, as in Tracker
    for a, b in zip(res_rows, res_full):
        _assert_same_results(a, b, min_rows=4)
    print(f'multi tracker over the masks model: alive per step {alive}, rows asked {asked}')


# ---------------------------------------------------------------------------------- refusals
def test_refusals_that_remain():
    from fake_detector import TRACKER_CFGS
    from fake_mask_detector import mask_blobs
    from kinet_amd.models import DeformablePostProcess, PostProcessSegm
    from kinet_amd.tracker import MultiTracker
    det = M.BatchedFakeMaskDetector(0, [0]).cuda()
    cfg = TRACKER_CFGS['default']
    post = {'bbox': DeformablePostProcess(), 'segm': PostProcessSegm()}
    with pytest.raises(NotImplementedError):
        MultiTracker(det, {'bbox': post['bbox']}, dict(cfg, masks=True), 1)
    with pytest.raises(NotImplementedError):
        MultiTracker(det, post, cfg, 1)
    tracker = MultiTracker(det, post, dict(cfg, masks=True), 1)
    blob = mask_blobs(0, 1, device='cuda')[0]
    del blob['size']
    with pytest.raises(ValueError, match='size'):
        tracker.step([blob])
