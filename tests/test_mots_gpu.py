"""Segmentation masks inside kinet_amd.tracker.Tracker (tracker_cfg['masks']).

  * against the reference Tracker + PostProcessSegm on identical detector outputs (FakeMaskDetector;
    tests/golden/tracker_masks.npz from make_golden_mots.py): the box bookkeeping as in test_tracker_gpu.py,
    and every mask bit outside the fixture's ambiguous pixels (the reference's best probability within 5e-4
    of 0.5, its best two closer than 1e-5, or such a pixel carried into the next frame by a stale mask);
  * DETRSegmBase.mask_logits (defer_masks) against the rows of the full head, bit for bit;
  * the real masks model under the tracker, through mask_logits and through the full pred_masks.
"""
import os

import numpy as np
import pytest
import torch

import segm_refs as R

pytestmark = pytest.mark.gpu


def _unpack(bits, shape):
    return np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape).astype(bool)


@pytest.mark.parametrize('name', ['default', 'reid_lsa'])
@pytest.mark.parametrize('seq', [0, 1])
def test_tracker_masks_match_reference(golden_dir, name, seq):
    from fake_detector import TRACKER_CFGS, flatten_results
    from fake_mask_detector import ORIG_HW, FakeMaskDetector, mask_blobs
    from kinet_amd.models import DeformablePostProcess, PostProcessSegm
    from kinet_amd.tracker import Tracker
    d = np.load(os.path.join(golden_dir, 'tracker_masks.npz'))
    key, frames = f'{name}_{seq}', int(d['frames'])
    det = FakeMaskDetector(mask_seed=int(d['mask_seed']), seed=seq).cuda()
    tracker = Tracker(det, {'bbox': DeformablePostProcess(), 'segm': PostProcessSegm()},
                      dict(TRACKER_CFGS[name], masks=True))
    tracker.reset()
    for blob in mask_blobs(seq, frames, device='cuda'):
        tracker.step(blob)
    res = tracker.get_results()
    ids, vals = flatten_results(res)
    np.testing.assert_array_equal(ids.numpy(), d[f'{key}_ids'])
    np.testing.assert_allclose(vals.numpy(), d[f'{key}_vals'], rtol=1e-5, atol=1e-3)
    assert tracker.num_reids == int(d[f'{key}_reids'])
    assert tracker.track_num == int(d[f'{key}_tracks'])
    want = _unpack(d[f'{key}_masks'], (len(ids),) + ORIG_HW)
    amb = _unpack(d[f'{key}_amb'], (frames,) + ORIG_HW)
    assert amb.mean() <= 5e-3
    got = np.stack([res[t][f]['mask'] for f, t, _ in ids.tolist()])
    assert got.dtype == np.bool_ and got.shape == want.shape
    frame_of = ids[:, 0].numpy()
    clear = ~amb[frame_of]
    diff = (got != want) & clear
    print(f'tracker masks {key}: {int((got != want).sum())} differing bits, {int(diff.sum())} outside the '
          f'ambiguous pixels (share {amb.mean():.3e}); owned share {got.any(0).mean():.3f}')
    assert not diff.any()
    for f in range(frames):                     # at most one owner per pixel, everywhere
        assert got[frame_of == f].sum(0).max(initial=0) <= 1


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and torch.equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.fixture(scope='module')
def case_b(golden_dir):
    d = np.load(os.path.join(golden_dir, 'segm_b.npz'))
    model, post = R.build_case(golden_dir, 'b', int(d['seed']))
    model = model.cuda()
    model.tracking()
    return model, post


def test_deferred_mask_rows_bit_identical(case_b):
    from kinet_amd import _native as N
    model, _ = case_b
    frames = [f.cuda() for f in R.frames()]
    rows = torch.tensor([16, 3, 3, 0, 11], device='cuda')
    with torch.no_grad():
        out0 = model(frames)[0]
        targets = []
        for b in range(len(frames)):
            top = out0['pred_logits'][b].sigmoid().max(-1)[0].topk(R.N_TRACK).indices
            targets.append({'track_query_hs_embeds': out0['hs_embed'][b, top], 'track_query_boxes': out0['pred_boxes'][b, top]})
        for dtype in (torch.float32, torch.bfloat16):
            model.set_compute_dtype(dtype)
            try:
                full = model(frames, targets)[0]
                model.defer_masks = True
                out = model(frames, targets)[0]
                assert 'pred_masks' not in out
                assert _same({k: v for k, v in full.items() if k != 'pred_masks'}, out)
                assert full['pred_masks'].shape[1] == R.N_QUERIES + R.N_TRACK
                for b in range(len(frames)):
                    got = model.mask_logits(rows, b)
                    assert got.dtype == torch.float32 and got.shape == (5,) + R.FEATS[0]
                    assert torch.equal(got, full['pred_masks'][b, rows]), (dtype, b)
                N.trace_begin()
                empty = model.mask_logits(rows[:0], 1)
                assert N.trace_end() == [] and empty.shape == (0,) + R.FEATS[0]
                # a forward without defer_masks ends the context
                model.defer_masks = False
                again = model(frames, targets)[0]
                assert torch.equal(again['pred_masks'], full['pred_masks'])
                with pytest.raises(RuntimeError, match='defer_masks'):
                    model.mask_logits(rows, 0)
            finally:
                model.defer_masks = False
                model.set_compute_dtype(torch.float32)


class _FullMasks(torch.nn.Module):
    """The masks model as a detector that returns pred_masks itself (no mask_logits attribute)."""

    def __init__(self, model):
        super().__init__()
        self.model = model
        self.num_queries, self.overflow_boxes = model.num_queries, model.overflow_boxes

    def forward(self, img, targets=None, prev_features=None):
        return self.model(img, targets, prev_features)


def test_tracker_over_segm_model(case_b):
    model, post = case_b
    net_hw, orig_hw = (104, 200), (157, 301)
    g = torch.Generator().manual_seed(4201)
    frames = [torch.randn(1, 3, *net_hw, generator=g).cuda() for _ in range(4)]
    # the fixture's weights never rank class 0 (person) first: silence the other classes for this test, as
    # tools/track_hz.py does, and put the biases back afterwards (the model is shared)
    biases = [ce.bias.detach().clone() for ce in model.class_embed]
    with torch.no_grad():
        for ce in model.class_embed:
            ce.bias.fill_(-20.0)
            ce.bias[0] = 0.0
    try:
        _tracker_over_segm_model(model, post, frames, net_hw, orig_hw)
    finally:
        with torch.no_grad():
            for ce, b in zip(model.class_embed, biases):
                ce.bias.copy_(b)


def _tracker_over_segm_model(model, post, frames, net_hw, orig_hw):
    from fake_detector import TRACKER_CFGS, flatten_results
    from kinet_amd.tracker import Tracker
    with torch.no_grad():
        r0 = post['bbox'](model(frames[0])[0], torch.tensor([orig_hw], device='cuda'))[0]
    s = torch.sort(r0['scores'][r0['labels'] == 0], descending=True)[0]
    assert len(s) >= 8
    thr = float((s[5] + s[6]) / 2)                      # about six queries pass on the first frame
    cfg = dict(TRACKER_CFGS['reid_lsa'], detection_obj_score_thresh=thr, track_obj_score_thresh=thr,
               reid_score_thresh=thr, detection_nms_thresh=0.9, track_nms_thresh=0.9, masks=True)
    blobs = [{'img': f, 'orig_size': torch.tensor([orig_hw]), 'size': torch.tensor([net_hw]),
              'dets': [torch.zeros(0, 4)]} for f in frames]

    def run(det):
        tracker = Tracker(det, post, cfg)
        tracker.reset()
        alive = []
        for blob in blobs:
            tracker.step(blob)
            alive.append(len(tracker.tracks))
        return tracker.get_results(), alive

    asked = []
    real = model.mask_logits

    def spy(rows, frame=0):
        asked.append(int(rows.numel()))
        return real(rows, frame)
    model.mask_logits = spy
    try:
        res_rows, alive = run(model)
    finally:
        del model.mask_logits
    assert not model.defer_masks                        # the tracker leaves the switch as it found it
    res_full, alive_full = run(_FullMasks(model))
    assert alive == alive_full and 4 <= alive[0] <= 6 and len(asked) == sum(a > 0 for a in alive)
    assert all(n <= a for n, a in zip(asked, [a for a in alive if a > 0])), (asked, alive)
    ids_a, vals_a = flatten_results(res_rows)
    ids_b, vals_b = flatten_results(res_full)
    assert torch.equal(ids_a, ids_b) and torch.equal(vals_a, vals_b) and len(ids_a) >= 6
    owned = 0
    for f, t, _ in ids_a.tolist():
        ma, mb = res_rows[t][f]['mask'], res_full[t][f]['mask']
        assert ma.dtype == np.bool_ and ma.shape == orig_hw and np.array_equal(ma, mb)
        owned += int(ma.sum())
    print(f'tracker over the masks model: alive per frame {alive}, rows asked {asked}, owned pixels {owned}')
    assert owned > 0
