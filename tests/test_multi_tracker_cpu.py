"""Host side of the multi-sequence tracker: the track-query planner, the restatements the GPU tests compare
against (checked here against DeformablePostProcess + clip_boxes_to_image on the CPU), and the C header
against the ctypes bindings."""
import os
import re

import numpy as np
import pytest
import torch

import multi_track_refs as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('n_active,n_inactive,kmax,offsets', [
    ((0, 0), (0, 0), 0, [0, 0, 0]),
    ((0, 3), (0, 2), 5, [0, 0, 5]),
    ((4, 1), (0, 3), 4, [0, 4, 8]),
    ((2,), (1,), 3, [0, 3]),
])
def test_plan_track_queries(n_active, n_inactive, kmax, offsets):
    from kinet_amd.tracker import plan_track_queries
    Q = 6
    plan = plan_track_queries(n_active, n_inactive, Q)
    k = [a + b for a, b in zip(n_active, n_inactive)]
    assert plan['Kmax'] == kmax and plan['K'].tolist() == k and plan['K'].dtype == np.int32
    assert plan['offsets'].tolist() == offsets and plan['offsets'].dtype == np.int32
    assert plan['mask'].shape == (len(k), kmax + Q) and plan['mask'].dtype == bool
    for s, ks in enumerate(k):
        assert plan['mask'][s].tolist() == [False] * ks + [True] * (kmax - ks) + [False] * Q


def test_plan_refuses_more_rows_than_the_kernels_take():
    from kinet_amd.tracker import plan_track_queries
    plan_track_queries((3596,), (0,), 500)
    with pytest.raises(ValueError):
        plan_track_queries((3000, 10), (597, 0), 500)
    with pytest.raises(ValueError):
        plan_track_queries((), (), 500)


@pytest.mark.parametrize('clip', [True, False])
def test_decide_restatement_is_the_trackers_composition(clip):
    """decide_ref == DeformablePostProcess + clip_boxes_to_image + Tracker.step's compares, sample by sample."""
    from kinet_amd.models import DeformablePostProcess
    from kinet_amd.tracker import clip_boxes_to_image
    g = torch.Generator().manual_seed(0)
    S, kmax, Q, C = 3, 4, 6, 5
    k = [4, 0, 2]
    logits = torch.randn(S, kmax + Q, C, generator=g) * 1.5
    boxes = torch.cat([torch.rand(S, kmax + Q, 2, generator=g) * 1.2 - 0.1, torch.rand(S, kmax + Q, 2, generator=g) * 0.5], -1)
    sizes = torch.tensor([[480, 640], [375, 1242], [1080, 1920]])
    th = (0.4, 0.6, 0.5)
    got = R.decide_ref(logits, boxes, sizes.float(), k, kmax, *th, clip)
    for s in range(S):
        res = DeformablePostProcess()({'pred_logits': logits[s:s + 1], 'pred_boxes': boxes[s:s + 1]}, sizes[s:s + 1])[0]
        b = clip_boxes_to_image(res['boxes'], sizes[s]) if clip else res['boxes']
        sc, lb = res['scores'], res['labels']
        dec = torch.stack([sc > th[0], sc > th[1], sc > th[2], lb == 0])
        byte = (dec[0] * 1 + dec[1] * 2 + dec[2] * 4 + dec[3] * 8).to(torch.uint8)
        real = [r for r in range(kmax + Q) if not k[s] <= r < kmax]
        assert torch.equal(got[0][s, real], b[real])
        assert torch.equal(got[1][s, real], sc[real])
        assert torch.equal(got[2][s, real].long(), lb[real])
        assert torch.equal(got[3][s, real], byte[real])
        for t in got:
            assert not t[s, k[s]:kmax].any()


def test_nms_restatement_keeps_existing_tracks():
    boxes = torch.tensor([[0., 0, 10, 10], [1, 1, 11, 11], [50, 50, 60, 60], [0, 0, 10, 10]])
    scores = torch.tensor([0.5, 0.9, 0.1, 0.5])
    idx = torch.tensor([3, 1, 0, 2], dtype=torch.int32)
    off = torch.tensor([0, 4], dtype=torch.int32)
    assert R.nms_segments_ref(boxes, scores, idx, off, 0.5).tolist() == [0, 1, 0, 1]
    flag = torch.tensor([1, 0, 0, 0], dtype=torch.uint8)       # entry 0 (row 3) is an existing track: it wins
    assert R.nms_segments_ref(boxes, scores, idx, off, 0.5, flag).tolist() == [1, 0, 0, 1]
    assert R.nms_segments_ref(boxes, scores, idx[:0], torch.tensor([0, 0]), 0.5).tolist() == []


def test_gather_and_commit_restatements():
    d = 3
    bank = torch.zeros(4, d + 5)
    hs = torch.arange(6.).view(2, 3)
    R.commit_ref(bank, hs, torch.tensor([[10., 20, 30, 60], [0, 0, 8, 4]]), torch.tensor([0.7, 0.2]),
                 torch.tensor([1, 0], dtype=torch.int32), torch.tensor([2, 3], dtype=torch.int32))
    assert bank[2, :d + 4].tolist() == [3, 4, 5, 0, 0, 8, 4] and bank[2, d + 4].item() == np.float32(0.2)
    assert not bank[:2].any()
    emb, box, mask = R.gather_ref(bank, torch.tensor([3], dtype=torch.int32), torch.tensor([0, 0, 1]),
                                  torch.tensor([[100., 200.], [100., 200.]]), 1, 2)
    assert emb[1, 0].tolist() == [0, 1, 2] and emb[0, 0].tolist() == [0, 0, 0]
    assert box[0, 0].tolist() == [0.5] * 4
    np.testing.assert_allclose(box[1, 0].numpy(), [20 / 200, 40 / 100, 20 / 200, 40 / 100], rtol=1e-6)
    assert mask.tolist() == [[True, False, False], [False, False, False]]


def test_shared_helpers_are_the_trackers():
    """Tracker and MultiTracker call the same gating / matching helpers (none is copied)."""
    import inspect
    from kinet_amd import tracker as T
    for name in ('public_detections_mask', 'reid_match_greedy', 'reid_match_lsa', 'deferred_masks', 'copy_with_sizes',
                 'plan_mask_resolve', 'self._score_phase', 'self._drop_suppressed', 'self._assign_reid',
                 'self._count_new_tracks', 'self._end_frame', 'self._read_cfg'):
        assert name + '(' in inspect.getsource(T.Tracker), name
        assert name + '(' in inspect.getsource(T.MultiTracker), name
    # the per-frame rules themselves are written once, in the class both inherit
    for cls in (T.Tracker, T.TrackerKinematic, T.MultiTracker):
        assert issubclass(cls, T._TrackRules)
        for name in ('_score_phase', '_drop_suppressed', '_assign_reid', '_count_new_tracks', '_end_frame', '_read_cfg'):
            assert getattr(cls, name) is getattr(T._TrackRules, name), (cls, name)


def test_header_declares_what_the_bindings_bind():
    from kinet_amd import _native
    src = open(os.path.join(REPO, 'include', 'kinet_track.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    declared = set(re.findall(r'\b(kinet_[a-z0-9_]+)\s*\(', src))
    bound = {n for n in _native._SIGS if n.startswith('kinet_track_') or n == 'kinet_nms_segments'}
    assert declared == bound and len(bound) == 5
    lib = _native.lib()
    for n in bound:
        assert hasattr(lib, n), n
    # argument counts of the declarations and the ctypes signatures agree
    for n in bound:
        args = re.search(r'\b' + n + r'\s*\(([^)]*)\)', src, flags=re.S).group(1)
        assert len(args.split(',')) == len(_native._SIGS[n]), n


def test_kernels_reject_bad_arguments_before_touching_the_device():
    """include/kinet_track.h: KINET_ERR_ARG and a message (null pointers would fault otherwise)."""
    from kinet_amd import _native as N
    lib = N.lib()
    assert lib.kinet_track_decide(None, None, None, None, None, None, 1, 4097, 1, 0, 0.4, 0.4, 0.4, 1, None) == 1
    assert b'4096' in lib.kinet_last_error()
    assert lib.kinet_track_decide(None, None, None, None, None, None, 1, 10, 1, 11, 0.4, 0.4, 0.4, 1, None) == 1
    assert lib.kinet_track_gather(None, 4, 16, None, None, None, None, None, None, 1, 4000, 500, None) == 1
    assert b'4096' in lib.kinet_last_error()
    assert lib.kinet_track_gather(None, 4, 16, None, None, None, None, None, None, 1, 0, 500, None) == 1
    assert lib.kinet_nms_segments(None, 3, None, 1, 4, None, None, None, None, 1, 1, 0.5, None) == 1
    assert lib.kinet_track_commit(None, None, None, 4, None, None, -1, None, 4, 16, None) == 1
    assert lib.kinet_track_reid_dist(None, 4, None, 4, 0, None, None, None, None, None, None, 1, 1, None) == 1
    # empty work returns before any pointer is read
    assert lib.kinet_nms_segments(None, 4, None, 1, 0, None, None, None, None, 0, 0, 0.5, None) == 0
    assert lib.kinet_track_commit(None, None, None, 0, None, None, 0, None, 0, 16, None) == 0
