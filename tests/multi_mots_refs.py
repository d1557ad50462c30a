"""Shared by the multi-sequence MOTS tests (test infrastructure): the batched stand-in detector of
multi_track_refs with segmentation masks, and the runs / assertions of the tracker-masks fixture."""
import os

import numpy as np
import torch

from multi_track_refs import BatchedFakeDetector


class BatchedFakeMaskDetector(BatchedFakeDetector):
    """One fake_mask_detector.FakeMaskDetector(mask_seed, seed=s) per sequence behind the batched, ragged
    interface of BatchedFakeDetector: pred_masks (S, Kmax + Q, 24, 34) rides along, and its placeholder rows
    are NaN like those of the logits, boxes and embeddings."""

    def __init__(self, mask_seed, seeds, **kw):
        torch.nn.Module.__init__(self)
        from fake_mask_detector import FakeMaskDetector
        self.fakes = torch.nn.ModuleList([FakeMaskDetector(mask_seed=mask_seed, seed=s, **kw) for s in seeds])
        self.live = list(range(len(seeds)))
        self.num_queries = self.fakes[0].num_queries
        self.overflow_boxes = self.fakes[0].overflow_boxes
        self.calls = []

    def forward(self, samples, targets=None, prev_features=None):
        assert samples.tensors.shape[0] == len(self.live)
        outs, ks = [], []
        Q = self.num_queries
        kmax = 0 if targets is None else targets[0]['track_query_boxes'].shape[0]
        for j, s in enumerate(self.live):
            k = 0
            if targets is not None:
                m = targets[j]['track_queries_placeholder_mask']
                assert m.shape == (kmax + Q,) and m.dtype == torch.bool and not m[kmax:].any()
                k = kmax - int(m[:kmax].sum())
                assert not m[:k].any() and m[k:kmax].all()
            t = None
            if k:
                t = [{'track_query_boxes': targets[j]['track_query_boxes'][:k],
                      'track_query_hs_embeds': targets[j]['track_query_hs_embeds'][:k]}]
            out = self.fakes[s](None, t, None)[0]
            pad = {}
            for name, v in out.items():
                nan = torch.full((1, kmax - k) + tuple(v.shape[2:]), float('nan'), dtype=v.dtype, device=v.device)
                pad[name] = torch.cat([v[:, :k], nan, v[:, k:]], 1)
            outs.append(pad)
            ks.append(k)
        self.calls.append(ks)
        out = {name: torch.cat([o[name] for o in outs]) for name in outs[0]}
        return out, None, ['features of the batch'], None, None


def multi(name, mask_seed, seeds, **kw):
    from fake_detector import TRACKER_CFGS
    from kinet_amd.models import DeformablePostProcess, PostProcessSegm
    from kinet_amd.tracker import MultiTracker
    det = BatchedFakeMaskDetector(mask_seed, seeds).cuda()
    post = {'bbox': DeformablePostProcess(), 'segm': PostProcessSegm()}
    return MultiTracker(det, post, dict(TRACKER_CFGS[name], masks=True), len(seeds), **kw), det


def run_multi(tracker, det, seeds, frames, retire_at=None):
    """multi_track_refs.run_multi on mask_blobs: -> the transfers of every step."""
    from fake_mask_detector import mask_blobs
    blobs = [mask_blobs(s, frames, device='cuda') for s in seeds]
    live = list(range(len(seeds)))
    counts = []
    for f in range(frames):
        if retire_at is not None and f == retire_at[1]:
            tracker.retire(retire_at[0])
            det.retire(retire_at[0])
            live.remove(retire_at[0])
        before = tracker.sync_count
        tracker.step([blobs[i][f] for i in live])
        counts.append(tracker.sync_count - before)
    return counts


def run_single(name, mask_seed, seq, frames):
    """kinet_amd.tracker.Tracker with masks on the plain FakeMaskDetector: -> its results."""
    from fake_detector import TRACKER_CFGS
    from fake_mask_detector import FakeMaskDetector, mask_blobs
    from kinet_amd.models import DeformablePostProcess, PostProcessSegm
    from kinet_amd.tracker import Tracker
    det = FakeMaskDetector(mask_seed=mask_seed, seed=seq).cuda()
    tracker = Tracker(det, {'bbox': DeformablePostProcess(), 'segm': PostProcessSegm()},
                      dict(TRACKER_CFGS[name], masks=True))
    tracker.reset()
    for blob in mask_blobs(seq, frames, device='cuda'):
        tracker.step(blob)
    return tracker.get_results()


def unpack(bits, shape):
    return np.unpackbits(bits)[:int(np.prod(shape))].reshape(shape).astype(bool)


def assert_fixture(d, name, seq, results, q=None, frames=None):
    """The assertions of test_mots_gpu.test_tracker_masks_match_reference on one sequence's results
    (frames: only the fixture's frames below it, for a retired sequence) -> the stacked masks."""
    from fake_detector import flatten_results
    from fake_mask_detector import ORIG_HW
    key, n_frames = f'{name}_{seq}', int(d['frames'])
    ids, vals = flatten_results(results)
    want_ids, want_vals = d[f'{key}_ids'], d[f'{key}_vals']
    want = unpack(d[f'{key}_masks'], (len(want_ids),) + ORIG_HW)
    amb = unpack(d[f'{key}_amb'], (n_frames,) + ORIG_HW)
    if frames is not None:
        sel = want_ids[:, 0] < frames
        want_ids, want_vals, want = want_ids[sel], want_vals[sel], want[sel]
    np.testing.assert_array_equal(ids.numpy(), want_ids)
    np.testing.assert_allclose(vals.numpy(), want_vals, rtol=1e-5, atol=1e-3)
    if q is not None:
        assert q.num_reids == int(d[f'{key}_reids'])
        assert q.track_num == int(d[f'{key}_tracks'])
    assert amb.mean() <= 5e-3
    got = np.stack([results[t][f]['mask'] for f, t, _ in ids.tolist()])
    assert got.dtype == np.bool_ and got.shape == want.shape
    frame_of = ids[:, 0].numpy()
    diff = (got != want) & ~amb[frame_of]
    print(f'multi tracker masks {key}: {int((got != want).sum())} differing bits, {int(diff.sum())} outside the '
          f'ambiguous pixels (share {amb.mean():.3e}); owned share {got.any(0).mean():.3f}')
    assert not diff.any()
    for f in range(n_frames if frames is None else frames):     # at most one owner per pixel, everywhere
        assert got[frame_of == f].sum(0).max(initial=0) <= 1
    return ids, got


def load_fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'tracker_masks.npz'))
