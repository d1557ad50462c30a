#!/usr/bin/env python
"""Generate tests/golden/tracker_masks.npz: the reference Tracker (tracker.py:18-562) with the
reference PostProcessSegm (detr_segmentation.py:219-253) on the CPU over FakeMaskDetector outputs
(fake_mask_detector.py), with the import harness of make_golden.py:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mots.py | tee profiles/mots_fixture.log

cfgs `default` and `reid_lsa` of fake_detector.TRACKER_CFGS x 2 sequences of FRAMES frames, original
size 120x176, network-input size 96x136.  Per run `{cfg}_{seq}_*`:
  ids, vals, reids, tracks   as tracker.npz (flatten_results order)
  masks                      results[track][frame]['mask'] (bool 120x176) of every row of ids, bit-packed
  amb                        per frame, the AMBIGUOUS pixels bit-packed: the reference's best probability
                             lies within BAND = 5e-4 of 0.5, or its best two are closer than GAP = 1e-5
                             while the best is above 0.5 - BAND.  (This project's bound on a probability is
                             2e-6, so a swap of owners needs a gap of at most 4e-6.)
plus `mask_seed`, the FakeMaskDetector noise seed taken.

What the reference really stacks (tracker.py:516): a track that stays active without being
re-detected (steps_termination = 2) still carries LAST frame's resolved bool mask, which torch.stack
promotes to 1.0 / 0.0 among the fresh probabilities.  The stacked tensor is read through a stand-in for
the `torch` name inside the reference's tracker module that records the result of its one stack of
2-d tensors; nothing of the reference is copied.

The generator asserts, and searches mask seeds from fake_mask_detector.MASK_SEED otherwise:
  * the ambiguous share per sequence is <= 0.5 %;
  * (counted inside that share) a pixel that was ambiguous in the frame before, with a track among its
    possible owners that is stale in this frame, is ambiguous in this frame too: the stale slot IS the
    earlier resolution, so a differently resolved pixel travels with it (`carried` in the log);
  * over the four runs there is at least one pixel contested by >= 2 tracks above 0.5, one stale mask
    resolved together with an overlapping fresh one, one reid() match carrying a mask, and one track
    query returning from inactive.
"""
import numpy as np
import torch

from make_golden import _install_stubs, save

FRAMES = 14
CFGS = ('default', 'reid_lsa')
SEQS = (0, 1)
BAND = 5e-4
GAP = 1e-5
MAX_AMBIGUOUS = 5e-3


class _TorchSpy:
    """Stands in for `torch` inside the reference tracker module: everything is torch's, and stack
    records the operands and the result when it stacks (oh, ow) maps."""

    def __init__(self):
        self.stacked = None

    def __getattr__(self, name):
        return getattr(torch, name)

    def stack(self, tensors, *a, **kw):
        out = torch.stack(tensors, *a, **kw)
        if len(tensors) and tensors[0].dim() == 2:
            assert self.stacked is None, 'one stack of masks per frame'
            self.stacked = ([t.dtype == torch.bool for t in tensors], out)
        return out


def run(cfg_name, seq, mask_seed, spy):
    """One sequence through the reference tracker -> (arrays, events, ambiguous share) or a rejection."""
    from trackformer.models.deformable_detr import DeformablePostProcess
    from trackformer.models.detr_segmentation import PostProcessSegm
    from trackformer.models.tracker import Tracker
    from fake_detector import TRACKER_CFGS, flatten_results
    from fake_mask_detector import ORIG_HW, FakeMaskDetector, mask_blobs

    det = FakeMaskDetector(mask_seed=mask_seed, seed=seq)
    tracker = Tracker(det, {'bbox': DeformablePostProcess(), 'segm': PostProcessSegm()}, TRACKER_CFGS[cfg_name], False)
    tracker.reset()
    reid_matches = []
    ref_reid = tracker.reid

    def reid(*a, **kw):
        keep = ref_reid(*a, **kw)
        reid_matches.append(int((~keep).sum()))
        return keep
    tracker.reid = reid

    ev = dict(contested=0, stale_overlap=0, reid_match=0, query_return=0)
    amb, prev_cand, prev_tracks = [], None, []
    for blob in mask_blobs(seq, FRAMES):
        spy.stacked = None
        reids0, n_match0 = tracker.num_reids, sum(reid_matches)
        with torch.no_grad():
            tracker.step(blob)
        matched = sum(reid_matches) - n_match0
        ev['reid_match'] += matched
        ev['query_return'] += tracker.num_reids - reids0 - matched
        a = torch.zeros(ORIG_HW, dtype=torch.bool)
        if spy.stacked is not None:
            stale, probs = spy.stacked
            assert probs.dtype == torch.float32 and tuple(probs.shape[1:]) == ORIG_HW, (probs.dtype, probs.shape)
            assert len(stale) == len(tracker.tracks)
            top = probs.topk(min(2, probs.shape[0]), dim=0)[0]
            best = top[0]
            a = (best - 0.5).abs() <= BAND
            if probs.shape[0] > 1:
                a |= ((best - top[1]) < GAP) & (best > 0.5 - BAND)
            ev['contested'] += int(((probs > 0.5).sum(0) >= 2).sum())
            # tracks that may own an ambiguous pixel in an implementation within the bounds
            cand = a[None] & (probs >= best[None] - GAP) & (best[None] > 0.5 - BAND)
            if any(stale):
                st = torch.tensor(stale)
                ev['stale_overlap'] += int(((probs[st] > 0.5).any(0) & (probs[~st] > 0.5).any(0)).sum()) if (~st).any() else 0
                # carry: a stale slot is last frame's RESOLVED mask, so a pixel that this track might or
                # might not have owned there is uncertain here as well, whatever the probabilities say
                carry = torch.zeros_like(a)
                for i in [i for i, s_ in enumerate(stale) if s_]:
                    carry |= prev_cand[[t is tracker.tracks[i] for t in prev_tracks].index(True)]
                carry &= ~a
                ev['carried'] = ev.get('carried', 0) + int(carry.sum())
                a = a | carry
                cand = cand | carry[None]          # (whoever it goes to: every slot is a candidate)
            prev_cand, prev_tracks = cand, list(tracker.tracks)
            # the reference's own result must be what the label-map reading of it says
            owner = probs.argmax(0)
            for i, t in enumerate(tracker.tracks):
                assert torch.equal(t.mask, (owner == i) & (probs[i] > 0.5))
        else:
            prev_cand, prev_tracks = None, []
        amb.append(a)
    share = float(torch.stack(amb).float().mean())
    if share > MAX_AMBIGUOUS:
        return None, f'ambiguous share {share:.3e}', None
    results = tracker.get_results()
    ids, vals = flatten_results(results)
    masks = np.stack([results[int(t)][int(f)]['mask'] for f, t, _ in ids.tolist()])
    assert masks.dtype == np.bool_ and masks.shape[1:] == ORIG_HW
    assert (masks.reshape(len(ids), -1).any(1)).mean() > 0.5, 'most tracks own pixels'
    arr = {'ids': ids, 'vals': vals, 'reids': torch.tensor(tracker.num_reids), 'tracks': torch.tensor(tracker.track_num),
           'masks': np.packbits(masks.reshape(-1)), 'amb': np.packbits(torch.stack(amb).numpy().reshape(-1)),
           'amb_share': np.array(share), 'owned_share': np.array(masks.any(0).mean() if len(masks) else 0.0)}
    return arr, ev, share


def main():
    _install_stubs()
    torch.set_num_threads(8)
    from trackformer.models import tracker as ref_tracker
    from fake_mask_detector import MASK_SEED

    # reference defect, patched exactly as make_golden.gen_tracker does: Track.reset_last_pos also
    # empties last_pos_relative, so a re-identified track that later goes inactive raises IndexError
    def _reset_last_pos(self):
        self.last_pos.clear()
        self.last_pos.append(self.pos.clone())
    ref_tracker.Track.reset_last_pos = _reset_last_pos

    # reference defect: add_tracks (tracker.py:100-108) passes the new track's mask and attention map
    # positionally, where Track.__init__ (:1059-1060) takes pos_rel first -- the mask lands in pos_rel,
    # track.mask stays None and the frame's torch.stack (:516) raises TypeError at the first new
    # track.  The harness hands them to the arguments add_tracks means.
    class Track(ref_tracker.Track):
        def __init__(self, pos, score, track_id, hs_embed, obj_ind, mask=None, attention_map=None):
            super().__init__(pos, score, track_id, hs_embed, obj_ind, mask=mask, attention_map=attention_map)
    ref_tracker.Track = Track
    spy = _TorchSpy()
    ref_tracker.torch = spy

    for mask_seed in range(MASK_SEED, MASK_SEED + 20):
        arr, total, why = {'mask_seed': np.array(mask_seed), 'frames': np.array(FRAMES)}, {}, None
        for cfg in CFGS:
            for seq in SEQS:
                a, ev, share = run(cfg, seq, mask_seed, spy)
                if a is None:
                    why = f'{cfg} seq {seq}: {ev}'
                    break
                print(f'mask seed {mask_seed} {cfg} seq {seq}: rows {len(a["ids"])} tracks {int(a["tracks"])} '
                      f'reids {int(a["reids"])} ambiguous share {share:.3e} owned share {float(a["owned_share"]):.3f} '
                      f'events {ev}')
                for k, v in ev.items():
                    total[k] = total.get(k, 0) + v
                arr.update({f'{cfg}_{seq}_{k}': v for k, v in a.items()})
            if why:
                break
        if why is None and not all(v for k, v in total.items() if k != 'carried'):
            why = f'missing events {total}'
        if why is None:
            print(f'mask seed {mask_seed} taken: events over the set {total}')
            break
        print(f'mask seed {mask_seed} REJECTED: {why}')
    else:
        raise RuntimeError('no mask seed met the fixture conditions')
    save('tracker_masks.npz', **arr)


if __name__ == '__main__':
    main()
