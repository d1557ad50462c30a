"""Online multi-object tracker over the kinet_amd detector: the reference's
`Tracker` (src/trackformer/models/tracker.py:18-562, `Track` :1056-1130) with the same
constructor, `reset()`, `step(blob)` and `get_results()`, so src/track.py drives it unchanged
(track.py:127-214: one `step` per frame, results {track_id: {frame: {'bbox', 'score',
'obj_ind'}}}).

Per frame (tracker.py:269-557): the active + inactive tracks become track queries (their
last box, cxcywh normalised by the image size, and their last decoder embedding); one
detector forward with the previous frame's features; post-process; track keep / terminate /
re-identify by score; track NMS; new detections above threshold (optionally gated by public
detections) are re-identified against inactive tracks (embedding-distance LSA) or start new
tracks; detection NMS; results.  Thresholds come from the reference's `tracker_cfg`
(cfgs/track.yaml:28-49).

MI355X-side choices: the detector, post-process, clipping, thresholding and NMS
(kernels.nms, a one-workgroup HIP kernel with torchvision.ops.nms semantics) run on the GPU;
the track bookkeeping is host Python as in the reference, fed by ONE batched device->host
copy of the small per-frame decision arrays instead of a sync per track.  Attention maps are
not built (generate_attention_maps asserts in the reference for Deformable DETR,
tracker.py:38-40).

Segmentation masks (tracker_cfg['masks'], MOTS; tracker.py:316-327, :339-379, :425-486, :515-545):
the reference post-processes every query's mask to the original size and keeps those of the
tracks alive at the end of the frame.  Here each track records the ROW of the frame's output its
mask comes from; after the last NMS the mask head runs on those rows only
(DETRSegmBase.mask_logits) and kinet_segm_track_resolve writes one int16 label map (the slot of
the owning track per pixel, -1 background), which rides in the end-of-frame results copy.  A
track that stays active without being re-detected (steps_termination > 1) keeps last frame's
RESOLVED mask in the reference, which torch.stack promotes to 1.0 / 0.0 among the fresh
probabilities: its slot is "stale" and names its slot in the previous label map (two maps,
ping-pong).  results[id][frame]['mask'] is a numpy bool (oh, ow), as in the reference.
"""
import contextlib
import functools
import math
import time
from collections import deque

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from kinet_amd import kernels as K
from kinet_amd.models.misc import box_xyxy_to_cxcywh


def clip_boxes_to_image(boxes, size):
    """torchvision.ops.clip_boxes_to_image: x to [0, w], y to [0, h]; size = (h, w)."""
    h, w = size[0], size[1]
    x = boxes[..., 0::2].clamp(min=0, max=w)
    y = boxes[..., 1::2].clamp(min=0, max=h)
    return torch.stack([x[..., 0], y[..., 0], x[..., 1], y[..., 1]], -1)


def box_iou(boxes1, boxes2):
    """IoU matrix of xyxy boxes (torchvision.ops.box_iou)."""
    a1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    a2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    lt = torch.max(boxes1[:, None, :2], boxes2[:, :2])
    rb = torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (a1[:, None] + a2 - inter)


def public_detections_mask(mode, new_det_boxes, public_det_boxes, iou_device=None):
    """tracker.py:127-170 as a host mask: which of the new detections (xyxy) a public detection
    claims.  `mode` is tracker_cfg['public_detections']; the IoU matrix of 'min_iou_0_5' is taken on
    `iou_device` (None: where new_det_boxes lives).  Shared by Tracker and MultiTracker."""
    n = new_det_boxes.size(0)
    if not mode:
        return torch.ones(n, dtype=torch.bool)
    if not len(public_det_boxes) or not n:
        return torch.zeros(n, dtype=torch.bool)
    mask = torch.zeros(n, dtype=torch.bool)
    if mode == 'center_distance':
        nb = new_det_boxes.cpu()
        item_size = ((nb[:, 2] - nb[:, 0]) * (nb[:, 3] - nb[:, 1])).numpy().astype(np.float32)
        a = box_xyxy_to_cxcywh(nb).numpy()[:, :2]
        b = box_xyxy_to_cxcywh(public_det_boxes.cpu()).numpy()[:, :2]
        dist3 = ((a.reshape(-1, 1, 2) - b.reshape(1, -1, 2)) ** 2).sum(axis=2)
        for j in range(len(public_det_boxes)):
            i = dist3[:, j].argmin()
            if dist3[i, j] < item_size[i]:
                dist3[i, :] = 1e18
                mask[i] = True
    elif mode == 'min_iou_0_5':
        dev = new_det_boxes.device if iou_device is None else iou_device
        iou = box_iou(new_det_boxes.to(dev), public_det_boxes.to(dev)).cpu()
        for j in range(len(public_det_boxes)):
            i = iou[:, j].argmax()
            if iou[i, j] >= 0.5:
                iou[i, :] = 0
                mask[i] = True
    else:
        raise NotImplementedError(mode)
    return mask


def reid_match_greedy(nb, ib):
    """tracker.py:190-233: greedy centre-distance matching of inactive tracks (ib, (a, 4) cxcywh numpy)
    with new detections (nb, (b, 4) cxcywh numpy) -> (dist_mat, rows, cols).  Shared by Tracker and
    MultiTracker."""
    dist_mat = ((ib[:, :2].reshape(-1, 1, 2) - nb[:, :2].reshape(1, -1, 2)) ** 2).sum(axis=2)
    track_size = ib[:, 2] * ib[:, 3]
    item_size = nb[:, 2] * nb[:, 3]
    invalid = (dist_mat > track_size.reshape(-1, 1)) + (dist_mat > item_size.reshape(1, -1))
    dist_mat = dist_mat + invalid * 1e18
    matched = []
    for i in range(dist_mat.shape[0]):
        j = dist_mat[i].argmin()
        if dist_mat[i][j] < 1e16:
            dist_mat[:, j] = 1e18
            dist_mat[i, j] = 0.0
            matched.append([i, j])
    matched = np.array(matched, np.int32).reshape(-1, 2)
    return dist_mat, matched[:, 0], matched[:, 1]


def reid_match_lsa(dist_mat):
    """tracker.py:236-246: the linear-sum assignment of an (inactive track, detection) embedding
    distance matrix -> (rows, cols).  Shared by Tracker and MultiTracker."""
    return linear_sum_assignment(dist_mat)


@contextlib.contextmanager
def deferred_masks(detector, on):
    """Run the detector with `defer_masks` set (the mask head then runs after the bookkeeping, on the
    surviving tracks' rows only) and restore the switch; nothing is touched when `on` is false."""
    if not on:
        yield
        return
    was_deferred, detector.defer_masks = detector.defer_masks, True
    try:
        yield
    finally:
        detector.defer_masks = was_deferred


def copy_with_sizes(payload, size_tensors, to_host):
    """A frame's decisions (`payload`, a flat uint8 device tensor) and its frame sizes (tensors whose first
    two elements are (h, w)) through ONE `to_host(tensor) -> numpy` transfer: sizes that live on the device
    ride behind the payload as int32 bytes, host sizes are read where they are -> (the payload's host copy,
    (len(size_tensors), 2) int32 sizes)."""
    size_t = [t.reshape(-1)[:2] for t in size_tensors]
    if any(t.is_cuda for t in size_t):
        extra = torch.cat([t.to(payload.device, torch.int32) for t in size_t]).view(torch.uint8)
        host = to_host(torch.cat([payload, extra]))
        return host[:payload.numel()], np.frombuffer(host[payload.numel():].tobytes(), np.int32).reshape(-1, 2)
    return to_host(payload), np.asarray([[int(v) for v in t.tolist()] for t in size_t], np.int32).reshape(-1, 2)


class _TrackRules:
    """The reference's per-frame track rules, each once, for Tracker, TrackerKinematic and MultiTracker.
    The tracker (`self`) holds the thresholds and the logger; `state` is the object with one sequence's
    `tracks`, `inactive_tracks`, `track_num`, `num_reids`, `frame_index` and `results`: the tracker itself
    for the single-sequence classes, the _Sequence for MultiTracker.  Where the trackers differ (what a
    track takes from a row, how tracks go inactive, what a removed track releases) the caller passes the
    action in."""

    def _read_cfg(self, tracker_cfg, generate_attention_maps):
        """The thresholds of cfgs/track.yaml:28-49; attention maps are refused."""
        if generate_attention_maps:
            raise NotImplementedError('attention maps (tracker.py:38-40) need the decoder\'s attention '
                                      'probabilities, which the fused attention kernels do not export')
        self.detection_obj_score_thresh = tracker_cfg['detection_obj_score_thresh']
        self.track_obj_score_thresh = tracker_cfg['track_obj_score_thresh']
        self.detection_nms_thresh = tracker_cfg['detection_nms_thresh']
        self.track_nms_thresh = tracker_cfg['track_nms_thresh']
        self.public_detections = tracker_cfg['public_detections']
        self.inactive_patience = float(tracker_cfg['inactive_patience'])
        self.reid_sim_threshold = tracker_cfg['reid_sim_threshold']
        self.reid_sim_only = tracker_cfg['reid_sim_only']
        self.reid_score_thresh = tracker_cfg['reid_score_thresh']
        self.reid_greedy_matching = tracker_cfg['reid_greedy_matching']
        self.prev_frame_dist = tracker_cfg['prev_frame_dist']
        self.steps_termination = tracker_cfg['steps_termination']

    def _score_phase(self, state, track_keep, reid_keep, take, go_inactive):
        """tracker.py:351-432: an active track whose row i passes `track_keep` takes it (`take(i, track)`),
        one that fails steps_termination times in a row goes inactive (`go_inactive(tracks)`); an inactive
        track whose row passes `reid_keep` takes it and is active again (a re-identification by score)."""
        to_inactive, from_inactive = [], []
        for i, track in enumerate(state.tracks):
            if track_keep[i]:
                take(i, track)
                track.count_termination = 0
            else:
                track.count_termination += 1
                if track.count_termination >= self.steps_termination:
                    to_inactive.append(track)
        for i, track in enumerate(state.inactive_tracks, start=len(state.tracks)):
            if reid_keep[i]:
                take(i, track)
                from_inactive.append(track)
        if to_inactive:
            self._logger(f'NEW INACTIVE TRACK IDS (track_obj_score_thresh={self.track_obj_score_thresh}): '
                         f'{[t.id for t in to_inactive]}')
        state.num_reids += len(from_inactive)
        for track in from_inactive:
            state.inactive_tracks.remove(track)
            state.tracks.append(track)
        go_inactive(to_inactive)

    def _drop_suppressed(self, state, keep, what, release=None):
        """tracker.py:437-447 / :511-527: drop the tracks NMS suppressed; keep[i] tells whether
        state.tracks[i] survived, `what` names the threshold, `release(track)` frees what a dropped track
        held."""
        remove = [t for t, k in zip(state.tracks, keep) if not k]
        if remove:
            self._logger(f'REMOVE TRACK IDS ({what}={getattr(self, what)}): {[t.id for t in remove]}')
            if release is not None:
                for t in remove:
                    release(t)
            state.tracks = [t for t in state.tracks if t not in remove]

    def _assign_reid(self, state, dist_mat, rows, cols, take):
        """tracker.py:246-265: every matched (inactive track r, detection c) within reid_sim_threshold is
        active again and takes its detection (`take(c, track)`) -> the detections assigned."""
        assigned, remove_inactive = [], []
        for r, c in zip(rows, cols):
            if dist_mat[r, c] <= self.reid_sim_threshold:
                track = state.inactive_tracks[r]
                self._logger(f'REID: track.id={track.id} - count_inactive={track.count_inactive} - '
                             f'to_inactive_frame={state.frame_index - track.count_inactive}')
                track.count_inactive = 0
                take(int(c), track)
                assigned.append(int(c))
                remove_inactive.append(track)
                state.tracks.append(track)
                state.num_reids += 1
        for track in remove_inactive:
            state.inactive_tracks.remove(track)
        return assigned

    def _count_new_tracks(self, state, new_track_ids):
        state.track_num += len(new_track_ids)
        if new_track_ids:
            self._logger(f'INIT TRACK IDS (detection_obj_score_thresh={self.detection_obj_score_thresh}): '
                         f'{new_track_ids}')

    @staticmethod
    def _end_frame(state, sim_only_move=None):
        """tracker.py:553-557; `sim_only_move` (reid_sim_only) sends every active track inactive."""
        for t in state.inactive_tracks:
            t.count_inactive += 1
        state.frame_index += 1
        if sim_only_move is not None:
            sim_only_move(state.tracks)


class Track:
    """tracker.py:1056-1130."""

    def __init__(self, pos, score, track_id, hs_embed, obj_ind, pos_rel=None, mask=None, attention_map=None):
        self.id = track_id
        self.pos = pos
        self.last_pos = deque([pos.clone()])
        self.last_pos_relative = deque([-1] if pos_rel is None else [pos_rel.clone()])
        self.score = score
        self.mask_row = None      # masks: the row of this frame's detector output the mask comes from
        self.mask_slot = None     # masks: the track's slot in the previous frame's label map
        self.mask_size = None     # masks: the (oh, ow) of that label map
        self.ims = deque([])
        self.count_inactive = 0
        self.count_termination = 0
        self.gt_id = None
        self.hs_embed = [hs_embed]
        self.mask = mask
        self.attention_map = attention_map
        self.obj_ind = obj_ind

    def has_positive_area(self):
        return bool(self.pos[2] > self.pos[0] and self.pos[3] > self.pos[1])

    def repeat_last_pos(self):
        self.last_pos.append(self.last_pos[-1])
        self.last_pos_relative.append(self.last_pos_relative[-1])

    def reset_last_pos(self, clear_relative=False):
        """tracker.py:1120-1124.  The reference also clears last_pos_relative, after which its
        repeat_last_pos raises IndexError on the next frame the track is not re-detected
        (tracker.py:1110-1114); this build keeps that list by default.  clear_relative=True
        (tracker cfg `reference_clear_last_pos_relative`) reproduces the reference exactly,
        defect included."""
        self.last_pos.clear()
        if clear_relative:
            self.last_pos_relative.clear()
        self.last_pos.append(self.pos.clone())


class Tracker(_TrackRules):
    """tracker.py:18-562 (image detector path)."""

    def __init__(self, obj_detector, obj_detector_post, tracker_cfg, generate_attention_maps=False, logger=None,
                 verbose=False):
        self._read_cfg(tracker_cfg, generate_attention_maps)
        self.masks = bool(tracker_cfg.get('masks', False))
        if 'segm' in obj_detector_post and not self.masks:
            # opt-in: the reference's own three-argument detector call (tracker.py:309) is a TypeError
            # with a masks model (DETRSegmBase.forward takes no prev_features)
            raise NotImplementedError('the tracker carries segmentation masks only with tracker_cfg[\'masks\'] = True: '
                                      'set it, or give the tracker the \'bbox\' postprocessor alone')
        if self.masks and 'segm' not in obj_detector_post:
            raise ValueError('tracker_cfg[\'masks\'] needs the \'segm\' postprocessor of a masks model')
        self.obj_detector = obj_detector
        self.obj_detector_post = obj_detector_post
        self.generate_attention_maps = False
        # compatibility switch for a reference defect (Track.reset_last_pos): False = keep the
        # relative-position history on re-identification (default), True = clear it as the
        # reference does (its next repeat_last_pos then raises IndexError)
        self.reference_clear_last_pos_relative = bool(tracker_cfg.get('reference_clear_last_pos_relative', False))
        self._logger = logger if logger is not None else (lambda *a: None)
        self._verbose = verbose

    @property
    def num_object_queries(self):
        return self.obj_detector.num_queries

    @property
    def device(self):
        return next(self.obj_detector.parameters()).device

    def reset(self, hard=True):
        self.tracks = []
        self.inactive_tracks = []
        self._prev_features = deque([None], maxlen=self.prev_frame_dist)
        self._label_maps = [None, None]     # masks: this frame's and the previous frame's labels (ping-pong)
        self._label_cur = 0
        if hard:
            self.track_num = 0
            self.results = {}
            self.frame_index = 0
            self.num_reids = 0

    def get_results(self):
        return self.results

    # ------------------------------------------------------------------ bookkeeping
    def _prune_inactive(self):
        """tracker.py:274-277 / :216-219 (one batched positive-area check)."""
        if not self.inactive_tracks:
            return
        pos = torch.stack([t.pos for t in self.inactive_tracks]).cpu()
        ok = ((pos[:, 2] > pos[:, 0]) & (pos[:, 3] > pos[:, 1])).tolist()
        self.inactive_tracks = [t for t, o in zip(self.inactive_tracks, ok)
                                if o and t.count_inactive <= self.inactive_patience]

    def move_tracks_to_inactive(self, inactive_tracks):
        self.tracks = [t for t in self.tracks if t not in inactive_tracks]
        for track in inactive_tracks:
            track.repeat_last_pos()
        self.inactive_tracks += inactive_tracks

    def add_tracks(self, pos, scores, hs_embeds, indices, rows=None):
        new_track_ids = []
        for i in range(len(pos)):
            self.tracks.append(Track(pos[i], scores[i], self.track_num + i, hs_embeds[i], indices[i]))
            if rows is not None:
                self.tracks[-1].mask_row = rows[i]
            new_track_ids.append(self.track_num + i)
        self._count_new_tracks(self, new_track_ids)
        return new_track_ids

    def public_detections_mask(self, new_det_boxes, public_det_boxes):
        """tracker.py:127-170."""
        return self._public_detections_mask(new_det_boxes, public_det_boxes).to(self.device)

    def _public_detections_mask(self, new_det_boxes, public_det_boxes):
        """The mask on the host (step reads it there too: the rows that survive are host knowledge)."""
        return public_detections_mask(self.public_detections, new_det_boxes, public_det_boxes, self.device)

    def reid(self, new_det_boxes, new_det_scores, new_det_hs_embeds, new_det_rows=None):
        """tracker.py:172-267: re-identify inactive tracks with the new detections.  new_det_rows
        (masks): the detections' rows of the frame's output; a matched track takes its detection's."""
        return self._reid(new_det_boxes, new_det_scores, new_det_hs_embeds, new_det_rows).to(self.device)

    def _reid(self, new_det_boxes, new_det_scores, new_det_hs_embeds, new_det_rows=None):
        self._prune_inactive()
        n = new_det_boxes.size(0)
        if not self.inactive_tracks or not n:
            return torch.ones(n, dtype=torch.bool)
        if self.reid_greedy_matching:
            nb = box_xyxy_to_cxcywh(new_det_boxes).cpu().numpy()
            ib = box_xyxy_to_cxcywh(torch.stack([t.pos for t in self.inactive_tracks])).cpu().numpy()
            dist_mat, rows, cols = reid_match_greedy(nb, ib)
        else:
            # F.pairwise_distance(track_sim, det_sim): ||x - y + 1e-6||_2, as one batched op
            sims = torch.stack([t.hs_embed[-1] for t in self.inactive_tracks])
            dist_mat = (sims[:, None, :] - new_det_hs_embeds[None, :, :] + 1e-6).norm(dim=-1).cpu().numpy()
            rows, cols = reid_match_lsa(dist_mat)

        def take(c, track):
            track.pos = new_det_boxes[c]
            track.score = new_det_scores[c]
            track.hs_embed.append(new_det_hs_embeds[c])
            track.reset_last_pos(self.reference_clear_last_pos_relative)
            if new_det_rows is not None:
                track.mask_row = new_det_rows[c]
        mask = torch.ones(n, dtype=torch.bool)
        for c in self._assign_reid(self, dist_mat, rows, cols, take):
            mask[c] = False
        return mask

    # ------------------------------------------------------------------ one frame
    @torch.no_grad()
    def step(self, blob):
        """tracker.py:269-557."""
        self._prune_inactive()
        self._logger(f'FRAME: {self.frame_index + 1}')
        for track in self.tracks:
            track.last_pos.append(track.pos.clone())
        img = blob['img'].to(self.device)
        orig_size = blob['orig_size'].to(self.device)
        Q = self.num_object_queries
        if self.masks and 'size' not in blob:
            raise ValueError('tracker masks need blob[\'size\'], the (1, 2) network-input frame size '
                             '(max_target_sizes of PostProcessSegm, tracker.py:322)')

        target = None
        prev = self.tracks + self.inactive_tracks
        num_prev_track = len(prev)
        if num_prev_track:
            boxes = box_xyxy_to_cxcywh(torch.stack([t.pos for t in prev]).float())
            hw = orig_size[0].float()
            boxes = boxes / torch.stack([hw[1], hw[0], hw[1], hw[0]])
            target = [{'track_query_boxes': boxes,
                       'image_id': torch.tensor([1], device=self.device),
                       'track_query_hs_embeds': torch.stack([t.hs_embed[-1] for t in prev])}]

        with deferred_masks(self.obj_detector, self.masks and hasattr(self.obj_detector, 'mask_logits')):
            outputs, _, features, _, _ = self.obj_detector(img, target, self._prev_features[0])
        hs_embeds = outputs['hs_embed'][0]
        result = self.obj_detector_post['bbox'](outputs, orig_size)[0]
        boxes = result['boxes'] if self.obj_detector.overflow_boxes else clip_boxes_to_image(result['boxes'],
                                                                                              orig_size[0])
        scores, labels = result['scores'], result['labels']
        person = labels == 0
        # every threshold decision of this frame in ONE device -> host copy
        dec = torch.stack([scores > self.track_obj_score_thresh, scores > self.reid_score_thresh,
                           scores > self.detection_obj_score_thresh, person])
        if self.masks:
            host, hw = copy_with_sizes(dec.flatten().view(torch.uint8), [blob['orig_size'], blob['size']],
                                       lambda t: t.cpu().numpy())
            dec = torch.from_numpy(host).view(dec.shape).bool()
            out_hw, net_hw = (tuple(int(v) for v in s) for s in hw)
        else:
            dec = dec.cpu()

        if num_prev_track:
            nt = num_prev_track
            track_keep = (dec[0, :nt] & dec[3, :nt]).tolist()
            reid_keep = (dec[1, :nt] & dec[3, :nt]).tolist()

            def take(i, track):
                track.score = scores[i]
                track.hs_embed.append(hs_embeds[i])
                track.pos = boxes[i]
                track.mask_row = i
            self._score_phase(self, track_keep, reid_keep, take, self.move_tracks_to_inactive)
            if self.track_nms_thresh and self.tracks:
                self._drop_suppressed(self, self._nms_keep(self.track_nms_thresh), 'track_nms_thresh')

        # new detections (tracker.py:456-505)
        det_keep = (dec[2, -Q:] & dec[3, -Q:]).nonzero().flatten()
        det_rows = (det_keep + (scores.shape[0] - Q)).tolist() if self.masks else None
        det_keep = det_keep.to(self.device)
        new_det_boxes = boxes[-Q:][det_keep]
        new_det_scores = scores[-Q:][det_keep]
        new_det_hs_embeds = hs_embeds[-Q:][det_keep]
        new_det_indices = det_keep[:, None]                 # .float().nonzero() indices (:469)
        pub = self._public_detections_mask(new_det_boxes, blob['dets'][0] if 'dets' in blob else [])
        if det_rows is not None:
            det_rows = [r for r, k in zip(det_rows, pub.tolist()) if k]
        pub = pub.to(self.device)
        new_det_boxes, new_det_scores = new_det_boxes[pub], new_det_scores[pub]
        new_det_hs_embeds, new_det_indices = new_det_hs_embeds[pub], new_det_indices[pub]
        reid_mask = self._reid(new_det_boxes, new_det_scores, new_det_hs_embeds, det_rows)
        if det_rows is not None:
            det_rows = [r for r, k in zip(det_rows, reid_mask.tolist()) if k]
        reid_mask = reid_mask.to(self.device)
        new_det_boxes, new_det_scores = new_det_boxes[reid_mask], new_det_scores[reid_mask]
        new_det_hs_embeds, new_det_indices = new_det_hs_embeds[reid_mask], new_det_indices[reid_mask]
        new_track_ids = self.add_tracks(new_det_boxes, new_det_scores, new_det_hs_embeds, new_det_indices, det_rows)

        if self.detection_nms_thresh and self.tracks:
            self._drop_suppressed(self, self._nms_keep(self.detection_nms_thresh, new_track_ids), 'detection_nms_thresh')

        # results (tracker.py:529-552), one batched copy
        if self.tracks:
            packed = self._result_rows(orig_size)
            if self.masks:
                # the label map rides in the same copy, as bytes behind the packed rows
                labels = self._resolve_masks(outputs, out_hw, net_hw)
                nb = packed.numel() * 4
                both = torch.cat([packed.contiguous().view(torch.uint8).flatten(),
                                  labels.view(torch.uint8).flatten()]).cpu().numpy()
                packed = both[:nb].view(np.float32).reshape(len(self.tracks), 6)
                labels = both[nb:].view(np.int16).reshape(out_hw)
            else:
                packed = packed.cpu().numpy()
            self._write_results(packed)
            if self.masks:
                for slot, track in enumerate(self.tracks):
                    self.results[track.id][self.frame_index]['mask'] = labels == slot
        self._prev_features.append(features)
        self._end_frame(self, self.move_tracks_to_inactive if self.reid_sim_only else None)

    def _nms_keep(self, thresh, new_track_ids=None):
        """K.nms over the active tracks -> one keep flag per track.  With `new_track_ids` (the detection
        NMS, tracker.py:511-521) every other track's score is lifted to inf: existing tracks always win."""
        scores = torch.stack([t.score for t in self.tracks])
        if new_track_ids is not None:
            new_ids = set(new_track_ids)
            scores[torch.tensor([t.id not in new_ids for t in self.tracks], device=self.device)] = float('inf')
        keep = set(K.nms(torch.stack([t.pos for t in self.tracks]), scores, thresh).tolist())
        return [i in keep for i in range(len(self.tracks))]

    def _result_rows(self, orig_size):
        """(tracks, 6) f32 on the device: the clipped box, the score and obj_ind of every active track."""
        pos = torch.stack([t.pos for t in self.tracks])
        if not self.obj_detector.overflow_boxes:
            pos = clip_boxes_to_image(pos, orig_size[0])
        return torch.cat([pos.float(), torch.stack([t.score for t in self.tracks]).float()[:, None],
                          torch.stack([t.obj_ind.reshape(()) for t in self.tracks]).float()[:, None]], 1)

    def _write_results(self, packed):
        """tracker.py:529-552 from the host copy of `_result_rows`."""
        for track, row in zip(self.tracks, packed):
            self.results.setdefault(track.id, {})[self.frame_index] = {
                'bbox': row[:4].copy(), 'score': np.float32(row[4]), 'obj_ind': int(row[5])}

    def _resolve_masks(self, outputs, out_hw, net_hw):
        """tracker.py:515-527 for the tracks alive at the end of the frame: slot t of the label map
        is self.tracks[t].  A track with a row of this frame is fresh; one that stayed active without
        being re-detected names its slot in the previous frame's map.  The head runs once, on the
        fresh rows; 0.5 is the reference's constant (:522), not the post-processor's threshold."""
        prev = self._label_maps[1 - self._label_cur]
        plan = plan_mask_resolve([self.tracks], [out_hw])
        src = plan['src'].tolist()
        idx = torch.tensor(plan['rows'], dtype=torch.int64, device=self.device)
        if hasattr(self.obj_detector, 'mask_logits'):
            logits = self.obj_detector.mask_logits(idx, 0)
        else:
            logits = outputs['pred_masks'][0].index_select(0, idx)
        cur = self._label_maps[self._label_cur]
        if cur is None or tuple(cur.shape) != out_hw:
            cur = self._label_maps[self._label_cur] = torch.empty(out_hw, dtype=torch.int16, device=self.device)
        stale = any(s < 0 for s in src)
        K.segm_track_resolve(logits, src, prev if stale else None, net_hw, net_hw, out_hw, 0.5, out=cur)
        for slot, track in enumerate(self.tracks):
            track.mask_row, track.mask_slot, track.mask_size = None, slot, out_hw
        self._label_cur = 1 - self._label_cur
        return cur


# ---------------------------------------------------------------------------------- KineT
# The kinematic tracker (tracker.py:580-959, TrackKinematic :961-1053) drives the KineT model
# (kinet_amd/models/kinet.py, `KinetTracking`) with each track's trail of the last n_frames
# relative boxes (+ its score trail) as tracklet queries.  As shipped the reference class
# cannot run past its first detections; the defects are fixed here by default and each is
# reproduced (same exception at the same step) when its name is in tracker_cfg
# ['reference_defects'] (tests/golden/make_golden.py gen_tracker_kinematic):
REFERENCE_DEFECTS = (
    # add_tracks passes `confidence=` (tracker.py:868), TrackKinematic.__init__ (:964) has no
    # such argument -> TypeError at the first new track.  Fixed: the [score, class] vector is
    # the track's `metadata`.
    'track_init_confidence_kwarg',
    # get_trail stacks 0-d scores into an (n_frames,) trail (:1039-1045) that step indexes
    # [:, :, :dim_metadata] (:661-662) -> IndexError once a track exists.  Fixed: (n_frames, 1).
    'metadata_trail_rank',
    # SineEncodingTracklet returns (B, n*4*F) (detr_tracking.py:305), step flattens it again
    # with .flatten(1, 2) (:660-662) -> IndexError, and add_tracks encodes a 2-d trail
    # (:869-870) -> IndexError.  Fixed: a 2-d trail gets a batch axis, the encoding is
    # (B, n, 4*F) -- the same values in the same order after the callers' flattens.
    'sine_encoding_rank',
    # Tracker.move_tracks_to_inactive (:88-94) calls track.repeat_last_pos(), which
    # TrackKinematic lacks (its method is repeat_last_state, :1018-1024) -> AttributeError
    # when a track first goes inactive.  Fixed: repeat_last_state.
    'inactive_repeat_method',
)


class IdentityEncoding:
    """detr_tracking.py:310-316."""

    def __call__(self, x):
        return x


class SineEncodingTracklet:
    """detr_tracking.py:286-307: sine / cosine features of tracklet coordinates in [0, 1]
    (x * 2 pi / temperature^(2 floor(i/2) / F), cos of the even, sin of the odd features) --
    (B, n, c) -> (B, n, c*F); `reference_rank` keeps the reference's (B, n*c*F) output and its
    failure on 2-d input."""

    def __init__(self, num_pos_feats=64, temperature=10000, scale=None, reference_rank=False):
        self.num_pos_feats = num_pos_feats
        self.temperature = temperature
        self.scale = 2 * math.pi if scale is None else scale   # (unused by the reference's __call__)
        self.reference_rank = reference_rank

    def __call__(self, x):
        if x.dim() == 2:
            if self.reference_rank:
                raise IndexError('too many indices for tensor of dimension 2')   # x[:, :, :, None] (:300)
            x = x[None]
        dim_t = torch.arange(self.num_pos_feats, dtype=torch.float32, device=x.device)
        dim_t = self.temperature ** (2 * (dim_t // 2) / self.num_pos_feats)
        freq = (x[:, :, :, None] * torch.pi * 2) / dim_t
        emb = torch.cat([freq[:, :, :, 0::2].cos(), freq[:, :, :, 1::2].sin()], dim=3)
        return emb.flatten(1) if self.reference_rank else emb.flatten(2)


def generate_pseudo_tracklets(detections, n_frames):
    """detr_tracking.py:319-326: each detection repeated as an n_frames trail."""
    return torch.tile(detections[:, None, :4], [1, n_frames, 1])


class TrackKinematic:
    """tracker.py:961-1053: position / relative-position / score histories of one track."""

    def __init__(self, pos, pos_rel, metadata, metadata_encoded, pos_encoded, track_id, obj_ind, mask=None):
        self.id = track_id
        self.pos = pos
        self.last_pos = deque([pos.clone()])
        self.last_score = deque([metadata[0].clone()])
        self.last_pos_relative = deque([-1] if pos_rel is None else [pos_rel.clone()])
        self.metadata_encoded = metadata_encoded
        self.position_encoded = pos_encoded
        self.mask = mask
        self.obj_ind = obj_ind
        self.count_inactive = 0
        self.count_termination = 0
        self.gt_id = None
        self.metadata = metadata

    def has_positive_area(self):
        return bool(self.pos[2] > self.pos[0] and self.pos[3] > self.pos[1])

    def update_state(self, pos, relative_pos, metadata, encoding_pos, encoding_metadata):
        self.last_pos.append(pos.clone())
        self.last_score.append(metadata[0].clone())
        self.pos = pos
        self.last_pos_relative.append(relative_pos.clone())
        self.metadata_encoded = encoding_metadata
        self.position_encoded = encoding_pos
        self.metadata = metadata

    @property
    def score(self):
        return self.metadata[0]

    def repeat_last_state(self):
        self.last_pos.append(self.last_pos[-1])
        self.last_pos_relative.append(self.last_pos_relative[-1])
        self.last_score.append(self.last_score[-1])

    def get_trail(self, n_frames, reference_rank=False):
        """(n_frames, 4) relative boxes, oldest first, padded with the first one, and the score
        trail: (n_frames, 1) (reference_rank: the reference's (n_frames,))."""
        present = min(n_frames, len(self.last_pos))
        idx = [0] * (n_frames - present) + [len(self.last_pos_relative) - present + i for i in range(present)]
        pos = torch.stack([self.last_pos_relative[i].clone() for i in idx], 0)
        meta = torch.stack([self.last_score[i].clone() for i in idx], 0)
        return pos, (meta if reference_rank else meta[:, None])

    def reset_last_pos(self):
        self.last_pos.clear()
        self.last_pos_relative.clear()
        self.last_pos.append(self.pos.clone())
        self.last_score.clear()


class TrackerKinematic(Tracker):
    """tracker.py:580-959: the online tracker over the KineT kinematic model (its detector input
    is the frame's detections + metadata, its track queries the tracks' box / score trails).
    Same constructor, reset / step / get_results as the reference (track.py:104-107 builds it
    from the detector's args); GPU post-process, thresholds and NMS kernel, one batched
    device -> host copy of the per-frame decisions, host bookkeeping."""

    def __init__(self, obj_detector, obj_detector_post, tracker_cfg, obj_detector_args, generate_attention_maps=False,
                 logger=None, verbose=False):
        if tracker_cfg.get('masks', False):
            # (the reference's own mask code in TrackerKinematic.step is commented out)
            raise NotImplementedError('TrackerKinematic does not carry segmentation masks')
        super().__init__(obj_detector, obj_detector_post, tracker_cfg, generate_attention_maps, logger, verbose)
        self.n_classes = tracker_cfg['n_classes']
        self.dim_metadata = 1 + self.n_classes if obj_detector_args.use_class else 1
        self.defects = frozenset(tracker_cfg.get('reference_defects', ()))
        unknown = self.defects - set(REFERENCE_DEFECTS)
        if unknown:
            raise ValueError(f'unknown reference_defects {sorted(unknown)} (known: {REFERENCE_DEFECTS})')
        if self.dim_metadata != 1 and 'metadata_trail_rank' not in self.defects:
            # the track keeps only its score history (last_score, :980), so a [score, class]
            # trail of use_class models has no source; the reference fails earlier anyway
            raise NotImplementedError('TrackerKinematic: use_class metadata trails (dim_metadata > 1)')
        self.use_empty_start = obj_detector_args.use_empty_start   # (collate choice of the loader)
        self.n_frames = obj_detector_args.track_prev_frame_range
        self.use_sine_encoding = obj_detector_args.use_encoding_tracklets
        if self.use_sine_encoding:
            rr = 'sine_encoding_rank' in self.defects
            self.encoder_tracklets_det = SineEncodingTracklet(obj_detector_args.encoding_dim_tracklets, reference_rank=rr)
            self.encoder_tracklets_metada = SineEncodingTracklet(obj_detector_args.encoding_dim_tracklets,
                                                                 reference_rank=rr)
        else:
            self.encoder_tracklets_det = IdentityEncoding()
            self.encoder_tracklets_metada = IdentityEncoding()

    def move_tracks_to_inactive(self, inactive_tracks):
        if inactive_tracks and 'inactive_repeat_method' in self.defects:
            raise AttributeError("'TrackKinematic' object has no attribute 'repeat_last_pos'")
        self.tracks = [t for t in self.tracks if t not in inactive_tracks]
        for track in inactive_tracks:
            track.repeat_last_state()
        self.inactive_tracks += inactive_tracks

    def _trail(self, track):
        return track.get_trail(self.n_frames, 'metadata_trail_rank' in self.defects)

    def _update(self, track, box, rel, meta):
        """manage_active_tracks / manage_inactive_tracks body (tracker.py:926-930, :937-941): the
        encodings of the trail BEFORE this update, passed in the reference's argument order
        (metadata encoding into `encoding_pos`, position encoding into `encoding_metadata`; they
        feed nothing the tracker outputs)."""
        pos_trail, meta_trail = self._trail(track)
        track.update_state(box, rel, meta,
                           self.encoder_tracklets_metada(meta_trail.view(1, self.n_frames, self.dim_metadata)).flatten(0),
                           self.encoder_tracklets_det(pos_trail[None]).flatten(0))

    def add_tracks(self, pos, pos_relatives, metadata_trail, pos_trail, indices, num_tracks):
        """tracker.py:858-890."""
        if len(pos) and 'track_init_confidence_kwarg' in self.defects:
            raise TypeError("TrackKinematic.__init__() got an unexpected keyword argument 'confidence'")
        new_track_ids = []
        for i in range(len(pos)):
            self.tracks.append(TrackKinematic(
                pos[i], pos_rel=pos_relatives[i], metadata=metadata_trail[i, -1],
                pos_encoded=self.encoder_tracklets_det(pos_trail[i]).flatten(0),
                metadata_encoded=self.encoder_tracklets_metada(metadata_trail[i, :, :self.dim_metadata]).flatten(0),
                track_id=self.track_num + i, obj_ind=indices[i]))
            new_track_ids.append(self.track_num + i)
        self._count_new_tracks(self, new_track_ids)
        return new_track_ids

    @torch.no_grad()
    def step(self, blob):
        """tracker.py:626-856."""
        self._prune_inactive()
        self._logger(f'FRAME: {self.frame_index + 1}')
        dev = self.device
        sample = blob[0].to(dev)
        labels = dict(blob[1][0])
        orig_size = labels['orig_size'].to(dev)[None]
        prev = self.tracks + self.inactive_tracks
        nt = len(prev)
        if nt:
            trails = [self._trail(t) for t in prev]
            det = self.encoder_tracklets_det(torch.stack([p for p, _ in trails], 0))
            meta = self.encoder_tracklets_metada(torch.stack([m for _, m in trails], 0)[:, :, :self.dim_metadata])
            labels['track_query_hs_embeds_det'] = det.flatten(1, 2)
            labels['track_query_hs_embeds_meta'] = meta.flatten(1, 2)
            labels = {k: v.to(dev) for k, v in labels.items()}
        else:
            labels['track_query_hs_embeds_det'] = torch.empty([0])
            labels['track_query_hs_embeds_meta'] = torch.empty([0])
        targets = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in labels.items()}]
        outputs, _, features, _, _ = self.obj_detector(sample, targets)
        result = self.obj_detector_post['bbox'](outputs, orig_size)[0]
        pred_boxes = outputs['pred_boxes'][0, :, :4]
        if self.obj_detector.overflow_boxes:
            boxes, relative_boxes = result['boxes'], pred_boxes
        else:
            boxes, relative_boxes = clip_boxes_to_image(result['boxes'], orig_size[0]), pred_boxes.clamp(0.0, 1.0)
        scores, cls = result['scores'], result['labels']
        # every threshold decision of this frame in ONE device -> host copy
        dec = torch.stack([scores > self.track_obj_score_thresh, scores > self.reid_score_thresh,
                           scores > self.detection_obj_score_thresh, cls == 0, cls < self.n_classes]).cpu()

        if nt:
            track_keep = (dec[0, :nt] & dec[3, :nt]).tolist()
            reid_keep = (dec[1, :nt] & dec[3, :nt]).tolist()
            track_boxes, track_rel = boxes[:nt], pred_boxes[:nt]
            track_meta = torch.stack([scores[:nt], cls[:nt].to(scores.dtype)], dim=1)
            # manage_active_tracks (:933-955), manage_inactive_tracks (:922-931)
            self._score_phase(self, track_keep, reid_keep,
                              lambda i, track: self._update(track, track_boxes[i], track_rel[i], track_meta[i]),
                              self.move_tracks_to_inactive)
            if self.track_nms_thresh and self.tracks:
                self._drop_suppressed(self, self._nms_keep(self.track_nms_thresh), 'track_nms_thresh')

        # new detections (generate_new_tracks, :892-920)
        keep = (dec[2, nt:] & dec[4, nt:]).nonzero().flatten().to(dev)
        new_boxes, new_rel = boxes[nt:][keep], relative_boxes[nt:][keep]
        new_scores, new_cls = scores[nt:][keep], cls[nt:][keep]
        new_indices = keep[:, None]                                   # .float().nonzero() (:907)
        pub = self.public_detections_mask(new_boxes, blob[0].detections)
        new_boxes, new_rel, new_scores, new_indices = new_boxes[pub], new_rel[pub], new_scores[pub], new_indices[pub]
        new_tracklets = generate_pseudo_tracklets(new_rel, self.n_frames)
        new_cls = new_cls[pub] / self.n_classes
        new_meta = torch.tile(torch.stack([new_scores, new_cls.to(new_scores.dtype)], 1)[:, None, :],
                              dims=(1, self.n_frames, 1))
        new_track_ids = self.add_tracks(new_boxes, new_rel, new_meta, new_tracklets, new_indices, nt)

        if self.detection_nms_thresh and self.tracks:                # (:790-808)
            self._drop_suppressed(self, self._nms_keep(self.detection_nms_thresh, new_track_ids), 'detection_nms_thresh')

        if self.tracks:                                               # results (:828-841), one copy
            self._write_results(self._result_rows(orig_size).cpu().numpy())
        self._end_frame(self)                                         # (this step has no reid_sim_only move)


# ---------------------------------------------------------------------------------- multi-sequence
# S independent sequences advanced in lock-step on ONE batched detector forward per frame (DESIGN.md
# section 4 "Multi-sequence tracker").  Sequence i holds K_i track queries; the batch carries
# Kmax = max K_i rows per sample and marks rows K_i..Kmax-1 as placeholders
# (targets[i]['track_queries_placeholder_mask'], kinet_amd/models/deformable_transformer.py).  The
# tracks' embeddings, boxes and scores live in a device table (the track bank, one row = slot per
# track, include/kinet_track.h); the state machine of each sequence is Tracker.step's -- the same
# functions (_TrackRules), called with the sequence as their state -- on host mirrors (numpy) of the
# boxes and scores.

def plan_track_queries(n_active, n_inactive, num_queries):
    """The host plan of one frame's track queries: per-sequence counts of active and inactive tracks ->
    {'K': (S,) int32 K_i = n_active[i] + n_inactive[i], 'Kmax': max K_i, 'offsets': (S + 1,) int32 starts of
    the sequences' slot lists in one flat list, 'mask': (S, Kmax + Q) bool, True exactly on rows K_i..Kmax-1}."""
    k = np.asarray(n_active, np.int64).reshape(-1) + np.asarray(n_inactive, np.int64).reshape(-1)
    if k.size == 0 or (k < 0).any():
        raise ValueError(f'plan_track_queries: counts {list(n_active)}, {list(n_inactive)}')
    kmax = int(k.max())
    if kmax + num_queries > K.TRACK_MAX_ROWS:
        raise ValueError(f'{kmax} track queries + {num_queries} object queries exceed the tracker kernels\' '
                         f'{K.TRACK_MAX_ROWS} rows per sequence')
    offsets = np.zeros(k.size + 1, np.int32)
    offsets[1:] = np.cumsum(k)
    col = np.arange(kmax + num_queries)[None, :]
    mask = (col >= k[:, None]) & (col < kmax)
    return {'K': k.astype(np.int32), 'Kmax': kmax, 'offsets': offsets, 'mask': mask}


def plan_mask_resolve(tracks, out_hws):
    """The host plan of one frame's mask resolution (Tracker._resolve_masks for every sequence at once):
    tracks[b] the tracks of sequence b alive at the end of the frame, in slot order (objects with id,
    mask_row -- the GLOBAL frame row b * Nrows + row of this frame's detector output, or None --, mask_slot
    and mask_size), out_hws[b] its (oh, ow) ->
    {'rows': the distinct frame rows whose mask logits are needed, in order of first use (a row named by
     two tracks -- of one sequence or of two -- is computed once), 'src': (total,) int32, >= 0 an index into
     'rows', < 0 the stale slot -e-1 of the sequence's previous map, 'src_off': (S + 1,) int32}.
    Raises Tracker's two RuntimeErrors: a stale track whose kept map has another size, and a track with
    neither a row of this frame nor a kept mask."""
    rows, src = {}, []
    src_off = np.zeros(len(tracks) + 1, np.int32)
    for b, (seq, out_hw) in enumerate(zip(tracks, out_hws)):
        for track in seq:
            if track.mask_row is not None:
                src.append(rows.setdefault(int(track.mask_row), len(rows)))
            elif track.mask_slot is not None:
                if tuple(track.mask_size) != tuple(out_hw):
                    raise RuntimeError(f'track {track.id} keeps a mask of size {track.mask_size}, the frame is '
                                       f'{tuple(out_hw)} (the reference\'s torch.stack fails there too)')
                src.append(-int(track.mask_slot) - 1)
            else:
                raise RuntimeError(f'track {track.id} has neither a mask row of this frame nor a kept mask')
        src_off[b + 1] = len(src)
    return {'rows': list(rows), 'src': np.asarray(src, np.int32), 'src_off': src_off}


class _SlotTrack:
    """One track of a MultiTracker sequence: Track's bookkeeping fields with host mirrors (numpy f32) of
    the box and the score; the embedding and the device copies are row `slot` of the track bank.  (Track's
    last_pos history feeds nothing the tracker outputs and is not kept.)  Masks: mask_row is the global
    frame row b * Nrows + row this frame's mask comes from, mask_slot the track's slot in its sequence's
    previous label map, mask_size that map's (oh, ow) (Track's fields)."""
    __slots__ = ('id', 'pos', 'score', 'slot', 'obj_ind', 'count_inactive', 'count_termination', 'mask_row',
                 'mask_slot', 'mask_size')

    def __init__(self, pos, score, track_id, slot, obj_ind):
        self.id, self.pos, self.score, self.slot, self.obj_ind = track_id, pos, score, slot, obj_ind
        self.count_inactive = 0
        self.count_termination = 0
        self.mask_row = self.mask_slot = self.mask_size = None


class _Sequence:
    def __init__(self):
        self.retired = False
        self.tracks, self.inactive_tracks = [], []
        self.track_num = self.frame_index = self.num_reids = 0
        self.results = {}
        self.map_off = None     # masks: element offset of the sequence's map in the previous packed label buffer

    def move_tracks_to_inactive(self, inactive_tracks):
        self.tracks = [t for t in self.tracks if t not in inactive_tracks]
        self.inactive_tracks += inactive_tracks


class MultiTracker(_TrackRules):
    """`num_sequences` Trackers in one: reset(), step(blobs) with one blob per live sequence (the keys
    Tracker.step reads; frame sizes may differ), retire(i), get_results() -> one Tracker.get_results()
    dict per sequence.  Track ids, track_num, num_reids and frame_index are per sequence
    (`sequence(i)`).  Every device -> host transfer of step goes through `_to_host`, which counts
    them in `sync_count`: at most four per step (decisions, track NMS, re-identification distances,
    detection NMS), each skipped when no sequence needs it, whatever S is.
    Masks (tracker_cfg['masks'] with the 'segm' postprocessor; blob['size'] is then required): after the
    detection NMS the mask head runs ONCE on the surviving tracks' rows of all sequences
    (DETRSegmBase.mask_logits_rows; the detector runs with defer_masks), ONE
    kinet_segm_track_resolve_segments launch writes every sequence's int16 label map and each slot's pixel
    count and box into one packed buffer, and a fifth transfer carries it: results[id][frame]['mask'] is
    a numpy bool (oh, ow) built inside the slot's box only.  Two packed buffers ping-pong (a stale track
    names its slot in its sequence's previous map)."""

    def __init__(self, obj_detector, obj_detector_post, tracker_cfg, num_sequences, logger=None,
                 generate_attention_maps=False):
        from kinet_amd.models.deformable_detr import DeformablePostProcess
        from kinet_amd.models.kinet import KinematicDetectorTransformer
        self._read_cfg(tracker_cfg, generate_attention_maps or tracker_cfg.get('generate_attention_maps', False))
        self.masks = bool(tracker_cfg.get('masks', False))
        if self.masks and 'segm' not in obj_detector_post:
            raise NotImplementedError('MultiTracker carries segmentation masks (MOTS) only with the \'segm\' '
                                      'postprocessor of a masks model')
        if 'segm' in obj_detector_post and not self.masks:
            raise NotImplementedError('MultiTracker takes the \'segm\' postprocessor only with '
                                      'tracker_cfg[\'masks\'] = True')
        if type(obj_detector_post.get('bbox')) is not DeformablePostProcess:
            raise NotImplementedError('MultiTracker runs DeformablePostProcess on the device '
                                      '(kinet_track_decide); other postprocessors are not built')
        if isinstance(obj_detector, KinematicDetectorTransformer):
            raise NotImplementedError('MultiTracker does not drive the kinematic detector: use TrackerKinematic')
        if num_sequences < 1:
            raise ValueError(f'num_sequences={num_sequences}')
        self.obj_detector = obj_detector
        self.obj_detector_post = obj_detector_post
        self.num_sequences = int(num_sequences)
        self._logger = logger if logger is not None else (lambda *a: None)
        self.sync_count = 0
        self.reset()

    @property
    def num_object_queries(self):
        return self.obj_detector.num_queries

    @property
    def device(self):
        return next(self.obj_detector.parameters()).device

    def reset(self):
        self._seqs = [_Sequence() for _ in range(self.num_sequences)]
        self._prev_features = deque([None], maxlen=self.prev_frame_dist)
        self._bank = None            # (capacity, d + 5) f32, allocated at the first frame (d is the detector's)
        self._free_slots, self._next_slot = [], 0
        self._pending = ([], [])     # (frame rows, bank slots) to commit with the next launch
        self._sizes_key, self._sizes = None, None
        self._mask_bufs, self._mask_cur = [None, None], 0   # masks: the packed stats + labels buffers (ping-pong)
        self._prev_labels = None                            # masks: the labels view of the last resolve
        self.mask_seconds = 0.0                             # masks: host time spent building the bool masks
        self.sync_count = 0

    def sequence(self, i):
        """The per-sequence counters: .track_num, .num_reids, .frame_index, .tracks, .inactive_tracks."""
        return self._seqs[i]

    def live_sequences(self):
        return [i for i, q in enumerate(self._seqs) if not q.retired]

    def get_results(self):
        return [q.results for q in self._seqs]

    def retire(self, i):
        """Remove sequence i for good: its results stay, its slots are freed and every cached
        previous-feature NestedTensor loses its batch row."""
        q = self._seqs[i]
        if q.retired:
            raise ValueError(f'sequence {i} is already retired')
        row = self.live_sequences().index(i)
        for t in q.tracks + q.inactive_tracks:
            self._free(t.slot)
        q.tracks, q.inactive_tracks = [], []
        q.retired = True
        q.map_off = None
        self._sizes_key = None
        for features in self._prev_features:
            if features is None:
                continue
            for f in features:
                if not hasattr(f, 'tensors'):
                    continue
                keep = [r for r in range(f.tensors.shape[0]) if r != row]
                f.tensors = f.tensors[keep]
                if f.mask is not None:
                    f.mask = f.mask[keep]
                if getattr(f, 'sizes', None) is not None:
                    f.sizes = tuple(s for r, s in enumerate(f.sizes) if r != row)

    # ------------------------------------------------------------------ device plumbing
    def _to_host(self, t):
        """THE device -> host transfer of step (each one waits for the stream)."""
        self.sync_count += 1
        return t.cpu().numpy()

    def _upload(self, *arrays):
        """Small host index arrays (int32 / uint8) as views of ONE device buffer: one pinned,
        non-blocking copy per phase of the step."""
        parts, spans, o = [], [], 0
        for a in arrays:
            b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            pad = (-b.size) % 4
            parts += [b, np.zeros(pad, np.uint8)]
            spans.append((o, b.size, a.dtype))
            o += b.size + pad
        host = np.concatenate(parts) if o else np.zeros(4, np.uint8)
        buf = torch.from_numpy(host)
        buf = buf.pin_memory().to(self.device, non_blocking=True) if self.device.type == 'cuda' else buf
        return [buf[s:s + n] if dt == np.uint8 else buf[s:s + n].view(torch.int32) for s, n, dt in spans]

    def _alloc(self):
        if self._free_slots:
            return self._free_slots.pop()
        if self._next_slot == self._bank.shape[0]:
            grown = torch.zeros((2 * self._bank.shape[0], self._bank.shape[1]), dtype=torch.float32, device=self.device)
            grown[:self._bank.shape[0]] = self._bank
            self._bank = grown
        self._next_slot += 1
        return self._next_slot - 1

    def _free(self, slot):
        rows, slots = self._pending
        if slot in slots:
            keep = [p for p, s in enumerate(slots) if s != slot]
            self._pending = ([rows[p] for p in keep], [slots[p] for p in keep])
        self._free_slots.append(slot)

    def _flush(self, frame, *arrays):
        """Upload `arrays` together with the pending commits and launch the commit -> the arrays' device views."""
        rows, slots = self._pending
        self._pending = ([], [])
        if not rows and not arrays:
            return []
        dev = self._upload(np.asarray(rows, np.int32), np.asarray(slots, np.int32), *arrays)
        if rows:
            K.track_commit(frame['hs'], frame['boxes'], frame['scores'], dev[0], dev[1], len(rows), self._bank)
        return dev[2:]

    def _nms(self, frame, segments, thresh, flags=None):
        """One kinet_nms_segments launch over the bank for the listed sequences' slot lists -> the keep
        lists, or None when no sequence has a segment (no launch, no transfer; the pending commits wait
        for the next launch)."""
        if not any(len(s) for s in segments):
            return None
        offsets = np.zeros(len(segments) + 1, np.int32)
        offsets[1:] = np.cumsum([len(s) for s in segments])
        idx = np.asarray([t for s in segments for t in s], np.int32)
        total = int(offsets[-1])
        d = self._bank.shape[1] - 5
        if flags is None:
            idx_d, off_d = self._flush(frame, idx, offsets)
            flag_d = None
        else:
            idx_d, off_d, flag_d = self._flush(frame, idx, offsets, np.asarray([f for s in flags for f in s], np.uint8))
        keep = self._to_host(K.nms_segments(self._bank[:, d:d + 4], self._bank[:, d + 4], idx_d, off_d, total, thresh,
                                            inf_flag=flag_d))
        return [keep[offsets[b]:offsets[b + 1]] for b in range(len(segments))]

    # ------------------------------------------------------------------ bookkeeping (Tracker's, per sequence)
    def _prune_inactive(self, q):
        kept = []
        for t in q.inactive_tracks:
            if t.pos[2] > t.pos[0] and t.pos[3] > t.pos[1] and t.count_inactive <= self.inactive_patience:
                kept.append(t)
            else:
                self._free(t.slot)
        q.inactive_tracks = kept

    def _release(self, track):
        self._free(track.slot)

    # ------------------------------------------------------------------ masks
    def _resolve_masks(self, seqs, outputs, Nrows, out_hws, net_hws):
        """Tracker._resolve_masks for every sequence at once (tracker.py:515-527): slot t of sequence b's
        label map is seqs[b].tracks[t].  One pass of the head over the distinct fresh rows of all
        sequences, one segmented resolve launch, one transfer of the packed statistics + label maps ->
        per sequence the tracks' bool (oh, ow) masks, each built inside its slot's box.  0.5 is the
        reference's constant (:522).  Nothing is launched or copied when no sequence has a track."""
        plan = plan_mask_resolve([q.tracks for q in seqs], out_hws)
        total = int(plan['src_off'][-1])
        if not total:
            for q in seqs:
                q.map_off = None
            return [[] for _ in seqs]
        idx = torch.from_numpy(np.asarray(plan['rows'], np.int64)).to(self.device)
        if hasattr(self.obj_detector, 'mask_logits_rows'):
            logits = self.obj_detector.mask_logits_rows(idx % Nrows, (idx // Nrows).to(torch.int32))
        else:
            logits = outputs['pred_masks'].flatten(0, 1).index_select(0, idx)
        # PostProcessSegm's rule: the bilinear target is the element-wise maximum of the batch's sizes
        max_hw = (max(s[0] for s in net_hws), max(s[1] for s in net_hws))
        geom = [net_hws[b] + out_hws[b] if q.tracks else (0, 0, 0, 0) for b, q in enumerate(seqs)]
        # (a sequence reads its previous map only when one of its slots is stale: the plan has checked its size)
        so = plan['src_off']
        prev_off = [q.map_off if q.map_off is not None and (plan['src'][so[b]:so[b + 1]] < 0).any() else -1
                    for b, q in enumerate(seqs)]
        src_d, = self._upload(plan['src'])
        cur = self._mask_cur
        buf, _, labels_d, pix_off = K.segm_track_resolve_segments(
            logits, src_d, plan['src_off'], geom, self._prev_labels, prev_off, max_hw, 0.5, out=self._mask_bufs[cur])
        if self._mask_bufs[cur] is None or self._mask_bufs[cur].numel() < buf.numel():
            self._mask_bufs[cur] = buf
        self._mask_cur, self._prev_labels = 1 - cur, labels_d
        stats, labels = K.segm_resolve_views(self._to_host(buf), total, int(pix_off[-1]))
        t0 = time.perf_counter()
        out = []
        for b, q in enumerate(seqs):
            oh, ow = out_hws[b]
            q.map_off = int(pix_off[b]) if q.tracks else None
            lab = labels[pix_off[b]:pix_off[b + 1]].reshape(oh, ow) if q.tracks else None
            per = []
            for slot, track in enumerate(q.tracks):
                track.mask_row, track.mask_slot, track.mask_size = None, slot, (oh, ow)
                n, x0, y0, x1, y1 = (int(v) for v in stats[plan['src_off'][b] + slot])
                m = np.zeros((oh, ow), np.bool_)
                if n:
                    m[y0:y1, x0:x1] = lab[y0:y1, x0:x1] == slot
                per.append(m)
            out.append(per)
        self.mask_seconds += time.perf_counter() - t0
        return out

    # ------------------------------------------------------------------ one frame of every live sequence
    @torch.no_grad()
    def step(self, blobs):
        """Tracker.step for every live sequence: blobs[j] belongs to the j-th live sequence."""
        from kinet_amd.models.misc import nested_tensor_from_tensor_list
        live = self.live_sequences()
        if len(blobs) != len(live):
            raise ValueError(f'step takes one blob per live sequence: {len(live)} live, {len(blobs)} blobs')
        if not live:
            return
        seqs = [self._seqs[i] for i in live]
        B, Q, dev = len(seqs), self.num_object_queries, self.device
        if self.masks and any('size' not in b for b in blobs):
            raise ValueError('tracker masks need blob[\'size\'], the (1, 2) network-input frame size '
                             '(max_target_sizes of PostProcessSegm, tracker.py:322)')
        for q in seqs:
            self._prune_inactive(q)
            self._logger(f'FRAME: {q.frame_index + 1}')
        samples = nested_tensor_from_tensor_list([b['img'].to(dev).reshape(b['img'].shape[-3:]) for b in blobs])
        key = tuple(b['orig_size'] for b in blobs)
        if self._sizes_key is None or len(key) != len(self._sizes_key) or any(a is not b for a, b in zip(key, self._sizes_key)):
            # (the blobs of a sequence usually share one orig_size tensor: converted once)
            self._sizes_key = key
            self._sizes = torch.cat([t.reshape(-1)[:2].reshape(1, 2) for t in key]).to(dev, torch.float32).contiguous()
        sizes = self._sizes

        plan = plan_track_queries([len(q.tracks) for q in seqs], [len(q.inactive_tracks) for q in seqs], Q)
        Kmax, Nrows = plan['Kmax'], plan['Kmax'] + Q
        n_act = np.asarray([len(q.tracks) for q in seqs], np.int32)
        slots = np.asarray([t.slot for q in seqs for t in q.tracks + q.inactive_tracks], np.int32)
        n_act_d, n_inact_d, off_d, slots_d = self._upload(n_act, plan['K'] - n_act, plan['offsets'], slots)
        targets = None
        if Kmax:
            embeds, qboxes, mask = K.track_gather(self._bank, slots_d, off_d, sizes, Kmax, Q)
            targets = [{'track_query_boxes': qboxes[b], 'track_query_hs_embeds': embeds[b],
                        'track_queries_placeholder_mask': mask[b]} for b in range(B)]
        with deferred_masks(self.obj_detector, self.masks and hasattr(self.obj_detector, 'mask_logits_rows')):
            outputs, _, features, _, _ = self.obj_detector(samples, targets, self._prev_features[0])
        hs =outputs['hs_embed'].float().contiguous()
        logits = outputs['pred_logits'].float().contiguous()
        if tuple(logits.shape[:2]) != (B, Nrows):
            raise RuntimeError(f'the detector returned {tuple(logits.shape[:2])} rows for {B} sequences of {Kmax} track '
                               f'+ {Q} object queries')
        d = hs.shape[-1]
        if self._bank is None:
            self._bank = torch.zeros((256, d + 5), dtype=torch.float32, device=dev)
        packed = K.track_decide(logits, outputs['pred_boxes'].float().contiguous(), sizes, n_act_d, n_inact_d, Kmax,
                                self.track_obj_score_thresh, self.reid_score_thresh, self.detection_obj_score_thresh,
                                not self.obj_detector.overflow_boxes)
        boxes_d, scores_d, _, _ = K.track_decide_views(packed, B, Nrows)
        frame = {'hs': hs.view(B * Nrows, d), 'boxes': boxes_d.view(B * Nrows, 4), 'scores': scores_d.view(B * Nrows)}
        # every box, score and threshold decision of this frame, all sequences, in ONE copy
        out_hws = net_hws = None
        if self.masks:
            host, hw = copy_with_sizes(packed, [t for blob in blobs for t in (blob['orig_size'], blob['size'])],
                                       self._to_host)
            out_hws = [tuple(int(v) for v in s) for s in hw[0::2]]
            net_hws = [tuple(int(v) for v in s) for s in hw[1::2]]
        else:
            host = self._to_host(packed)
        boxes, scores, _, dec = K.track_decide_views(host, B, Nrows)
        person = (dec & K.TRACK_DEC_PERSON) != 0

        def update(b, row, track):
            """The track takes row `row` of sequence b's outputs: host mirrors now, its bank slot with the
            next launch."""
            track.score = scores[b, row]
            track.pos = boxes[b, row].copy()
            if self.masks:
                track.mask_row = b * Nrows + row
            self._pending[0].append(b * Nrows + row)
            self._pending[1].append(track.slot)

        # tracks kept / terminated / re-identified by score, then track NMS (tracker.py:351-447)
        segments = []
        for b, q in enumerate(seqs):
            nt = int(plan['K'][b])
            if not nt:
                segments.append([])
                continue
            track_keep = ((dec[b, :nt] & K.TRACK_DEC_TRACK) != 0) & person[b, :nt]
            reid_keep = ((dec[b, :nt] & K.TRACK_DEC_REID) != 0) & person[b, :nt]
            self._score_phase(q, track_keep, reid_keep, functools.partial(update, b), q.move_tracks_to_inactive)
            segments.append([t.slot for t in q.tracks] if self.track_nms_thresh else [])
        keeps = self._nms(frame, segments, self.track_nms_thresh)
        if keeps is not None:
            for q, seg, keep in zip(seqs, segments, keeps):
                if seg:
                    self._drop_suppressed(q, keep, 'track_nms_thresh', self._release)

        # new detections (tracker.py:456-505): thresholds and public-detection gating on the host mirrors
        dets = []
        for b, (q, blob) in enumerate(zip(seqs, blobs)):
            det_keep = (((dec[b, Kmax:] & K.TRACK_DEC_DET) != 0) & person[b, Kmax:]).nonzero()[0]
            new_boxes = torch.from_numpy(boxes[b, Kmax:][det_keep])
            pub_dets = blob['dets'][0] if 'dets' in blob else []
            pub = public_detections_mask(self.public_detections, new_boxes,
                                         pub_dets.cpu() if torch.is_tensor(pub_dets) else pub_dets).numpy()
            det_keep = det_keep[pub]
            self._prune_inactive(q)                          # (Tracker._reid's first statement)
            dets.append(det_keep)
        dist = [None] * B
        if not self.reid_greedy_matching:
            need = [b for b, q in enumerate(seqs) if q.inactive_tracks and len(dets[b])]
            if need:
                # the embedding distances of every sequence that has inactive tracks and new detections
                a_off, r_off, o_off = (np.zeros(B + 1, np.int32) for _ in range(3))
                a_list, r_list = [], []
                for b, q in enumerate(seqs):
                    if b in need:
                        a_list += [t.slot for t in q.inactive_tracks]
                        r_list += (dets[b] + (b * Nrows + Kmax)).tolist()
                    a_off[b + 1], r_off[b + 1] = len(a_list), len(r_list)
                    o_off[b + 1] = o_off[b] + (a_off[b + 1] - a_off[b]) * (r_off[b + 1] - r_off[b])
                a_d, ao_d, r_d, ro_d, oo_d = self._flush(frame, np.asarray(a_list, np.int32), a_off,
                                                         np.asarray(r_list, np.int32), r_off, o_off)
                flat = self._to_host(K.track_reid_dist(self._bank, frame['hs'], a_d, ao_d, r_d, ro_d, oo_d, int(o_off[-1])))
                for b in need:
                    dist[b] = flat[o_off[b]:o_off[b + 1]].reshape(a_off[b + 1] - a_off[b], r_off[b + 1] - r_off[b])

        # re-identification, new tracks, detection NMS (tracker.py:172-267, :505-527)
        segments, flags = [], []
        for b, q in enumerate(seqs):
            det_keep = dets[b]
            n = len(det_keep)
            reid_mask = np.ones(n, bool)
            if q.inactive_tracks and n:
                if self.reid_greedy_matching:
                    nb = box_xyxy_to_cxcywh(torch.from_numpy(boxes[b, Kmax:][det_keep])).numpy()
                    ib = box_xyxy_to_cxcywh(torch.from_numpy(np.stack([t.pos for t in q.inactive_tracks]))).numpy()
                    dist_mat, rows, cols = reid_match_greedy(nb, ib)
                else:
                    dist_mat = dist[b]
                    rows, cols = reid_match_lsa(dist_mat)
                reid_mask[self._assign_reid(q, dist_mat, rows, cols,
                                            lambda c, track: update(b, Kmax + int(det_keep[c]), track))] = False
            new_ids = []
            for j in det_keep[reid_mask].tolist():
                track = _SlotTrack(None, None, q.track_num + len(new_ids), self._alloc(), j)
                update(b, Kmax + j, track)
                q.tracks.append(track)
                new_ids.append(track.id)
            self._count_new_tracks(q, new_ids)
            if self.detection_nms_thresh and q.tracks:
                fresh = set(new_ids)
                segments.append([t.slot for t in q.tracks])
                flags.append([t.id not in fresh for t in q.tracks])   # existing tracks always win (:519)
            else:
                segments.append([])
                flags.append([])
        keeps = self._nms(frame, segments, self.detection_nms_thresh, flags)
        if keeps is not None:
            for q, seg, keep in zip(seqs, segments, keeps):
                if seg:
                    self._drop_suppressed(q, keep, 'detection_nms_thresh', self._release)
        self._flush(frame)                                   # (commits no launch of this frame carried)

        masks = self._resolve_masks(seqs, outputs, Nrows, out_hws, net_hws) if self.masks else None

        # results (tracker.py:529-552) from the host mirrors: decide already clipped them to the image
        for b, q in enumerate(seqs):
            for slot, track in enumerate(q.tracks):
                q.results.setdefault(track.id, {})[q.frame_index] = {
                    'bbox': track.pos.copy(), 'score': np.float32(track.score), 'obj_ind': int(track.obj_ind)}
                if masks is not None:
                    q.results[track.id][q.frame_index]['mask'] = masks[b][slot]
            self._end_frame(q, q.move_tracks_to_inactive if self.reid_sim_only else None)
        self._prev_features.append(features)
