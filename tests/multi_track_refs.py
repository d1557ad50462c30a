"""Shared by the multi-sequence tracker's tests (test infrastructure): a batched stand-in detector built
from the tracker fixtures' FakeDetector, and plain torch / numpy restatements of the five kernels of
include/kinet_track.h (what kinet_amd.tracker.Tracker computes with torch ops, batched)."""
import numpy as np
import torch

DEC_TRACK, DEC_REID, DEC_DET, DEC_PERSON = 1, 2, 4, 8


class BatchedFakeDetector(torch.nn.Module):
    """One fake_detector.FakeDetector(seed=s) per sequence behind the batched, ragged interface of the
    Deformable detector: for sample i it reads K_i from `track_queries_placeholder_mask`, calls sequence
    i's fake with the first K_i track queries (targets=None when K_i = 0, exactly as Tracker does), pads
    the fake's outputs back to Kmax track rows with NaN logits, boxes and embeddings, and concatenates
    over the batch.  `retire(i)` drops the i-th of the live sequences, as MultiTracker.retire does."""

    def __init__(self, seeds, **kw):
        super().__init__()
        from fake_detector import FakeDetector
        self.fakes = torch.nn.ModuleList([FakeDetector(seed=s, **kw) for s in seeds])
        self.live = list(range(len(seeds)))
        self.num_queries = self.fakes[0].num_queries
        self.overflow_boxes = self.fakes[0].overflow_boxes
        self.calls = []          # K_i per sample of every call

    def retire(self, i):
        self.live.remove(i)

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
                nan = torch.full((1, kmax - k, v.shape[-1]), float('nan'), dtype=v.dtype, device=v.device)
                pad[name] = torch.cat([v[:, :k], nan, v[:, k:]], 1)
            outs.append(pad)
            ks.append(k)
        self.calls.append(ks)
        out = {name: torch.cat([o[name] for o in outs]) for name in outs[0]}
        return out, None, ['features of the batch'], None, None


# ---------------------------------------------------------------------------------- restatements
def decide_ref(pred_logits, pred_boxes, sizes, k, kmax, t_track, t_reid, t_det, clip):
    """kinet_track_decide with torch ops (DeformablePostProcess + clip_boxes_to_image + Tracker.step's
    compares): -> boxes (S, N, 4), scores (S, N), labels (S, N) int32, decisions (S, N) uint8; zeros on the
    placeholder rows k[s]..kmax-1."""
    prob = pred_logits.sigmoid()
    scores, labels = prob.max(-1)
    cx, cy, w, h = pred_boxes.unbind(-1)
    boxes = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)
    img_h, img_w = sizes.unbind(1)
    boxes = boxes * torch.stack([img_w, img_h, img_w, img_h], 1)[:, None, :]
    if clip:
        x = torch.minimum(boxes[..., 0::2].clamp(min=0), img_w[:, None, None])
        y = torch.minimum(boxes[..., 1::2].clamp(min=0), img_h[:, None, None])
        boxes = torch.stack([x[..., 0], y[..., 0], x[..., 1], y[..., 1]], -1)
    dec = ((scores > t_track) * DEC_TRACK + (scores > t_reid) * DEC_REID + (scores > t_det) * DEC_DET
           + (labels == 0) * DEC_PERSON).to(torch.uint8)
    row = torch.arange(pred_logits.shape[1])[None, :]
    ph = (row >= torch.as_tensor(k)[:, None]) & (row < kmax)
    boxes = torch.where(ph[..., None], torch.zeros_like(boxes), boxes)
    scores = torch.where(ph, torch.zeros_like(scores), scores)
    labels = torch.where(ph, torch.zeros_like(labels), labels).to(torch.int32)
    dec = torch.where(ph, torch.zeros_like(dec), dec)
    return boxes, scores, labels, dec


def nms_ref(boxes, scores, thresh):
    """Greedy NMS of one list: keep flags (n,) bool.  Descending score, ties by position, NaN first,
    IoU > thresh suppresses (the restatement of test_tracker_gpu.py)."""
    n = boxes.shape[0]
    keep = torch.zeros(n, dtype=torch.bool)
    if not n:
        return keep
    order = torch.sort(scores, descending=True, stable=True)[1]
    a = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    lt = torch.max(boxes[:, None, :2], boxes[:, :2])
    rb = torch.min(boxes[:, None, 2:], boxes[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    iou = inter / (a[:, None] + a - inter)
    supp = torch.zeros(n, dtype=torch.bool)
    for i in order.tolist():
        if not supp[i]:
            keep[i] = True
            supp |= iou[i] > thresh
    return keep


def nms_segments_ref(boxes, scores, idx, offsets, thresh, inf_flag=None):
    """kinet_nms_segments: one keep byte per list entry."""
    keep = torch.zeros(int(offsets[-1]), dtype=torch.uint8)
    for s in range(len(offsets) - 1):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        rows = idx[lo:hi].long()
        sc = scores[rows].clone()
        if inf_flag is not None:
            sc[inf_flag[lo:hi].bool()] = float('inf')
        keep[lo:hi] = nms_ref(boxes[rows], sc, thresh).to(torch.uint8)
    return keep


def commit_ref(bank, hs, boxes, scores, rows, slots):
    """kinet_track_commit by indexing (bank (capacity, d + 5) is changed in place)."""
    d = hs.shape[1]
    bank[slots.long(), :d] = hs[rows.long()]
    bank[slots.long(), d:d + 4] = boxes[rows.long()]
    bank[slots.long(), d + 4] = scores[rows.long()]
    return bank


def gather_ref(bank, slots, offsets, sizes, kmax, Q):
    """kinet_track_gather by indexing: embeds (S, Kmax, d), cxcywh boxes / (w, h, w, h), mask (S, Kmax + Q)."""
    S, d = len(offsets) - 1, bank.shape[1] - 5
    embeds = torch.zeros(S, kmax, d)
    boxes = torch.full((S, kmax, 4), 0.5)
    mask = torch.zeros(S, kmax + Q, dtype=torch.bool)
    for s in range(S):
        rows = slots[int(offsets[s]):int(offsets[s + 1])].long()
        k = len(rows)
        embeds[s, :k] = bank[rows, :d]
        x0, y0, x1, y1 = bank[rows, d:d + 4].unbind(-1)
        h, w = sizes[s]
        boxes[s, :k] = torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0], -1) / torch.stack([w, h, w, h])
        mask[s, k:kmax] = True
    return embeds, boxes, mask


def reid_dist_ref(x, y):
    """Tracker._reid's ||x - y + 1e-6||_2 in f64: x (a, d), y (b, d) -> (a, b)."""
    return (x.double()[:, None, :] - y.double()[None, :, :] + 1e-6).norm(dim=-1)


# ---------------------------------------------------------------------------------- stand-ins for K.*
# Thin adapters with the signatures and return layouts of kinet_amd.kernels' six tracker calls over the
# restatements above, so the three trackers' state machines run on CPU tensors (test_tracker_state_cpu.py).
def nms_adapter(boxes, scores, iou_threshold):
    """K.nms: the kept indices by descending score, ties by index, NaN first."""
    s = scores.float()
    idx = nms_ref(boxes.float(), s, iou_threshold).nonzero().flatten()
    return idx[torch.sort(s[idx], descending=True, stable=True)[1]]


def track_decide_adapter(pred_logits, pred_boxes, sizes, n_active, n_inactive, Kmax, track_thresh, reid_thresh,
                         detection_thresh, clip, out=None):
    """K.track_decide: the packed uint8 buffer K.track_decide_views reads."""
    boxes, scores, labels, dec = decide_ref(pred_logits, pred_boxes, sizes, (n_active + n_inactive).tolist(), Kmax,
                                            track_thresh, reid_thresh, detection_thresh, clip)
    return torch.cat([t.contiguous().view(torch.uint8).flatten() for t in (boxes.float(), scores.float(), labels, dec)])


def nms_segments_adapter(boxes, scores, idx, offsets, total, iou_threshold, inf_flag=None, keep=None):
    assert int(offsets[-1]) == total
    return nms_segments_ref(boxes, scores, idx, offsets, iou_threshold, inf_flag)


def track_commit_adapter(hs_embed, boxes, scores, rows, slots, n, bank):
    commit_ref(bank, hs_embed, boxes, scores, rows[:n], slots[:n])


def track_gather_adapter(bank, slots, offsets, sizes, Kmax, Q):
    return gather_ref(bank, slots, offsets, sizes, Kmax, Q)


def track_reid_dist_adapter(bank, hs_embed, slots, slot_off, rows, row_off, out_off, total):
    d = hs_embed.shape[1]
    out = torch.empty(int(total), dtype=torch.float32)
    for s in range(out_off.numel() - 1):
        a = slots[int(slot_off[s]):int(slot_off[s + 1])].long()
        r = rows[int(row_off[s]):int(row_off[s + 1])].long()
        out[int(out_off[s]):int(out_off[s + 1])] = reid_dist_ref(bank[a, :d], hs_embed[r]).float().flatten()
    return out


KERNEL_ADAPTERS = {'nms': nms_adapter, 'track_decide': track_decide_adapter, 'nms_segments': nms_segments_adapter,
                   'track_commit': track_commit_adapter, 'track_gather': track_gather_adapter,
                   'track_reid_dist': track_reid_dist_adapter}


def small_tracking_model(golden_dir):
    """The small multi-frame Deformable tracking model of test_model_gpu.py's tracking tests (name-seeded
    weights of tests/golden/detr_tracking_mf_small.keys.txt), on the GPU in tracking mode."""
    import os
    from weights import make_state_dict
    from kinet_amd.models import build_model
    from kinet_amd.models.config import load_args
    model, _, _ = build_model(load_args('train_deformable', 'train_multi_frame', 'train_tracking', dataset='mot'))
    shapes = {}
    for ln in open(os.path.join(golden_dir, 'detr_tracking_mf_small.keys.txt')):
        k, *s = ln.split()
        shapes[k] = [int(x) for x in s]
    model.load_state_dict(make_state_dict(shapes, seed=31))
    model = model.cuda().eval()
    model.tracking()
    return model


def run_multi(tracker, det, seeds, frames, retire_at=None):
    """`frames` frames of sequence_blobs(seed) for every seed through `tracker`; retire_at = (i, frame)
    retires sequence i (on the tracker and the fake) before that frame."""
    from fake_detector import sequence_blobs
    blobs = [sequence_blobs(s, frames, device='cuda') for s in seeds]
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
