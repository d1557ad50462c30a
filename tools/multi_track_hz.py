#!/usr/bin/env python
"""Tracking throughput of kinet_amd.tracker.MultiTracker (S sequences in lock-step on one batched
detector forward) beside kinet_amd.tracker.Tracker (one sequence at batch 1), measured in the same
process in alternating windows.  Same synthetic set-up as tools/track_hz.py: the config-3 tracking
stack (multi-frame DeformableDETRTracking, d=288, 500 queries), N(0,1) frames, random-init weights, the
class bias calibrated on frame 0 so that --objects queries pass the detection threshold as persons.

Per S it reports frames/s over all sequences (median and min-max of the windows), the batch-S detector
forward (device-synchronised), the device -> host transfers per step and where a step's wall time goes
(waiting in those transfers / everything else on the host).  One JSON line per S, and one for Tracker,
to --out (default profiles/multi_track_hz.jsonl).

    python tools/multi_track_hz.py [--sequences 1,4,8,16] [--windows 5] [--frames 12] [--dtype f16]

--masks: the same comparison with segmentation masks (MOTS): the masks model (train_deformable +
train_tracking + train_mots20) at 800x1333 -> 1080x1920, MultiTracker with tracker_cfg['masks'] at
S = 1 / 4 / 8 beside Tracker with masks, to profiles/multi_mots_hz.jsonl.  Per S additionally the step's split
(batched forward, mask head, segmented resolve -- device events inside the windows --, waiting in
transfers, host, and of the host the construction of the bool masks), and three isolated comparisons
(medians of --reps >= 30, the two sides alternating): (a) DETRSegmBase.mask_logits_rows on the kept rows
of S frames against S mask_logits calls, (b) kinet_segm_track_resolve_segments against S
kinet_segm_track_resolve launches, both with device events, and (c) on the host clock the box-limited
construction of the bool masks against `labels == slot` over the whole map, on the same label maps.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sequences', default='1,4,8,16')
    ap.add_argument('--windows', type=int, default=5, help='timed windows per S (at least 5)')
    ap.add_argument('--frames', type=int, default=12, help='frames per window')
    ap.add_argument('--height', type=int, default=800)
    ap.add_argument('--width', type=int, default=1333)
    ap.add_argument('--objects', type=int, default=40, help='detections above threshold on frame 0')
    ap.add_argument('--dtype', default='f16', choices=['bf16', 'f16', 'f32'])
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'multi_track_hz.jsonl'))
    ap.add_argument('--masks', action='store_true', help='segmentation masks (MOTS): module docstring')
    ap.add_argument('--reps', type=int, default=30, help='--masks: repetitions of the isolated comparisons (>= 30)')
    a = ap.parse_args()
    if a.windows < 5:
        ap.error('--windows must be at least 5')
    if a.masks:
        if a.reps < 30:
            ap.error('--reps must be at least 30')
        return main_masks(a, ap)
    from kinet_amd.models import build_model
    from kinet_amd.models.config import TRACKER_CFG, load_args
    from kinet_amd.tracker import MultiTracker, Tracker
    dev = torch.device('cuda', 0)
    args = load_args('train_deformable', 'train_multi_frame', 'train_tracking', dataset='mot', device='cuda')
    torch.manual_seed(0)
    model, _, post = build_model(args)
    model = model.to(dev)
    model.tracking()
    model.set_compute_dtype({'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}[a.dtype])
    g = torch.Generator(device=dev).manual_seed(7)
    frames = [torch.randn(1, 3, a.height, a.width, generator=g, device=dev) for _ in range(4)]
    size = torch.tensor([[a.height, a.width]], device=dev)
    with torch.no_grad():
        for ce in model.class_embed:
            ce.bias.fill_(-20.0)
            ce.bias[0] = 0.0
        logits = model(frames[0])[0]['pred_logits'][0, :, 0].float()
        thr = math.log(TRACKER_CFG['detection_obj_score_thresh'] / (1 - TRACKER_CFG['detection_obj_score_thresh']))
        b = thr - torch.sort(logits, descending=True)[0][a.objects].item()
        for ce in model.class_embed:
            ce.bias[0] = b
    no_dets = [torch.zeros(0, 4)]

    def blob(s, f):
        return {'img': frames[(s + f) % 4], 'orig_size': size, 'dets': no_dets}

    single = Tracker(model, post, dict(TRACKER_CFG))

    def single_window():
        single.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(a.frames):
            single.step(blob(0, f))
        torch.cuda.synchronize()
        return a.frames / (time.perf_counter() - t0)

    def multi_window(multi, S, stats):
        multi.reset()
        wait = [0.0]
        plain = multi._to_host.__func__

        def timed(t):
            t0 = time.perf_counter()
            r = plain(multi, t)
            wait[0] += time.perf_counter() - t0
            return r
        multi._to_host = timed
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(a.frames):
            stats['queries'].append(sum(len(q.tracks) + len(q.inactive_tracks) for q in multi._seqs) / S)
            multi.step([blob(s, f) for s in range(S)])
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        del multi._to_host
        stats['syncs'].append(multi.sync_count / a.frames)
        stats['step_ms'].append(el / a.frames * 1e3)
        stats['wait_ms'].append(wait[0] / a.frames * 1e3)
        return S * a.frames / el

    def spread(v):
        return {'median': statistics.median(v), 'min': min(v), 'max': max(v)}

    lines, single_hz = [], []
    for S in [int(s) for s in a.sequences.split(',')]:
        multi = MultiTracker(model, post, dict(TRACKER_CFG), S)
        stats = {'queries': [], 'syncs': [], 'step_ms': [], 'wait_ms': []}
        multi_window(multi, S, stats)                  # warm-up: kernel caches, geometry of this batch size
        single_window()
        stats = {'queries': [], 'syncs': [], 'step_ms': [], 'wait_ms': []}
        hz, ref = [], []
        for _ in range(a.windows):
            hz.append(multi_window(multi, S, stats))
            ref.append(single_window())
        single_hz += ref
        # the batch-S detector forward alone at the mean track-query count, device-synchronised per call
        kq = max(1, int(round(sum(stats['queries']) / len(stats['queries']))))
        tgt = [{'track_query_boxes': torch.rand(kq, 4, generator=g, device=dev) * 0.5 + 0.1,
                'track_query_hs_embeds': torch.randn(kq, model.hidden_dim, generator=g, device=dev),
                'track_queries_placeholder_mask': torch.zeros(kq + model.num_queries, dtype=torch.bool, device=dev)}
               for _ in range(S)]
        batch = [frames[s % 4][0] for s in range(S)]
        with torch.no_grad():
            _, _, feats, _, _ = model(batch)
            model(batch, tgt, feats)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                model(batch, tgt, feats)
                torch.cuda.synchronize()
            det_ms = (time.perf_counter() - t0) / 5 * 1e3
        step_ms, wait_ms = statistics.median(stats['step_ms']), statistics.median(stats['wait_ms'])
        lines.append({'metric': 'multi-sequence tracking, frames/s over all sequences', 'S': S, 'unit': 'frames/s',
                      'multi_tracker': spread(hz), 'tracker_same_windows': spread(ref), 'windows': a.windows,
                      'frames_per_window': a.frames, 'mean_track_queries': sum(stats['queries']) / len(stats['queries']),
                      'detector_batch_forward_ms_synced': det_ms, 'sync_count_per_step': statistics.median(stats['syncs']),
                      'step_ms': step_ms, 'transfer_wait_ms_per_step': wait_ms, 'host_ms_per_step': step_ms - wait_ms,
                      'above_tracker_range': min(hz) > max(ref), 'dtype': a.dtype, 'frame': [3, a.height, a.width]})
        print(json.dumps(lines[-1]), flush=True)
        del multi, batch, feats
        torch.cuda.empty_cache()
    lines.append({'metric': 'Tracker, one sequence at batch 1, all windows of this run', 'unit': 'frames/s',
                  'tracker': spread(single_hz), 'windows': len(single_hz), 'frames_per_window': a.frames,
                  'dtype': a.dtype, 'frame': [3, a.height, a.width]})
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        for ln in lines:
            f.write(json.dumps(ln) + '\n')


ORIG_HW = (1080, 1920)


def _events(fns, reps, warmup=3):
    """Median / min / max ms (device events) of each callable, the callables alternating inside one loop."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            e.synchronize()
            ms[i].append(s.elapsed_time(e))
    return [{'median_ms': statistics.median(m), 'min_ms': min(m), 'max_ms': max(m)} for m in ms]


def _host_clock(fns, reps, warmup=2):
    for _ in range(warmup):
        for f in fns:
            f()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, f in enumerate(fns):
            t0 = time.perf_counter()
            f()
            ms[i].append((time.perf_counter() - t0) * 1e3)
    return [{'median_ms': statistics.median(m), 'min_ms': min(m), 'max_ms': max(m)} for m in ms]


def _blob_logits(n, h, w, g, dev):
    """n rows of mask logits shaped like a detector's: one bump per row (radius about a tenth of the frame)
    over a background at -2.5, plus noise."""
    ys = ((torch.arange(h, device=dev) + 0.5) / h).view(1, h, 1)
    xs = ((torch.arange(w, device=dev) + 0.5) / w).view(1, 1, w)
    c = torch.rand(n, 2, generator=g, device=dev) * 0.8 + 0.1
    r = torch.rand(n, 2, generator=g, device=dev) * 0.08 + 0.06
    r2 = ((xs - c[:, 0].view(n, 1, 1)) / r[:, 0].view(n, 1, 1)) ** 2 + ((ys - c[:, 1].view(n, 1, 1)) / r[:, 1].view(n, 1, 1)) ** 2
    return (6.0 * torch.exp(-r2) - 2.5 + 0.3 * torch.randn(n, h, w, generator=g, device=dev)).contiguous()


def main_masks(a, ap):
    import numpy as np
    from kinet_amd import kernels as K
    from kinet_amd.models import build_model
    from kinet_amd.models.config import TRACKER_CFG, load_args
    from kinet_amd.tracker import MultiTracker, Tracker
    default_out = ap.get_default('out')
    out_path = a.out if a.out != default_out else os.path.join(os.path.dirname(default_out), 'multi_mots_hz.jsonl')
    seq_list = [int(s) for s in (a.sequences if a.sequences != ap.get_default('sequences') else '1,4,8').split(',')]
    objects = a.objects if a.objects != ap.get_default('objects') else 20
    dev = torch.device('cuda', 0)
    net_hw = (a.height, a.width)
    args = load_args('train_deformable', 'train_tracking', 'train_mots20', device='cuda')
    torch.manual_seed(0)
    model, _, post = build_model(args)
    model = model.to(dev)
    model.tracking()
    model.set_compute_dtype({'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}[a.dtype])
    g = torch.Generator(device=dev).manual_seed(7)
    frames = [torch.randn(1, 3, *net_hw, generator=g, device=dev) for _ in range(4)]
    model.defer_masks = True
    with torch.no_grad():
        for ce in model.class_embed:
            ce.bias.fill_(-20.0)
            ce.bias[0] = 0.0
        logits = model(frames[0])[0]['pred_logits'][0, :, 0].float()
        thr = math.log(TRACKER_CFG['detection_obj_score_thresh'] / (1 - TRACKER_CFG['detection_obj_score_thresh']))
        b = thr - torch.sort(logits, descending=True)[0][objects].item()
        for ce in model.class_embed:
            ce.bias[0] = b
    model.defer_masks = False
    cfg = dict(TRACKER_CFG, masks=True)
    fixed = {'orig_size': torch.tensor([list(ORIG_HW)]), 'size': torch.tensor([list(net_hw)]), 'dets': [torch.zeros(0, 4)]}

    def blob(s, f):
        return dict(fixed, img=frames[(s + f) % 4])

    single = Tracker(model, post, cfg)

    def single_window():
        single.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(a.frames):
            single.step(blob(0, f))
        torch.cuda.synchronize()
        return a.frames / (time.perf_counter() - t0)

    def spread(v):
        return {'median': statistics.median(v), 'min': min(v), 'max': max(v)}

    def multi_window(multi, S, stats):
        multi.reset()
        wait, pairs = [0.0], {'head': [], 'resolve': []}
        plain = multi._to_host.__func__

        def timed(t):
            t0 = time.perf_counter()
            r = plain(multi, t)
            wait[0] += time.perf_counter() - t0
            return r

        def evented(fn, key):
            def f(*args, **kw):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                r = fn(*args, **kw)
                e.record()
                pairs[key].append((s, e))
                return r
            return f
        multi._to_host = timed
        head, resolve = model.mask_logits_rows, K.segm_track_resolve_segments
        model.mask_logits_rows = evented(head, 'head')
        K.segm_track_resolve_segments = evented(resolve, 'resolve')
        try:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for f in range(a.frames):
                stats['tracks'].append(sum(len(q.tracks) for q in multi._seqs) / S)
                multi.step([blob(s, f) for s in range(S)])
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
        finally:
            del multi._to_host, model.mask_logits_rows
            K.segm_track_resolve_segments = resolve
        stats['syncs'].append(multi.sync_count / a.frames)
        stats['step_ms'].append(el / a.frames * 1e3)
        stats['wait_ms'].append(wait[0] / a.frames * 1e3)
        stats['mask_ms'].append(multi.mask_seconds / a.frames * 1e3)
        for key in pairs:
            stats[key + '_ms'].append(sum(s.elapsed_time(e) for s, e in pairs[key]) / a.frames)
        return S * a.frames / el

    def fresh():
        return {k: [] for k in ('tracks', 'syncs', 'step_ms', 'wait_ms', 'mask_ms', 'head_ms', 'resolve_ms')}

    lines, single_hz = [], []
    h4, w4 = None, None
    for S in seq_list:
        multi = MultiTracker(model, post, cfg, S)
        multi_window(multi, S, fresh())                # warm-up
        single_window()
        stats = fresh()
        hz, ref = [], []
        for _ in range(a.windows):
            hz.append(multi_window(multi, S, stats))
            ref.append(single_window())
        single_hz += ref
        med = {k: statistics.median(v) for k, v in stats.items()}
        kq = max(1, int(round(sum(stats['tracks']) / len(stats['tracks']))))
        tgt = [{'track_query_boxes': torch.rand(kq, 4, generator=g, device=dev) * 0.5 + 0.1,
                'track_query_hs_embeds': torch.randn(kq, model.hidden_dim, generator=g, device=dev),
                'track_queries_placeholder_mask': torch.zeros(kq + model.num_queries, dtype=torch.bool, device=dev)}
               for _ in range(S)]
        batch = [frames[s % 4][0] for s in range(S)]
        with torch.no_grad():
            model.defer_masks = True
            model(batch, tgt)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                model(batch, tgt)
                torch.cuda.synchronize()
            det_ms = (time.perf_counter() - t0) / 5 * 1e3
            # (a) the head on kq kept rows per frame: one ragged pass against S per-frame passes (the
            # per-frame operands are computed once per forward on both sides and are not part of either)
            rows = torch.cat([torch.randperm(kq + model.num_queries, generator=g, device=dev)[:kq] for _ in range(S)])
            frs = torch.arange(S, device=dev, dtype=torch.int32).repeat_interleave(kq)
            model.mask_logits(rows[:1], 0)
            per = [rows[frs == bb] for bb in range(S)]
            same = bool(torch.equal(model.mask_logits_rows(rows, frs),
                                    torch.cat([model.mask_logits(per[bb], bb) for bb in range(S)])))
            head_one, head_loop = _events([lambda: model.mask_logits_rows(rows, frs),
                                           lambda: [model.mask_logits(per[bb], bb) for bb in range(S)]], a.reps)
            h4, w4 = model._mask_ctx['fpns'][2].shape[1:3]
            model.defer_masks = False
        # (b) the resolve of kq slots per sequence: one segmented launch against S single launches
        lg = _blob_logits(S * kq, h4, w4, g, dev)
        src = torch.arange(S * kq, dtype=torch.int32, device=dev)
        src_off = [bb * kq for bb in range(S + 1)]
        geom = [net_hw + ORIG_HW] * S
        outs = [torch.empty(ORIG_HW, dtype=torch.int16, device=dev) for _ in range(S)]
        src1 = torch.arange(kq, dtype=torch.int32, device=dev)
        packed = torch.empty(20 * S * kq + 2 * S * ORIG_HW[0] * ORIG_HW[1] + 4, dtype=torch.uint8, device=dev)

        def seg():
            return K.segm_track_resolve_segments(lg, src, src_off, geom, None, None, net_hw, 0.5, out=packed)

        def singles():
            for bb in range(S):
                K.segm_track_resolve(lg[bb * kq:(bb + 1) * kq], src1, None, net_hw, net_hw, ORIG_HW, 0.5, out=outs[bb])
        buf, _, lab_d, pix_off = seg()
        singles()
        same_labels = all(bool(torch.equal(lab_d[pix_off[bb]:pix_off[bb + 1]].view(ORIG_HW), outs[bb])) for bb in range(S))
        res_one, res_loop = _events([seg, singles], a.reps)
        # (c) the host's bool masks from the same label maps: inside each slot's box against the whole map
        st, lab = K.segm_resolve_views(buf.cpu().numpy(), S * kq, int(pix_off[-1]))
        maps = [lab[pix_off[bb]:pix_off[bb + 1]].reshape(ORIG_HW) for bb in range(S)]

        def boxed():
            out = []
            for bb in range(S):
                for t in range(kq):
                    n, x0, y0, x1, y1 = (int(v) for v in st[bb * kq + t])
                    m = np.zeros(ORIG_HW, np.bool_)
                    if n:
                        m[y0:y1, x0:x1] = maps[bb][y0:y1, x0:x1] == t
                    out.append(m)
            return out

        def whole():
            return [maps[bb] == t for bb in range(S) for t in range(kq)]
        same_masks = all(np.array_equal(x, y) for x, y in zip(boxed(), whole()))
        host_box, host_whole = _host_clock([boxed, whole], a.reps)
        lines.append({'metric': 'multi-sequence tracking with masks (MOTS), frames/s over all sequences', 'S': S,
                      'unit': 'frames/s', 'multi_tracker': spread(hz), 'tracker_same_windows': spread(ref),
                      'windows': a.windows, 'frames_per_window': a.frames,
                      'mean_tracks_alive': sum(stats['tracks']) / len(stats['tracks']),
                      'sync_count_per_step': med['syncs'], 'step_ms': med['step_ms'],
                      'detector_batch_forward_ms_synced': det_ms, 'mask_head_ms_per_step': med['head_ms'],
                      'resolve_ms_per_step': med['resolve_ms'], 'transfer_wait_ms_per_step': med['wait_ms'],
                      'host_ms_per_step': med['step_ms'] - med['wait_ms'], 'host_mask_build_ms_per_step': med['mask_ms'],
                      'above_tracker_range': min(hz) > max(ref), 'dtype': a.dtype, 'frame': [3, *net_hw],
                      'orig': list(ORIG_HW)})
        print(json.dumps(lines[-1]), flush=True)
        lines.append({'metric': 'isolated comparisons at S sequences of n rows / slots each', 'S': S, 'n': kq,
                      'reps': a.reps, 'unit': 'ms',
                      'head_rows_one_pass': head_one, 'head_loop_of_S_mask_logits': head_loop, 'head_equal': same,
                      'resolve_segments': res_one, 'resolve_S_single_launches': res_loop, 'resolve_equal': same_labels,
                      'host_masks_inside_boxes': host_box, 'host_masks_whole_map': host_whole, 'host_equal': same_masks,
                      'dtype': a.dtype, 'frame': [3, *net_hw], 'orig': list(ORIG_HW)})
        print(json.dumps(lines[-1]), flush=True)
        del multi, batch, lg, packed, outs, buf, lab_d
        torch.cuda.empty_cache()
    lines.append({'metric': 'Tracker with masks, one sequence at batch 1, all windows of this run', 'unit': 'frames/s',
                  'tracker': spread(single_hz), 'windows': len(single_hz), 'frames_per_window': a.frames,
                  'dtype': a.dtype, 'frame': [3, *net_hw], 'orig': list(ORIG_HW)})
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        for ln in lines:
            f.write(json.dumps(ln) + '\n')


if __name__ == '__main__':
    main()
