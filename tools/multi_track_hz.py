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
    a = ap.parse_args()
    if a.windows < 5:
        ap.error('--windows must be at least 5')
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


if __name__ == '__main__':
    main()
