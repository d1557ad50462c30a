"""Device time of mask training (kinet_amd/models/segmentation.py, csrc/segm_train.hip) at the real
workload's sizes.  Two JSON lines, times in milliseconds as [median, min, max] of `--repeats` windows
of `--iters` calls between HIP events after a warm-up, the variants alternating window by window:

  segm_mask_loss      the fused mask loss, forward + backward, logits n x 200 x 334 against targets
                      n x 800 x 1333 (n = 8 and 32), next to the torch composition the reference runs
                      (F.interpolate bilinear -> sigmoid_focal_loss + dice_loss -> autograd) on the same
                      device in the same process.  `hbm_frac` is the compulsory traffic over the time over
                      the HBM peak: the target read once per pass (forward, backward) and the logits read
                      once forward, read and their gradient written backward.
  segm_train_head     the training head of one step, B = 2 frames of 800 x 1333, Q = 300 queries, 8
                      matched rows per frame: `forward` is the inference head over all 600 rows (no graph
                      kept), `backward` the recompute + backward on the 16 matched rows; `all_rows` is the
                      backward differentiating every row, at the largest Q per frame of --all-rows-q that
                      runs (named in the line, with the error that stopped the next one).

usage: python tools/bench_segm_train.py [--iters N] [--repeats R] [--out FILE] [--skip-head]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kinet_amd import autograd as A  # noqa: E402
from kinet_amd.train import HBM_PEAK_GBS  # noqa: E402


def windows(fns, iters, repeats, timed_part=None):
    """{name: [median, min, max]} ms per call.  timed_part[name](state) is the timed call, fns[name]() its
    untimed preparation returning `state`; without timed_part the whole fns[name]() is timed."""
    for k, fn in fns.items():
        s = fn()
        if timed_part:
            timed_part[k](s)
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            total = 0.0
            for _ in range(iters):
                state = fn() if timed_part else None
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                timed_part[k](state) if timed_part else fn()
                e.record()
                torch.cuda.synchronize()
                total += s.elapsed_time(e)
            t[k].append(total / iters)
    return {k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in t.items()}


def torch_mask_losses(logits, target, num_boxes):
    """detr.py:779-790 / util/misc.py:616-665 as the reference composes them."""
    from kinet_amd.models.criterion import sigmoid_focal_loss
    src = F.interpolate(logits[:, None], size=target.shape[-2:], mode='bilinear', align_corners=False)[:, 0].flatten(1)
    tgt = target.flatten(1).to(src)
    p = src.sigmoid()
    dice = 1 - (2 * (p * tgt).sum(1) + 1) / (p.sum(-1) + tgt.sum(-1) + 1)
    return sigmoid_focal_loss(src, tgt, num_boxes), dice.sum() / num_boxes


def bench_loss(n, iters, repeats):
    g = torch.Generator().manual_seed(n)
    h, w, H, W = 200, 334, 800, 1333
    logits = (torch.randn(n, h, w, generator=g) * 3).cuda().requires_grad_(True)
    ys = (torch.arange(H).view(1, -1, 1) + 0.5) / H
    xs = (torch.arange(W).view(1, 1, -1) + 0.5) / W
    c = torch.rand(n, 2, generator=g) * 0.6 + 0.2
    target = (((ys - c[:, :1, None]) / 0.15) ** 2 + ((xs - c[:, 1:, None]) / 0.1) ** 2 <= 1).to(torch.uint8).cuda()

    def run(fn):
        logits.grad = None
        lm, ld = fn(logits, target, float(n))
        (lm + ld).backward()
        return lm.detach(), ld.detach(), logits.grad

    def fwd_only(fn):
        with torch.no_grad():
            return fn(logits, target, float(n))
    fused, plain = run(A.segm_mask_loss), run(torch_mask_losses)
    diff = {'loss_mask': abs(fused[0] - plain[0]).item(), 'loss_dice': abs(fused[1] - plain[1]).item(),
            'dlogits_max_abs': (fused[2] - plain[2]).abs().max().item(), 'dlogits_peak': plain[2].abs().max().item()}
    r = windows({'fused_fwd_bwd': lambda: run(A.segm_mask_loss), 'torch_fwd_bwd': lambda: run(torch_mask_losses),
                 'fused_fwd': lambda: fwd_only(A.segm_mask_loss), 'torch_fwd': lambda: fwd_only(torch_mask_losses)},
                iters, repeats)
    bytes_fwd = n * H * W + 4 * n * h * w
    bytes_bwd = n * H * W + 8 * n * h * w
    fwd_ms, both_ms = r['fused_fwd'][0], r['fused_fwd_bwd'][0]
    return {'what': 'segm_mask_loss', 'n': n, 'logits': [h, w], 'target': [H, W], 'ms_median_min_max': r,
            'torch_over_fused_fwd_bwd': round(r['torch_fwd_bwd'][0] / both_ms, 2),
            'compulsory_bytes': {'forward': bytes_fwd, 'backward': bytes_bwd},
            'hbm_frac': {'forward': round(bytes_fwd / (fwd_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                         'forward_backward': round((bytes_fwd + bytes_bwd) / (both_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
            'hbm_peak_gbs': HBM_PEAK_GBS, 'backward_form': 'gather per low-resolution pixel (the only form built)',
            'fused_vs_torch': diff, 'iters': iters, 'repeats': repeats}


def bench_head(iters, repeats, matched, all_rows_q):
    from kinet_amd.models import segmentation as S
    from kinet_amd.models.config import load_args
    from kinet_amd.train import build_mask_training
    torch.manual_seed(0)
    torch.set_float32_matmul_precision('high')      # the training benchmark's setting (kinet_amd.train.benchmark_train)
    B, Q = 2, 300
    args = load_args('train_deformable', masks=True, num_queries=Q, dropout=0.0, freeze_detr=True, device='cuda')
    model = build_mask_training(args)[0].cuda().train()
    frames = [torch.randn(3, 800, 1333, generator=torch.Generator().manual_seed(1 + b)).cuda() for b in range(B)]
    cap, orig = {}, S._MaskHeadTrain.apply

    def grab(*a):
        cap['args'] = a
        return orig(*a)
    S._MaskHeadTrain.apply = grab
    try:
        out = model(frames)[0]
    finally:
        S._MaskHeadTrain.apply = orig
    mask = cap['args'][1]
    tensors = [t.detach() for t in cap['args'][2:2 + S._MaskHeadTrain.N_IN]]
    params = list(cap['args'][2 + S._MaskHeadTrain.N_IN:])
    shape = tuple(out['pred_masks'].shape)
    del out

    def forward(q=Q):
        ins = [tensors[0][:, :q].contiguous()] + tensors[1:]
        return orig(model, mask, *ins, *params)

    def dseg(q, rows):
        g = torch.zeros((B, q) + shape[2:], device='cuda')
        g[:, :rows] = torch.randn((B, rows) + shape[2:], generator=torch.Generator().manual_seed(7)).cuda() * 1e-3
        return g
    d_matched = dseg(Q, matched)
    with torch.no_grad():
        r_fwd = windows({'forward': forward}, iters, repeats)
    r_bwd = windows({'backward': forward}, iters, repeats, {'backward': lambda o: o.backward(d_matched)})
    assert model.last_mask_rows == [list(range(matched))] * B
    line = {'what': 'segm_train_head', 'frames': [B, 800, 1333], 'queries': Q, 'matched_rows_per_frame': matched,
            'logits': list(shape[2:]), 'dtype': 'float32', 'f32_matmul_precision': torch.get_float32_matmul_precision(),
            'ms_median_min_max': dict(r_fwd, **r_bwd), 'iters': iters, 'repeats': repeats}
    model.mask_train_all_rows = True
    for q in all_rows_q:
        try:
            d_all = dseg(q, q)
            r = windows({'all_rows': lambda: forward(q)}, 1, 2, {'all_rows': lambda o: o.backward(d_all)})
            line['all_rows'] = {'queries_per_frame': q, 'rows': B * q, 'backward_ms_median_min_max': r['all_rows'],
                                'peak_memory_gib': round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}
        except RuntimeError as e:       # out of memory, or an operand beyond kinet_conv2d's 2 GiB limit
            line['all_rows_refused_at_q'] = {'queries_per_frame': q, 'error': str(e)[:160]}
            break
        finally:
            d_all = None
            torch.cuda.empty_cache()
    model.mask_train_all_rows = False
    if 'all_rows' in line:
        a = line['all_rows']
        line['all_rows_ms_per_row_over_matched_ms_per_row'] = round(
            (a['backward_ms_median_min_max'][0] / a['rows']) / (r_bwd['backward'][0] / (B * matched)), 2)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--matched', type=int, default=8)
    ap.add_argument('--all-rows-q', type=int, nargs='*', default=[16, 64])
    ap.add_argument('--skip-head', action='store_true')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_segm_train: needs a GPU')
    lines = [bench_loss(n, a.iters, a.repeats) for n in (8, 32)]
    if not a.skip_head:
        lines.append(bench_head(a.iters, a.repeats, a.matched, a.all_rows_q))
    for ln in lines:
        s = json.dumps(ln)
        print(s, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(s + '\n')


if __name__ == '__main__':
    main()
