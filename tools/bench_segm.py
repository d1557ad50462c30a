"""Device time of the segmentation head (kinet_amd/models/segmentation.py on csrc/segm.hip) alone at
config-2 size: one 800x1333 frame (layer shapes 200x334, 100x167, 50x84, 25x42), 300 queries, batch 1,
bf16.  The head's inputs (level-1 src, decoder output, memory level, backbone features) come from one
forward of the masks model with seeded weights.

One JSON line with, in milliseconds per frame (median of `--repeats` windows of `--iters` calls
between HIP events, after a warm-up; min / max alongside; the variants alternate window by window):
  attention   q_linear + k_linear + the joint-softmax attention map
  head        the shipped head: lay1 as one f32 convolution per frame + the 8-channel per-query kernel,
              GroupNorm + ReLU (+ nearest upsample + FPN add) in one entry point, the direct out_lay
  plain       the same head composed from the ops the library had before csrc/segm.hip: concatenate
              [src | attention] per query, a full 264 -> 264 kinet_conv2d, kinet_groupnorm, then ReLU,
              nearest upsampling (index_select) and the FPN add as torch element-wise ops, out_lay as a
              kinet_conv2d with its one output channel padded to 8
  detector    the whole one-stage detector forward without masks (train_deformable.yaml, ResNet-50)
  segm        the whole masks model forward (detector + attention + head)
and `head_share_of_detector` = head / detector, `plain_over_head`, and the two heads' max |diff|.

usage: python tools/bench_segm.py [--queries 300] [--iters N] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kinet_amd import kernels as K  # noqa: E402


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters   # ms per call


def timed(fns, iters, repeats):
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window(fn, iters))
    return {k: [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)] for k, v in t.items()}


def nearest_idx(n_in, n_out, device):
    scale = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_out, dtype=torch.float32)
    return torch.floor(torch.arange(n_out, dtype=torch.float32) * scale).long().clamp(max=n_in - 1).to(device)


def plain_head(head, src, att, fpns, Q, chunk):
    """The head from the library's older ops (module docstring); same chunking as the shipped head."""
    dt = att.dtype
    adapted = head.adapters(fpns)
    R = att.shape[0]
    H, W = adapted[2].shape[1:3]
    out = torch.empty((R, H, W), dtype=torch.float32, device=att.device)
    w_out = K.cached(head.out_lay.weight, ('bench_out8', dt), lambda t: torch.nn.functional.pad(
        t.detach().permute(0, 2, 3, 1), (0, 0, 0, 0, 0, 0, 0, 7)).to(dt).contiguous())
    b_out = K.cached(head.out_lay.bias, 'bench_out8_bias', lambda t: torch.nn.functional.pad(t.detach().float(), (0, 7)))

    def gn(x, m):
        n, h, w, C = x.shape
        return torch.relu_(K.groupnorm_nhwc(x.view(n, h * w, C), m.weight, m.bias, m.num_groups, m.eps)).view(n, h, w, C)

    def up_add(x, f, r0):
        b = r0 // Q      # batch 1 in this tool: every row belongs to frame 0
        iy, ix = nearest_idx(x.shape[1], f.shape[1], x.device), nearest_idx(x.shape[2], f.shape[2], x.device)
        return x.index_select(1, iy).index_select(2, ix).add_(f[b:b + 1])
    for r0 in range(0, R, chunk):
        r1 = min(R, r0 + chunk)
        x = torch.cat([src[r0 // Q:r0 // Q + 1].expand(r1 - r0, -1, -1, -1), att[r0:r1]], -1)
        x = gn(head._conv(x, head.lay1), head.gn1)
        x = up_add(gn(head._conv(x, head.lay2), head.gn2), adapted[0], r0)
        x = up_add(gn(head._conv(x, head.lay3), head.gn3), adapted[1], r0)
        x = up_add(gn(head._conv(x, head.lay4), head.gn4), adapted[2], r0)
        x = gn(head._conv(x, head.lay5), head.gn5)
        y = K.conv2d_nhwc(x, w_out, 1, 1, bias=b_out, ksplit=1)
        out[r0:r1] = y[..., 0].float()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--queries', type=int, default=300)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None, help='append the JSON line to this file as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_segm: needs a GPU')
    from kinet_amd.models import build_model
    from kinet_amd.models.config import load_args
    from kinet_amd.models.segmentation import MASK_WORKSPACE_BYTES
    torch.manual_seed(0)
    dt = torch.bfloat16
    segm = build_model(load_args('train_deformable', masks=True, num_queries=a.queries))[0].cuda().eval().set_compute_dtype(dt)
    det = build_model(load_args('train_deformable', num_queries=a.queries))[0].cuda().eval().set_compute_dtype(dt)
    frames = [torch.randn(3, 800, 1333, generator=torch.Generator().manual_seed(1)).cuda()]
    head, cap = segm.mask_head, {}
    orig = head.forward

    def grab(src, att, fpns, Q, chunk=None):
        cap.update(src=src, att=att, fpns=fpns, Q=Q)
        return orig(src, att, fpns, Q, chunk)
    with torch.no_grad():
        head.forward = grab
        _, _, _, memory, hs = segm(frames)
        head.forward = orig
        src, att, fpns, Q = cap['src'].contiguous(), cap['att'], cap['fpns'], cap['Q']
        H, W = fpns[2].shape[1:3]
        chunk = max(1, MASK_WORKSPACE_BYTES // (H * W * (2 * 32 + 16) * att.element_size()))
        k_rows = memory.flatten(2).permute(0, 2, 1).contiguous()
        mask = torch.zeros(1, k_rows.shape[1], dtype=torch.bool, device='cuda')
        a_head, a_plain = head(src, att, fpns, Q, chunk), plain_head(head, src, att, fpns, Q, chunk)
        diff = (a_head - a_plain).abs().max().item()
        r = timed({'attention': lambda: segm.bbox_attention(hs[-1], k_rows, mask),
                   'head': lambda: head(src, att, fpns, Q, chunk),
                   'plain': lambda: plain_head(head, src, att, fpns, Q, chunk),
                   'detector': lambda: det(frames),
                   'segm': lambda: segm(frames)}, a.iters, a.repeats)
    line = json.dumps({'what': 'segm_head', 'frame': [800, 1333], 'queries': Q, 'batch': 1, 'dtype': 'bfloat16',
                       'map': [int(src.shape[1]), int(src.shape[2])], 'out': [int(H), int(W)], 'rows_per_chunk': chunk,
                       'ms_median_min_max': r, 'head_share_of_detector': round(r['head'][0] / r['detector'][0], 3),
                       'plain_over_head': round(r['plain'][0] / r['head'][0], 3),
                       'head_vs_plain_max_abs_diff': round(diff, 4), 'logit_abs_max': round(a_head.abs().max().item(), 3),
                       'iters': a.iters, 'repeats': a.repeats})
    print(line, flush=True)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
