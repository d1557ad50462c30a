"""Device time of the two-stage proposal stage (csrc/two_stage.hip, DeformableTransformer.
_proposal_queries) at config-2 geometry: one 800x1333 frame = level shapes 100x167, 50x84, 25x42,
13x21, S = 22 223 tokens, 300 proposals, 91 class logits, bf16, batch 1 / 16 / 28.

Per batch size one JSON line with, in microseconds per call (median of `--repeats` windows of
`--iters` calls between HIP events, after a warm-up; min / max of the windows alongside):
  proposals      kinet_two_stage_proposals (once per geometry in the model: cached)
  topk           kinet_topk_rows on channel 0 of the (B, S, 91) f32 logits, read in place
  torch_topk     torch.topk on the same strided view (its result is compared first: the same set
                 per row; torch's order among equal scores is unspecified)
  queries        kinet_two_stage_queries
  fill_rows      kinet_two_stage_fill_rows
  boxes          kinet_two_stage_boxes
  stage          the whole proposal stage: enc_output GEMM + LayerNorm, constant-row fill, class
                 GEMM, box MLP, boxes, top-k, queries, pos_trans GEMM + LayerNorm, the two splits
  decoder        the 6-layer decoder the stage feeds (300 queries, box refinement)
Then one line per batch size in `--e2e` with the whole detector forward, two-stage against the
one-stage model (train_deformable.yaml, ResNet-50, 300 queries), alternating the two.

usage: python tools/bench_two_stage.py [--batches 1,16,28] [--e2e 1,16] [--iters N] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kinet_amd import kernels as K  # noqa: E402

SHAPES = [(100, 167), (50, 84), (25, 42), (13, 21)]
S = sum(h * w for h, w in SHAPES)
K_PROP, N_CLS, D = 300, 91, 256


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3   # us per call


def timed(fns, iters, repeats):
    """{name: fn} -> {name: [median, min, max]} us; the variants alternate window by window."""
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window(fn, iters))
    return {k: [round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)] for k, v in t.items()}


def build_transformer():
    from kinet_amd.models.deformable_detr import MLP
    from kinet_amd.models.deformable_transformer import DeformableTransformer
    torch.manual_seed(0)
    t = DeformableTransformer(d_model=D, return_intermediate_dec=True, two_stage=True, two_stage_num_proposals=K_PROP)
    t.decoder.class_embed = nn.ModuleList(nn.Linear(D, N_CLS) for _ in range(7))
    t.decoder.bbox_embed = nn.ModuleList(MLP(D, D, 4, 3) for _ in range(7))
    return t.cuda().eval()


def bench_stage(t, B, iters, repeats):
    dev = torch.device('cuda')
    g = torch.Generator(device='cuda').manual_seed(B)
    memory = torch.randn(B, S, D, device=dev, generator=g).to(torch.bfloat16)
    vr = torch.ones(B, len(SHAPES), 2, device=dev)
    with torch.no_grad():
        geo = t.geometry(SHAPES, vr, None, dev, padded=False)
        qpos, tgt, ref, cls, unact = t._proposal_queries(memory, geo)
        scores = cls[..., 0]
        idx = t.topk_proposals
        same = all(set(a.tolist()) == set(b.tolist()) for a, b in zip(idx, torch.topk(scores, K_PROP, dim=1)[1]))
        om = torch.randn(B, S, D, device=dev, generator=g).to(torch.bfloat16)
        row = t._invalid_row(torch.bfloat16)
        tmp = torch.randn(B, S, 4, device=dev, generator=g)
        fns = {
            'proposals': lambda: K.two_stage_proposals(SHAPES, None, B, dev),
            'topk': lambda: K.topk_rows(scores, K_PROP),
            'torch_topk': lambda: torch.topk(scores, K_PROP, dim=1),
            'queries': lambda: K.two_stage_queries(unact, idx, torch.bfloat16),
            'fill_rows': lambda: K.two_stage_fill_rows(om, geo['keep'], row),
            'boxes': lambda: K.two_stage_boxes(tmp, geo['proposals']),
            'stage': lambda: t._proposal_queries(memory, geo),
            'decoder': lambda: t.decoder(tgt, ref, memory, geo['spatial_shapes'], vr, qpos, None, None),
        }
        r = timed(fns, iters, repeats)
    return {'what': 'proposal_stage', 'B': B, 'S': S, 'k': K_PROP, 'n_cls': N_CLS, 'dtype': 'bfloat16',
            'us_median_min_max': r, 'topk_set_equals_torch': same,
            'topk_vs_torch_speedup': round(r['torch_topk'][0] / r['topk'][0], 2),
            'stage_over_decoder': round(r['stage'][0] / r['decoder'][0], 3), 'iters': iters, 'repeats': repeats}


def bench_e2e(B, iters, repeats):
    from kinet_amd.models import build_model
    from kinet_amd.models.config import load_args
    torch.manual_seed(0)
    two = build_model(load_args('train_deformable', two_stage=True))[0].cuda().eval().set_compute_dtype(torch.bfloat16)
    one = build_model(load_args('train_deformable'))[0].cuda().eval().set_compute_dtype(torch.bfloat16)
    x = torch.randn(B, 3, 800, 1333, generator=torch.Generator().manual_seed(1)).cuda()
    frames = list(x)
    with torch.no_grad():
        r = timed({'two_stage': lambda: two(frames), 'one_stage': lambda: one(frames)}, iters, repeats)
    return {'what': 'detector_forward', 'B': B, 'frame': [800, 1333], 'queries': K_PROP, 'dtype': 'bfloat16',
            'us_median_min_max': r, 'two_over_one': round(r['two_stage'][0] / r['one_stage'][0], 3),
            'iters': iters, 'repeats': repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,16,28')
    ap.add_argument('--e2e', default='1,16')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_two_stage: needs a GPU')

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    t = build_transformer()
    for B in [int(b) for b in a.batches.split(',') if b]:
        emit(bench_stage(t, B, a.iters, a.repeats))
    del t
    for B in [int(b) for b in a.e2e.split(',') if b]:
        emit(bench_e2e(B, max(3, a.iters // 4), a.repeats))


if __name__ == '__main__':
    main()
