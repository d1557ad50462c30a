"""Device time of vanilla DETR (config 1) training: the f32 attention training pair of csrc/attn_train.hip
(kernels.mha_train_forward / mha_train_backward) next to the pair it replaces on the dense layers
(kernels.mha_core in f32 + kernels.mha_backward), and one training step with either.  JSON lines; times as
[median, min, max] of `--repeats` windows of `--iters` calls between HIP events after a warm-up, the variants
alternating window by window; peak bytes are torch's allocator peak above what was allocated before the call.

  attn_ab      forward + backward of both pairs, H = 8, D = 32, at B = 2: 1050x1050, 100x1050, 100x100 and
               B = 8: 2100x2100, each at p = 0 and p = 0.1; microseconds, peak bytes, and the largest
               difference between the two pairs' results (same seed, same dropout mask)
  train_step   kinet_amd.train.train_step of cfgs/train.yaml (R-50, 6 + 6 layers, dropout 0.1) on 2 frames of
               3x800x1333, with the dense layers on the new pair and with `dense_attn` off (the older pair);
               ms per step and frames/s
  --profile-steps N   runs N such steps and nothing else: the program to put after `rocprofv3 --kernel-trace
               --stats ... --` (a run of its own); --dense 0 profiles the older pair
  --kernel-stats CSV  reads that run's kernel_stats CSV and emits the share of kernel time spent in the
               attention kernels (no GPU needed)

usage: python tools/bench_detr_train.py [--iters N] [--repeats R] [--steps K] [--out FILE]
"""
import argparse
import csv
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H_IMG, W_IMG, B_IMG = 800, 1333, 2
HEADS, D = 8, 32
AB_SHAPES = ((2, 1050, 1050), (2, 100, 1050), (2, 100, 100), (8, 2100, 2100))
# the kernels of either pair by name (csrc/attn_train.hip; csrc/ops.hip mha_kernel, csrc/grad.hip attn_bwd_*)
ATTN_KERNELS = ('mha_train_fwd_kernel', 'mha_train_dq_kernel', 'mha_train_dkv_kernel', 'mha_kernel', 'attn_bwd_q2_kernel',
                'attn_bwd_kv2_kernel')


def windows(fns, iters, repeats):
    """{name: [median, min, max]} microseconds per call, the variants alternating window by window."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            t[k].append(s.elapsed_time(e) * 1e3 / iters)
    return {k: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)] for k, v in t.items()}


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def attn_ab(emit, iters, repeats):
    from kinet_amd import kernels as K
    scale = D ** -0.5
    for B, Lq, Lk in AB_SHAPES:
        g = torch.Generator().manual_seed(Lq * 7 + Lk)
        q, do = (torch.randn(B, Lq, HEADS * D, generator=g).cuda() for _ in range(2))
        k, v = (torch.randn(B, Lk, HEADS * D, generator=g).cuda() for _ in range(2))
        km = torch.zeros(B, Lk, dtype=torch.uint8, device='cuda')
        km[1:, Lk - Lk // 6:] = 1                          # padded keys on every frame but the first
        seed = torch.tensor([20260101], dtype=torch.int64, device='cuda')
        for p in (0.0, 0.1):
            def new():
                o, lse = K.mha_train_forward(q, k, v, HEADS, scale, km, dropout_p=p, seed=seed)
                return (o,) + tuple(K.mha_train_backward(q, k, v, o, do, lse, HEADS, scale, km, dropout_p=p, seed=seed))

            def old():
                o = K.mha_core(q, k, v, HEADS, scale, km, dropout_p=p, seed=seed)
                return (o,) + tuple(K.mha_backward(q, k, v, do, HEADS, scale, km, dropout_p=p, seed=seed))
            diff = max((a - b).abs().max().item() for a, b in zip(new(), old()))
            it = max(2, iters // 8) if Lq * Lk * B > 4e6 else iters
            r = windows({'new': new, 'old': old}, it, repeats)
            flops = 14.0 * B * HEADS * Lq * Lk * D                # 4 forward + 10 backward, as counted by the wrappers
            emit({'what': 'attn_ab', 'batch': B, 'heads': HEADS, 'head_dim': D, 'Lq': Lq, 'Lk': Lk, 'dropout': p,
                  'us_median_min_max': r, 'old_over_new': round(r['old'][0] / r['new'][0], 2),
                  'ranges_overlap': not (r['new'][2] < r['old'][1] or r['old'][2] < r['new'][1]),
                  'new_tflops': round(flops / r['new'][0] * 1e-6, 2),
                  'peak_bytes': {'new': peak_bytes(new), 'old': peak_bytes(old)}, 'new_vs_old_max_abs': diff,
                  'iters': it, 'repeats': repeats})


def build_step(dense):
    from kinet_amd.models import build_model
    from kinet_amd.models.config import load_args
    from kinet_amd.train import build_optimizer, synthetic_mot_batch, train_step
    args = load_args(device='cuda')
    torch.manual_seed(0)
    model, criterion, _ = build_model(args)
    model = model.cuda().train()
    for layer in list(model.transformer.encoder.layers) + list(model.transformer.decoder.layers):
        layer.dense_attn = bool(dense)
    opt = build_optimizer(model, args)
    samples, targets = synthetic_mot_batch(B_IMG, H_IMG, W_IMG, torch.device('cuda'), torch.Generator().manual_seed(1000))
    targets = [{k: t[k] for k in ('boxes', 'labels')} for t in targets]
    criterion = criterion.cuda()

    def step():
        return train_step(model, criterion, opt, samples, [dict(t) for t in targets], args.clip_max_norm)[0]
    return step


def train_steps(emit, steps):
    fns = {'new_pair': build_step(True), 'old_pair': build_step(False)}
    for fn in fns.values():
        fn()                                              # (windows() warms each once more)
    r = windows(fns, 1, steps)
    ms = {k: [round(x / 1e3, 2) for x in v] for k, v in r.items()}
    emit({'what': 'train_step', 'config': 'cfgs/train.yaml (vanilla DETR, R-50, 6 + 6 layers, 100 queries, dropout 0.1)',
          'frames': [B_IMG, H_IMG, W_IMG], 'ms_median_min_max': ms,
          'frames_per_s': {k: round(B_IMG / (v[0] * 1e-3), 2) for k, v in ms.items()},
          'old_over_new': round(ms['old_pair'][0] / ms['new_pair'][0], 3),
          'ranges_overlap': not (ms['new_pair'][2] < ms['old_pair'][1] or ms['old_pair'][2] < ms['new_pair'][1]),
          'loss': {k: float(fn()) for k, fn in fns.items()}, 'steps': steps})


def kernel_stats(emit, path, label):
    """rocprofv3 --kernel-trace --stats writes <...>_kernel_stats.csv: Name, Calls, TotalDurationNs, ..."""
    total, attn, by = 0.0, 0.0, {}
    with open(path) as f:
        for row in csv.DictReader(f):
            ns = float(row['TotalDurationNs'])
            total += ns
            hit = [k for k in ATTN_KERNELS if k in row['Name']]       # (no name is a substring of another)
            if hit:
                attn += ns
                by[hit[0]] = by.get(hit[0], 0.0) + ns
    emit({'what': 'attention_share_of_kernel_time', 'pair': label, 'source': 'rocprofv3 --kernel-trace --stats',
          'kernel_ms_total': round(total * 1e-6, 2), 'attention_ms': round(attn * 1e-6, 2),
          'attention_share': round(attn / total, 4) if total else None,
          'by_kernel_ms': {k: round(v * 1e-6, 2) for k, v in sorted(by.items())}})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--skip-steps', action='store_true', help='attn_ab only')
    ap.add_argument('--profile-steps', type=int, default=0)
    ap.add_argument('--dense', type=int, default=1)
    ap.add_argument('--kernel-stats', default=None)
    ap.add_argument('--label', default='new_pair')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    a = ap.parse_args()

    def emit(line):
        line.update(dtype='float32', f32_matmul_precision='high')
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(s + '\n')

    if a.kernel_stats:
        return kernel_stats(emit, a.kernel_stats, a.label)
    if not torch.cuda.is_available():
        sys.exit('bench_detr_train: needs a GPU')
    torch.set_float32_matmul_precision('high')
    if a.profile_steps:
        step = build_step(a.dense)
        for _ in range(a.profile_steps):
            step()
        torch.cuda.synchronize()
        return
    attn_ab(emit, a.iters, a.repeats)
    if not a.skip_steps:
        train_steps(emit, a.steps)


if __name__ == '__main__':
    main()
