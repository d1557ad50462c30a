"""Device time of two-stage Deformable DETR training (kinet_amd.train.build_two_stage_training,
csrc/criterion.hip) at the real workload's sizes: 2 frames of 3 x 800 x 1333 (22 223 encoder tokens each),
300 proposals, 10-30 targets per frame from synthetic_mot_batch, f32 with 'high' matmul precision (the
training benchmark's setting), dropout 0.  JSON lines, times in milliseconds as [median, min, max] of
`--repeats` windows of `--iters` calls between HIP events after a warm-up, the variants alternating window
by window; peak memory is torch's allocator peak above what was allocated before the call.

  enc_match_cost       (a) the enc_outputs matcher cost: HungarianMatcher.cost_block_diagonal (one kernel)
                       next to HungarianMatcher.cost_matrix (the torch composition it replaces) on the
                       same tensors
  enc_focal_loss       (a) loss_ce_enc forward + backward: autograd.focal_set_loss next to
                       SetCriterion.loss_labels_focal on the same tensors and indices
  proposal_stage       (b) DeformableTransformer._proposal_queries_train forward + backward (memory -> queries,
                       enc class logits and boxes), every output given a gradient
  train_step           (c) kinet_amd.train.train_step of the two-stage model next to the one-stage model
                       (two_stage: false, otherwise the same config, the weights it shares and the same frames)

usage: python tools/bench_two_stage_train.py [--iters N] [--repeats R] [--steps K] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, B, Q = 800, 1333, 2, 300


def windows(fns, iters, repeats):
    """{name: [median, min, max]} ms per call, the variants alternating window by window."""
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
            t[k].append(s.elapsed_time(e) / iters)
    return {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in t.items()}


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)


def build(two_stage):
    from kinet_amd.models import build_model
    from kinet_amd.models.config import load_args
    from kinet_amd.train import build_optimizer, build_two_stage_training
    args = load_args('train_deformable', two_stage=two_stage, with_box_refine=True, dropout=0.0, num_queries=Q,
                     device='cuda')
    torch.manual_seed(0)
    model, criterion, _ = (build_two_stage_training if two_stage else build_model)(args)
    model = model.cuda().train()
    return args, model, criterion.cuda(), build_optimizer(model, args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_two_stage_train: needs a GPU')
    from kinet_amd.train import synthetic_mot_batch, train_step
    torch.set_float32_matmul_precision('high')
    dev = torch.device('cuda')
    samples, targets = synthetic_mot_batch(B, H, W, dev, torch.Generator().manual_seed(1000))
    targets = [{k: t[k] for k in ('boxes', 'labels')} for t in targets]
    lines = []

    def emit(line):
        line.update(frames=[B, H, W], targets_per_frame=[len(t['labels']) for t in targets], dtype='float32',
                    f32_matmul_precision='high')
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(s + '\n')
        lines.append(line)

    args, model, criterion, opt = build(True)
    t = model.transformer
    cap, orig = {}, t._proposal_queries_train

    def grab(memory, geo, head=None):
        cap.update(memory=memory.detach(), geo=geo, head=head)
        return orig(memory, geo, head)
    t._proposal_queries_train = grab
    try:
        out = model(samples, targets)[0]
    finally:
        del t._proposal_queries_train
    enc = {k: v.detach() for k, v in out['enc_outputs'].items()}
    S, C = enc['pred_logits'].shape[1:]
    del out
    bin_targets = [dict(tg, labels=torch.zeros_like(tg['labels'])) for tg in targets]
    matcher = criterion.matcher

    # (a) the matcher cost of the enc_outputs set
    fused_cost = matcher.cost_block_diagonal(enc, bin_targets, [])
    comp_cost = matcher.cost_matrix(enc, bin_targets, [])
    sizes = [len(tg['labels']) for tg in targets]
    diag = torch.cat([c[b] for b, c in enumerate(comp_cost.split(sizes, -1))], 1)
    r = windows({'fused': lambda: matcher.cost_block_diagonal(enc, bin_targets, []),
                 'torch': lambda: matcher.cost_matrix(enc, bin_targets, [])}, a.iters, a.repeats)
    emit({'what': 'enc_match_cost', 'tokens': S, 'classes': C, 'ms_median_min_max': r,
          'torch_over_fused': round(r['torch'][0] / r['fused'][0], 2),
          'peak_mib': {'fused': peak_mib(lambda: matcher.cost_block_diagonal(enc, bin_targets, [])),
                       'torch': peak_mib(lambda: matcher.cost_matrix(enc, bin_targets, []))},
          'fused_vs_torch_max_abs': (fused_cost - diag).abs().max().item(), 'iters': a.iters, 'repeats': a.repeats})

    # (a) loss_ce_enc forward + backward
    indices = [tuple(i.cuda() for i in pair) for pair in matcher(enc, bin_targets)]
    nb = float(sum(sizes))
    logits = enc['pred_logits'].clone().requires_grad_(True)

    def fused_loss():
        logits.grad = None
        loss = criterion.loss_labels_focal_set({'pred_logits': logits}, bin_targets, indices, nb)['loss_ce']
        loss.backward()
        return loss.detach(), logits.grad

    def torch_loss():
        logits.grad = None
        loss = criterion.loss_labels_focal({'pred_logits': logits}, bin_targets, indices, nb, log=False)['loss_ce']
        loss.backward()
        return loss.detach(), logits.grad
    (lf, gf), (lt, gt) = fused_loss(), torch_loss()

    def loss_peak(fn):
        logits.grad = None          # (the previous call's gradient is not part of this call's baseline)
        return peak_mib(fn)
    diff = {'loss_rel': abs(lf - lt).item() / abs(lt).item(), 'dlogits_max_abs': (gf - gt).abs().max().item(),
            'dlogits_peak': gt.abs().max().item()}
    r = windows({'fused': fused_loss, 'torch': torch_loss}, a.iters, a.repeats)
    emit({'what': 'enc_focal_loss', 'tokens': S, 'classes': C, 'ms_median_min_max': r,
          'torch_over_fused': round(r['torch'][0] / r['fused'][0], 2),
          'peak_mib': {'fused': loss_peak(fused_loss), 'torch': loss_peak(torch_loss)}, 'fused_vs_torch': diff,
          'iters': a.iters, 'repeats': a.repeats})

    # (b) the proposal stage, forward + backward
    memory = cap['memory'].clone().requires_grad_(True)

    def stage():
        memory.grad = None
        query_pos, tgt, _, enc_class, _ = orig(memory, cap['geo'], cap['head'])
        boxes = t.enc_outputs_coord
        (query_pos.sum() + tgt.sum() + enc_class.sum() * 1e-3 + boxes.sum()).backward()
    r = windows({'forward_backward': stage}, max(1, a.iters // 4), a.repeats)
    model.zero_grad(set_to_none=True)
    emit({'what': 'proposal_stage', 'tokens': S, 'proposals': Q, 'ms_median_min_max': r,
          'peak_mib': peak_mib(stage), 'iters': max(1, a.iters // 4), 'repeats': a.repeats})
    model.zero_grad(set_to_none=True)
    memory = None
    cap.clear()

    # (c) the whole training step, two-stage next to one-stage
    args1, model1, criterion1, opt1 = build(False)
    own = model1.state_dict()
    shared = {k: v for k, v in model.state_dict().items() if k in own and own[k].shape == v.shape}
    model1.load_state_dict(shared, strict=False)

    def step2():
        return train_step(model, criterion, opt, samples, [dict(tg) for tg in targets], args.clip_max_norm)[0]

    def step1():
        return train_step(model1, criterion1, opt1, samples, [dict(tg) for tg in targets], args1.clip_max_norm)[0]
    r = windows({'two_stage': step2, 'one_stage': step1}, 1, a.steps)
    emit({'what': 'train_step', 'queries': Q, 'ms_median_min_max': r,
          'two_stage_over_one_stage': round(r['two_stage'][0] / r['one_stage'][0], 3),
          'shared_parameters': len(shared), 'loss': {'two_stage': float(step2()), 'one_stage': float(step1())},
          'steps': a.steps})


if __name__ == '__main__':
    main()
