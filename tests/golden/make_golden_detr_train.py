#!/usr/bin/env python
"""Generate tests/golden/detr_vanilla_train.npz: one training step of the reference's vanilla DETR (config 1,
cfgs/train.yaml as shipped) with its SetCriterion, and a criterion-free step with track queries, through
make_golden.py's import harness.  Only this generator imports the reference; the fixture holds data only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_detr_train.py

Setup, frames, targets and gates: tests/detr_train_refs.py (dropout 0, 2 + 2 layers, train mode, 180 keys of
which 50 are padded on the second frame -- more keys than one tile of the training attention, asserted
below from the plan export).

Case 1: forward -> criterion -> weighted sum -> backward in f32 and the same in f64.  Stored: every loss and
the total, the matched (row, target) pairs of the final and the auxiliary set, and the gradients of
detr_train_refs.GRADS -- up to 8192 elements in full, larger ones on an evenly strided lattice of the flattened
tensor with the L2 norm of the whole beside it -- with max |f32 - f64| over each stored gradient as
`err64:<name>`: the reference's own f32 error.

Case 2 (`track:*`): the same model gets N_TRACK track_query_hs_embeds per frame in `targets` as requires_grad
leaves; loss = sum(pred_logits * W1) + sum(pred_boxes * W2) with seeded W.  Stored: the outputs at TRACK_QSEL
and the gradients w.r.t. the embeddings and query_embed, with their err64.

Asserted here, searching weight seeds from SEED0 when one fails: matched pairs identical in f32 and f64;
every stored gradient non-zero; 10 x the reference's f32-vs-f64 difference under the tests' gates."""
import os
import sys

import numpy as np
import torch

from make_golden import HERE, _install_stubs, load_args, save
from make_golden_detr import build_detr
from weights import randomize

sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import detr_train_refs as T  # noqa: E402

SEED0 = 901


def build_criterion(args):
    """models/__init__.py:127-158 of the reference for the vanilla model (dataset coco: 91 classes)."""
    from trackformer.models.detr import SetCriterion
    from trackformer.models.matcher import build_matcher
    weight_dict = {'loss_ce': args.cls_loss_coef, 'loss_bbox': args.bbox_loss_coef, 'loss_giou': args.giou_loss_coef}
    aux = {}
    for i in range(args.dec_layers - 1):
        aux.update({k + f'_{i}': v for k, v in weight_dict.items()})
    weight_dict.update(aux)
    return SetCriterion(91, matcher=build_matcher(args), weight_dict=weight_dict, eos_coef=args.eos_coef,
                        losses=['labels', 'boxes', 'cardinality'], focal_loss=args.focal_loss,
                        focal_alpha=args.focal_alpha, focal_gamma=args.focal_gamma, tracking=args.tracking,
                        track_query_false_positive_eos_weight=args.track_query_false_positive_eos_weight)


def samples_of(dtype):
    from trackformer.util.misc import nested_tensor_from_tensor_list
    return nested_tensor_from_tensor_list(T.frames(dtype))


def step(model, crit, dtype):
    """One forward / criterion / backward in dtype."""
    model.to(dtype).train()
    crit.to(dtype)
    model.zero_grad(set_to_none=True)
    targets = T.targets(dtype)
    out, targets, features, memory, _ = model(samples_of(dtype), targets)
    assert tuple(memory.shape[-2:]) == T.MAP_HW and int(features[-1].mask[1].sum()) == T.PADDED_KEYS
    with torch.no_grad():
        pairs = {'': crit.matcher({k: v for k, v in out.items() if k != 'aux_outputs'}, targets),
                 '_0': crit.matcher(out['aux_outputs'][0], targets)}
    losses = crit(out, targets)
    total = sum(losses[k] * crit.weight_dict[k] for k in losses if k in crit.weight_dict)
    total.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return dict(losses={k: v.detach() for k, v in losses.items()}, total=total.detach(), pairs=pairs, grads=grads)


def track_step(model, dtype):
    model.to(dtype).train()
    model.zero_grad(set_to_none=True)
    emb = T.track_embeds(model.hidden_dim, dtype).requires_grad_(True)
    targets = [{'track_query_hs_embeds': emb[i]} for i in range(emb.shape[0])]
    out = model(samples_of(dtype), targets)[0]
    w1, w2 = T.track_weights(out['pred_logits'].shape[-1], dtype)
    loss = (out['pred_logits'] * w1).sum() + (out['pred_boxes'] * w2).sum()
    loss.backward()
    return dict(logits=out['pred_logits'].detach(), boxes=out['pred_boxes'].detach(), loss=loss.detach(),
                grads={'track_query_hs_embeds': emb.grad.clone(), 'query_embed.weight': model.query_embed.weight.grad.clone()})


def store_grad(arr, problems, key, name, g, g64):
    full = g
    g, g64 = T.lattice(g), T.lattice(g64)
    err, peak = float((g.double() - g64).abs().max()), float(g.abs().max())
    arr[f'{key}grad:{name}'] = g
    arr[f'{key}norm:{name}'] = full.double().norm()
    arr[f'{key}err64:{name}'] = np.array(err)
    if peak == 0.0:
        problems.append(f'{key}{name}: zero gradient')
    if 10 * err >= T.grad_gate(name, peak):
        problems.append(f'{key}{name}: 10 x f32-vs-f64 {err:.2e} reaches the gate {T.grad_gate(name, peak):.2e}')
    return err / T.grad_gate(name, peak)


def run(seed):
    """(arrays, problems, message) with weight seed `seed`."""
    args = load_args(resume='', device='cpu', **T.OVER)
    assert not args.deformable and not args.focal_loss and args.aux_loss and args.num_queries == 100 and args.hidden_dim == 256
    torch.manual_seed(0)
    model = randomize(build_detr(args), seed)
    crit = build_criterion(args)
    r = step(model, crit, torch.float32)
    r64 = step(model, crit, torch.float64)
    problems = []
    arr = {'seed': np.array(seed), 'loss_total': r['total'], 'loss_total64': r64['total']}
    assert sorted(r['losses']) == sorted(T.loss_keys()), sorted(r['losses'])
    for k, v in r['losses'].items():
        arr[k] = v
        arr[f'err64:{k}'] = np.array(abs(float(v) - float(r64['losses'][k])))
        if abs(float(v) - float(r64['losses'][k])) * 10 >= T.LOSS_RTOL * abs(float(r64['losses'][k])) + T.LOSS_ATOL:
            problems.append(f'{k}: f32 {float(v)} vs f64 {float(r64["losses"][k])}')
    for s, per_image in r['pairs'].items():
        for b, (rows, cols) in enumerate(per_image):
            arr[f'rows{s}:{b}'], arr[f'cols{s}:{b}'] = rows, cols
            rows64, cols64 = r64['pairs'][s][b]
            if not (torch.equal(rows, rows64) and torch.equal(cols, cols64)):
                problems.append(f'matched pairs of set "{s}" frame {b}: {rows.tolist()} vs f64 {rows64.tolist()}')
    assert set(T.GRADS) <= set(r['grads']), set(T.GRADS) - set(r['grads'])
    worst = max(store_grad(arr, problems, '', n, r['grads'][n], r64['grads'][n]) for n in T.GRADS)

    t = track_step(model, torch.float32)
    t64 = track_step(model, torch.float64)
    model.float()
    qsel = torch.tensor(T.TRACK_QSEL)
    arr['track:qsel'] = qsel
    for k in ('logits', 'boxes'):
        arr[f'track:{k}'] = t[k][:, qsel]
        arr[f'track:err64:{k}'] = np.array(float((t[k].double() - t64[k]).abs().max()))
    arr['track:loss'] = t['loss']
    worst = max([worst] + [store_grad(arr, problems, 'track:', n, g, t64['grads'][n]) for n, g in t['grads'].items()])
    msg = (f'seed {seed}: total {float(r["total"]):.5f}, rows {[p[0].tolist() for p in r["pairs"][""]]}, '
           f'worst f32-vs-f64 / gate {worst:.3f}')
    return arr, problems, msg


def main():
    _install_stubs()
    torch.set_num_threads(8)
    from kinet_amd import kernels as K
    kt = K.mha_train_plan(32, 1, 1, 1, 1)['kt']
    assert T.KEYS > kt, f'{T.KEYS} keys do not exceed one {kt}-key tile: grow detr_train_refs.FRAMES'
    for seed in range(SEED0, SEED0 + 60):
        arr, problems, msg = run(seed)
        print(msg, 'ok' if not problems else 'REJECTED: ' + '; '.join(problems[:4]), flush=True)
        if not problems:
            break
    else:
        raise RuntimeError('no weight seed met the fixture conditions')
    save('detr_vanilla_train.npz', **arr)
    size = os.path.getsize(os.path.join(HERE, 'detr_vanilla_train.npz'))
    assert size < (1 << 20), size


if __name__ == '__main__':
    main()
