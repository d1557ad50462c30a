#!/usr/bin/env python
"""Generate the vanilla-DETR (config 1) fixtures under tests/golden/ from the reference model,
with the import harness of make_golden.py (same stubs, same YAML loader, same writer).

Needs the reference checkout make_golden.py imports; the tests read only the files written here:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_detr.py

Every case runs two frames of different sizes, 3x672x992 and 3x608x800, in one NestedTensor: a
21x31 stride-32 feature map = 651 keys (above the resident attention kernels' 384 / 640 key
caps), 176 of the second frame's keys padded.  Weights are tests/golden/weights.py's name-seeded
tensors and the frames come from CPU generator seeds, so only outputs are stored:
  A  detr_vanilla_a.npz   train.yaml as shipped: d 256, 100 queries, 6 + 6 layers (seed 101)
  B  detr_vanilla_b.npz   + train_detr.yaml: d 288, 500 queries (seed 102)
  C  detr_vanilla_c.npz   B with tracking=True in tracking mode, 5 track queries per frame from
                          a seeded randn (seed 102, track-query generator seed 113)
To keep each file well under 1 MB the query-indexed tensors (pred_logits, pred_boxes, hs_embed,
aux*) are stored at the query indices `qsel` (A: every 2nd; B: every 8th; C: the first 8, which
hold the track queries, then every 8th), and encoder memory at [:, :, ::3, ::3].
detr_vanilla_{a,b}.keys.txt list the reference state_dict keys and shapes (C's equal B's).
"""
import os

import numpy as np
import torch

from make_golden import HERE, _install_stubs, load_args, save
from weights import randomize

FRAMES = ((1101, 672, 992), (1102, 608, 800))   # (generator seed, H, W)
N_TRACK = 5


def _frame(seed, h, w):
    return torch.randn(3, h, w, generator=torch.Generator().manual_seed(seed))


def build_detr(args):
    """Replays models/__init__.py:16-46 + :111-125 (vanilla branch) with the reference builders."""
    from trackformer.models.backbone import build_backbone
    from trackformer.models.detr import DETR
    from trackformer.models.detr_tracking import DETRTracking
    from trackformer.models.matcher import build_matcher
    from trackformer.models.transformer import build_transformer
    num_classes = {'coco': 91, 'mot': 20}[args.dataset]
    detr_kwargs = dict(backbone=build_backbone(args),
                       num_classes=num_classes - 1 if args.focal_loss else num_classes,
                       num_queries=args.num_queries, aux_loss=args.aux_loss, overflow_boxes=args.overflow_boxes,
                       transformer=build_transformer(args))
    if args.tracking:
        tracking_kwargs = dict(track_query_false_positive_prob=args.track_query_false_positive_prob,
                               track_query_false_negative_prob=args.track_query_false_negative_prob,
                               matcher=build_matcher(args), backprop_prev_frame=args.track_backprop_prev_frame)
        return DETRTracking(tracking_kwargs, detr_kwargs)
    return DETR(**detr_kwargs)


def write_keys(model, name):
    with open(os.path.join(HERE, name), 'w') as f:
        for k, v in model.state_dict().items():
            f.write(f'{k} {" ".join(str(s) for s in v.shape)}\n')


def run_case(name, model, qsel, targets=None):
    from trackformer.util.misc import nested_tensor_from_tensor_list
    samples = nested_tensor_from_tensor_list([_frame(*f) for f in FRAMES])
    with torch.no_grad():
        out, _, features, memory, hs = model(samples, targets)
    assert tuple(memory.shape[-2:]) == (21, 31), memory.shape
    assert int(features[-1].mask[1].sum()) == 176, int(features[-1].mask[1].sum())
    arr = dict(qsel=qsel, pred_logits=out['pred_logits'][:, qsel], pred_boxes=out['pred_boxes'][:, qsel],
               hs_embed=out['hs_embed'][:, qsel], memory_sub=memory[:, :, ::3, ::3],
               shape_logits=np.array(out['pred_logits'].shape), shape_hs_embed=np.array(out['hs_embed'].shape),
               shape_memory=np.array(memory.shape), shape_hs=np.array(hs.shape))
    for i, aux in enumerate(out['aux_outputs']):
        arr[f'aux{i}_logits'] = aux['pred_logits'][:, qsel]
        arr[f'aux{i}_boxes'] = aux['pred_boxes'][:, qsel]
    save(name, **arr)


def track_queries(d):
    g = torch.Generator().manual_seed(113)
    return [{'track_query_hs_embeds': torch.randn(N_TRACK, d, generator=g)} for _ in FRAMES]


def main():
    _install_stubs()
    torch.set_num_threads(8)
    torch.manual_seed(0)
    a = randomize(build_detr(load_args(resume='', device='cpu')), seed=101).eval()
    write_keys(a, 'detr_vanilla_a.keys.txt')
    run_case('detr_vanilla_a.npz', a, torch.arange(0, 100, 2))

    args_b = load_args('train_detr.yaml', resume='', device='cpu')
    b = randomize(build_detr(args_b), seed=102).eval()
    write_keys(b, 'detr_vanilla_b.keys.txt')
    run_case('detr_vanilla_b.npz', b, torch.arange(0, 500, 8))

    args_c = load_args('train_detr.yaml', resume='', device='cpu', tracking=True)
    c = randomize(build_detr(args_c), seed=102)
    c.tracking()
    assert {k: tuple(v.shape) for k, v in c.state_dict().items()} == \
        {k: tuple(v.shape) for k, v in b.state_dict().items()}
    qsel = torch.cat([torch.arange(0, 8), torch.arange(8, N_TRACK + 500, 8)])
    run_case('detr_vanilla_c.npz', c, qsel, track_queries(args_c.hidden_dim))


if __name__ == '__main__':
    main()
