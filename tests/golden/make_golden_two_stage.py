#!/usr/bin/env python
"""Generate the two-stage Deformable-DETR fixtures under tests/golden/ from the reference model,
with the import harness of make_golden.py (same stubs, same YAML loader, same writer).

Needs the reference checkout make_golden.py imports; the tests read only the files written here:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_two_stage.py

Config: train.yaml + train_deformable.yaml with two_stage=True, num_queries=100.  Two frames of
different sizes, 3x256x448 and 3x224x320, in one NestedTensor: level shapes 32x56, 16x28, 8x14,
4x7 (S = 2380).  Frame 0's first and last level-0 columns fall outside (0.01, 0.99) (64 invalid
tokens), frame 1 is padded (890 invalid tokens).  Weights are tests/golden/weights.py's
name-seeded tensors and the frames come from CPU generator seeds, so only outputs are stored:
  A  two_stage_a.npz   with_box_refine: true  (the config as shipped)
  B  two_stage_b.npz   with_box_refine: false
two_stage_{a,b}.keys.txt list the reference state_dict keys and shapes.

Reference defect (case B): without box refinement DeformableDETR sets decoder.bbox_embed = None
(deformable_detr.py:108) and the two-stage branch then reads decoder.bbox_embed[num_layers]
(deformable_transformer.py:185) -- a TypeError in the first forward.  The harness hands that line
the detector's shared box head (what the `num_pred += 1` above it provides for) as a plain list,
which registers no module, and hides it again while the decoder itself runs, so the decoder
still does not refine: state_dict keys and every other line are the reference's.

Every invalid token's class logit is one constant, class_embed[6](LN(enc_output.bias)); when it
lands inside the top k the selection is a tie among hundreds of equal scores, and adjacent gaps
inside the top k go down to 1e-6.  So the generator searches weight seeds from SEED0 and keeps
the first for which, on every frame, (i) the invalid-row constant is below the k-th score and
(ii) the k-th and (k+1)-th scores are >= 4e-3 apart (4x the project's fp32 gate of 1e-3: two
logits each within the gate cannot cross it).  The seed used is stored as `seed`.
"""
import os

import numpy as np
import torch

from make_golden import HERE, _install_stubs, build_deformable, load_args, save
from weights import randomize

FRAMES = ((2101, 256, 448), (2102, 224, 320))   # (generator seed, H, W)
SHAPES = ((32, 56), (16, 28), (8, 14), (4, 7))
K = 100
SEED0 = {'a': 201, 'b': 301}
MIN_GAP = 4e-3


def _frame(seed, h, w):
    return torch.randn(3, h, w, generator=torch.Generator().manual_seed(seed))


def patch_proposal_head(model):
    """Case B, see the module docstring."""
    dec = model.transformer.decoder
    assert dec.bbox_embed is None
    heads = list(model.bbox_embed)
    dec.bbox_embed = heads
    orig = dec.forward

    def forward(*a, **kw):
        dec.bbox_embed = None
        try:
            return orig(*a, **kw)
        finally:
            dec.bbox_embed = heads
    dec.forward = forward


def write_keys(model, name):
    with open(os.path.join(HERE, name), 'w') as f:
        for k, v in model.state_dict().items():
            f.write(f'{k} {" ".join(str(s) for s in v.shape)}\n')


def check(out):
    """(ok, message): conditions (i) and (ii) on every frame."""
    logits = out['enc_outputs']['pred_logits'][..., 0]
    boxes = out['enc_outputs']['pred_boxes']
    for b in range(logits.shape[0]):
        invalid = (boxes[b] == 1).all(-1)
        const = logits[b][invalid]
        assert (const == const[0]).all()
        s = torch.sort(logits[b], descending=True, stable=True)[0]
        if not float(const[0]) < float(s[K - 1]):
            return False, f'frame {b}: invalid-row constant {float(const[0]):.5f} >= k-th score {float(s[K - 1]):.5f}'
        if float(s[K - 1] - s[K]) < MIN_GAP:
            return False, f'frame {b}: gap at the cut {float(s[K - 1] - s[K]):.2e} < {MIN_GAP}'
    return True, ''


def run_case(tag, with_box_refine):
    from trackformer.util.misc import nested_tensor_from_tensor_list
    args = load_args('train_deformable.yaml', resume='', device='cpu', two_stage=True, num_queries=K,
                     with_box_refine=with_box_refine)
    torch.manual_seed(0)
    model = build_deformable(args)
    if not with_box_refine:
        patch_proposal_head(model)
    write_keys(model, f'two_stage_{tag}.keys.txt')
    samples = nested_tensor_from_tensor_list([_frame(*f) for f in FRAMES])
    for seed in range(SEED0[tag], SEED0[tag] + 200):   # about one seed in fifteen meets both conditions
        randomize(model, seed=seed).eval()
        with torch.no_grad():
            out, _, features, memory, hs = model(samples)
        ok, why = check(out)
        print(f'case {tag} seed {seed}: {"ok" if ok else why}')
        if ok:
            break
    else:
        raise RuntimeError('no weight seed met the selection conditions')
    assert [tuple(m.shape[-2:]) for m in memory] == list(SHAPES), [m.shape for m in memory]
    enc = out['enc_outputs']
    n_invalid = (enc['pred_boxes'] == 1).all(-1).sum(1).tolist()
    assert n_invalid == [64, 890], n_invalid
    topk = torch.topk(enc['pred_logits'][..., 0], K, dim=1)[1]     # deformable_transformer.py:188
    arr = dict(seed=np.array(seed), topk=topk, enc_logits0=enc['pred_logits'][..., 0], enc_boxes=enc['pred_boxes'],
               pred_logits=out['pred_logits'], pred_boxes=out['pred_boxes'], hs_embed=out['hs_embed'],
               shape_enc_logits=np.array(enc['pred_logits'].shape), shape_hs=np.array(hs.shape))
    for i, aux in enumerate(out['aux_outputs']):
        arr[f'aux{i}_logits'] = aux['pred_logits']
        arr[f'aux{i}_boxes'] = aux['pred_boxes']
    save(f'two_stage_{tag}.npz', **arr)


def main():
    _install_stubs()
    torch.set_num_threads(8)
    run_case('a', True)
    run_case('b', False)


if __name__ == '__main__':
    main()
