#!/usr/bin/env python
"""Generate the segmentation (pred_masks) fixtures under tests/golden/ from the reference's
DeformableDETRSegm / DeformableDETRSegmTracking and PostProcessSegm, with the import harness of
make_golden.py (same stubs, same YAML loader, same writer).

Needs the reference checkout make_golden.py imports; the tests read only the files written here:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_segm.py

Two frames of different sizes, 3x104x200 and 3x88x136, in one NestedTensor: backbone shapes 26x50
/ 13x25 / 7x13 / 4x7, so the second frame is padded and every upsampling ratio of the head is
non-integer (7x13 -> 13x25 -> 26x50).  Weights are weights.py's name-seeded tensors conditioned by
segm_weights.py (without it the masks do not depend on the query at all), frames come from CPU
generator seeds, so only outputs are stored:
  A  segm_a.npz   train_deformable.yaml + masks, Q = 12
  B  segm_b.npz   A + tracking: frame pair first without track queries, then with its top 5 per
                  frame as track queries (17 queries), as gen_detr_tracking_multiframe injects them
  C  segm_c.npz   B with train_multi_frame.yaml's multi_frame_attention and separate encoders (8
                  memory slices).  hidden_dim stays 256: that file's 288 cannot build a mask head
                  (context_dim // 16 = 18 channels under GroupNorm(8, .) raises in the reference's
                  constructor), and at 256 its multi_frame_encoding cannot run (the 3-d sine
                  embedding's 256 // 3 = 85 features per axis is odd: its sin / cos stack raises),
                  so multi_frame_encoding is false
No case passes prev_features.  segm_{a,b,c}.keys.txt list the reference state_dict keys and shapes.

PostProcessSegm runs on each case's pred_masks with max_target_sizes = the frame sizes and
orig_target_sizes = 208x400 and 131x203.  Its outputs are 110 k pixels per query, so they are stored
as: the binary masks bit-packed (`post{i}_bits`), the pixels whose probability lies within BAND of
the threshold bit-packed (`post{i}_band`: the tests skip those), and the probabilities of
`return_probs` on the pixel lattice [::3, ::3] (`post{i}_probs3`, case A only).

The generator asserts, and searches weight seeds from SEED0 when an assertion fails:
  * per frame, the median over pixels of max_q - min_q of pred_masks is >= 0.1 (100x the fp32 gate);
  * the share of upsampled, cropped logits with |logit| < 2e-3 is <= 0.5 %.
"""
import os
import shutil

import numpy as np
import torch

from make_golden import HERE, REF_CFG, _install_stubs, load_args, save
from make_golden_two_stage import write_keys
from segm_weights import randomize_segm

FRAMES = ((4101, 104, 200), (4102, 88, 136))    # (generator seed, H, W)
FEATS = ((26, 50), (13, 25), (7, 13), (4, 7))
ORIG = ((208, 400), (131, 203))
Q = 12
K_TRACK = 5
SEED0 = 401
BAND = 5e-4
MIN_SPREAD = 0.1
MAX_NEAR = 5e-3


def _frame(seed, h, w):
    return torch.randn(3, h, w, generator=torch.Generator().manual_seed(seed))


def build_segm(args):
    """Replays models/__init__.py:16-71 for deformable + masks with the reference's builders."""
    from trackformer.models.backbone import build_backbone
    from trackformer.models.deformable_transformer import build_deforamble_transformer
    from trackformer.models.detr_segmentation import DeformableDETRSegm, DeformableDETRSegmTracking
    from trackformer.models.matcher import build_matcher
    num_classes = 91 if args.dataset == 'coco' else 20
    backbone = build_backbone(args)
    backbone.strides = backbone[0].strides          # reference defect, see make_golden.py
    detr_kwargs = dict(backbone=backbone, num_classes=num_classes - 1 if args.focal_loss else num_classes,
                       num_queries=args.num_queries, aux_loss=args.aux_loss, overflow_boxes=args.overflow_boxes,
                       transformer=build_deforamble_transformer(args), num_feature_levels=args.num_feature_levels,
                       with_box_refine=args.with_box_refine, two_stage=args.two_stage,
                       multi_frame_attention=args.multi_frame_attention,
                       multi_frame_encoding=args.multi_frame_encoding,
                       merge_frame_features=args.merge_frame_features)
    mask_kwargs = dict(freeze_detr=args.freeze_detr)
    if args.tracking:
        tracking_kwargs = dict(track_query_false_positive_prob=args.track_query_false_positive_prob,
                               track_query_false_negative_prob=args.track_query_false_negative_prob,
                               matcher=build_matcher(args), backprop_prev_frame=args.track_backprop_prev_frame)
        return DeformableDETRSegmTracking(mask_kwargs, tracking_kwargs, detr_kwargs)
    return DeformableDETRSegm(mask_kwargs, detr_kwargs)


CASES = {
    'a': dict(),
    'b': dict(tracking=True),
    'c': dict(tracking=True, multi_frame_attention=True, multi_frame_encoding=False,
              multi_frame_attention_separate_encoder=True),
}


def forward(model, samples, tracking):
    """(out, memory, attention map) of the case's last forward."""
    att = []
    hook = model.bbox_attention.register_forward_hook(lambda m, i, o: att.append(o))
    with torch.no_grad():
        if tracking:
            out0 = model(samples)[0]
            att.clear()
            targets = []
            for b in range(len(FRAMES)):
                top = out0['pred_logits'][b].sigmoid().max(-1)[0].topk(K_TRACK).indices
                targets.append({'track_query_hs_embeds': out0['hs_embed'][b, top],
                                'track_query_boxes': out0['pred_boxes'][b, top]})
            out, _, _, memory, _ = model(samples, targets)
        else:
            out, _, _, memory, _ = model(samples)
    hook.remove()
    return out, memory, att[0]


def check(pred_masks):
    """(ok, message, measurements)."""
    import torch.nn.functional as F
    spreads = []
    for b, (_, h, w) in enumerate(FRAMES):
        m = pred_masks[b, :, :h // 4, :w // 4]
        spreads.append(float((m.max(0)[0] - m.min(0)[0]).median()))
    max_h, max_w = max(f[1] for f in FRAMES), max(f[2] for f in FRAMES)
    up = F.interpolate(pred_masks, size=(max_h, max_w), mode='bilinear', align_corners=False)
    near = [float((up[b, :, :h, :w].abs() < 2e-3).float().mean()) for b, (_, h, w) in enumerate(FRAMES)]
    msg = f'median spread {spreads}, near-threshold share {near}'
    return min(spreads) >= MIN_SPREAD and max(near) <= MAX_NEAR, msg, (spreads, near)


def post_arrays(pred_masks, with_probs):
    from trackformer.models.detr_segmentation import PostProcessSegm
    post = PostProcessSegm()
    max_sizes = torch.tensor([[h, w] for _, h, w in FRAMES])
    orig = torch.tensor(ORIG)
    outputs = {'pred_masks': pred_masks.unsqueeze(2)}
    binary = post([{} for _ in FRAMES], outputs, orig, max_sizes)
    probs = post([{} for _ in FRAMES], outputs, orig, max_sizes, return_probs=True)
    arr = {'orig_sizes': orig, 'max_sizes': max_sizes}
    for i, (rb, rp) in enumerate(zip(binary, probs)):
        mb, mp = rb['masks'], rp['masks']
        assert mb.dtype == torch.uint8 and mb.shape == (pred_masks.shape[1], 1) + ORIG[i], (mb.dtype, mb.shape)
        assert torch.equal(mb, (mp > post.threshold).byte())
        arr[f'post{i}_bits'] = np.packbits(mb.numpy().reshape(-1))
        arr[f'post{i}_band'] = np.packbits(((mp - post.threshold).abs() <= BAND).numpy().reshape(-1))
        arr[f'post{i}_band_share'] = ((mp - post.threshold).abs() <= BAND).float().mean()
        if with_probs:
            arr[f'post{i}_probs3'] = mp[:, :, ::3, ::3]
    return arr


def run_case(tag, over, seed0):
    from trackformer.util.misc import nested_tensor_from_tensor_list
    tracking = over.get('tracking', False)
    args = load_args('train_deformable.yaml', resume='', device='cpu', masks=True, num_queries=Q, **over)
    torch.manual_seed(0)
    model = build_segm(args)
    write_keys(model, f'segm_{tag}.keys.txt')
    samples = nested_tensor_from_tensor_list([_frame(*f) for f in FRAMES])
    for seed in range(seed0, seed0 + 50):
        randomize_segm(model, seed)
        model.tracking() if tracking else model.eval()
        out, memory, att = forward(model, samples, tracking)
        ok, msg, (spreads, near) = check(out['pred_masks'])
        print(f'case {tag} seed {seed}: {msg} peak attention {float(att.max()):.3f} {"ok" if ok else "REJECTED"}')
        if ok:
            break
    else:
        raise RuntimeError('no weight seed met the fixture conditions')
    nq = Q + (K_TRACK if tracking else 0)
    assert out['pred_masks'].shape == (len(FRAMES), nq) + FEATS[0], out['pred_masks'].shape
    assert att.shape == (len(FRAMES), nq, 8) + FEATS[2], att.shape
    assert torch.is_tensor(memory) and memory.shape == (len(FRAMES), 256) + FEATS[2], memory.shape
    model64 = model.double()
    s64 = nested_tensor_from_tensor_list([_frame(*f).double() for f in FRAMES])
    out64 = forward(model64, s64, tracking)[0]
    f32_err = float((out64['pred_masks'] - out['pred_masks'].double()).abs().max())
    print(f'case {tag}: reference f32 vs f64 forward, max diff on pred_masks {f32_err:.2e}')
    arr = dict(seed=np.array(seed), pred_masks=out['pred_masks'], attention=att, pred_logits=out['pred_logits'],
               pred_boxes=out['pred_boxes'], hs_embed=out['hs_embed'], shape_memory=np.array(memory.shape),
               median_spread=np.array(spreads), near_share=np.array(near), ref_f32_err=np.array(f32_err))
    arr.update(post_arrays(out['pred_masks'], with_probs=tag == 'a'))
    save(f'segm_{tag}.npz', **arr)


def main():
    _install_stubs()
    torch.set_num_threads(8)
    import sys
    for tag, over in CASES.items():
        if not sys.argv[1:] or tag in sys.argv[1:]:
            run_case(tag, over, SEED0)
    for cfg in ('train_coco_person_masks.yaml', 'train_mots20.yaml'):
        shutil.copyfile(os.path.join(REF_CFG, cfg), os.path.join(HERE, 'cfgs', cfg))


if __name__ == '__main__':
    main()
