"""f64 references and error bounds of the criterion kernels (csrc/criterion.hip;
tests/test_criterion_direct_gpu.py), and the constants, frames and targets that the two-stage training
fixture (tests/golden/make_golden_two_stage_train.py -> two_stage_train.npz) and its tests share.

Every reference is plain torch in double on the CPU over the same inputs the kernels read.  Bounds are
operation counts in the style of tests/direct_refs.py and tests/segm_refs.py -- per element,
    (roundings of the f32 evaluation) * 2^-24 * |the quantities they apply to|, times SLACK,
formed from the f64 values, never from what the kernels return.
"""
import math

import torch

from segm_refs import SLACK, U32, gen
from segm_train_refs import GRAD_ATOL, GRAD_GATE, GRAD_GATE_BACKBONE, grad_gate, lattice  # noqa: F401  (shared gates)

ALPHA, GAMMA = 0.25, 2.0
TINY = 1e-30    # absolute floor: f32 flushes what f64 still holds (sigmoid(-100)^2 = 1e-87)


# --------------------------------------------------------------------------- shared pieces
def logit_terms(x):
    """p = sigmoid(x), q = 1 - p without cancellation, softplus(x), softplus(-x) in the dtype of x."""
    e = torch.exp(-x.abs())
    inv = 1 / (1 + e)
    l = torch.log1p(e)
    p = torch.where(x >= 0, inv, e * inv)
    q = torch.where(x >= 0, e * inv, inv)
    return p, q, x.clamp(min=0) + l, (-x).clamp(min=0) + l


def xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)


# --------------------------------------------------------------------------- matcher cost
def cost_case(B, Q, C, sizes, seed, scale=3.0):
    """logits (B, Q, C) of a few units, prediction boxes with centres in (0.1, 0.9) and sides in (0.03, 0.5),
    sum(sizes) targets with sides in (0.05, 0.4) and labels in [0, C); sizes: targets per image."""
    g = gen(seed)
    T = sum(sizes)
    logits = torch.randn(B, Q, C, generator=g) * scale
    boxes = torch.cat([torch.rand(B, Q, 2, generator=g) * 0.8 + 0.1, torch.rand(B, Q, 2, generator=g) * 0.47 + 0.03], -1)
    labels = torch.randint(0, C, (T,), generator=g)
    tboxes = torch.cat([torch.rand(T, 2, generator=g) * 0.8 + 0.1, torch.rand(T, 2, generator=g) * 0.35 + 0.05], -1)
    return logits, boxes, labels, tboxes


def match_cost_ref(logits, boxes, labels, tboxes, sizes, w_class, w_bbox, w_giou, alpha=ALPHA, gamma=GAMMA):
    """(cost (Q, T), tol (Q, T)) in f64: matcher.py:135-171 on the image-diagonal blocks.

    Roundings counted (u = 2^-24):
      class  p, q: exp, 1 + e, the division, e * inv -> 4 u each; p^gamma, q^gamma 2 * 4 u + u; the log's
             argument p + 1e-8 carries 5 u relative, i.e. 5 u absolute on the log, and logf 2 u of |log|; three
             products and the difference.  pos = alpha q^g L(p), neg = (1 - alpha) p^g L(q), L = -log(. + 1e-8):
                 err <= 12 u (pos + neg) + (alpha q^g + (1 - alpha) p^g) 5 u + u |pos - neg|
      L1     four differences and three additions: 4 u L1
      GIoU   every xyxy coordinate is one rounding, d = u max|coordinate| of the pair.  A side (difference of
             two coordinates, clamped) errs by 2 d + u side; a product of sides s t by 2 d (s + t) + 3 u s t;
             union = a1 + a2 - inter adds the three and 2 u (a1 + a2 + inter);
                 iou = inter / union:      e_i / union + inter e_u / union^2 + u iou
                 (enc - union) / enc:      (e_enc + e_u + u |enc - union|) / enc + |enc - union| e_enc / enc^2 + u (.)
             and their difference u (|iou| + |.|).  First order: the tests keep every side >= 0.03.
      sum    three products and two additions of the weighted terms: 3 u sum |w term|."""
    B, Q, C = logits.shape
    T = labels.numel()
    l64, b64, t64 = logits.double(), boxes.double(), tboxes.double()
    cost = torch.zeros(Q, T, dtype=torch.float64)
    tol = torch.zeros(Q, T, dtype=torch.float64)
    o = 0
    for b, n in enumerate(sizes):
        if n == 0:
            continue
        lab, tb = labels[o:o + n], t64[o:o + n]
        p, q, _, _ = logit_terms(l64[b][:, lab])                                   # (Q, n)
        Lp, Lq = -torch.log(p + 1e-8), -torch.log(q + 1e-8)
        pos, neg = alpha * q ** gamma * Lp, (1 - alpha) * p ** gamma * Lq
        c_class = pos - neg
        e_class = U32 * (12 * (pos.abs() + neg.abs()) + 5 * (alpha * q ** gamma + (1 - alpha) * p ** gamma)
                         + c_class.abs())
        pb = b64[b]
        c_bbox = (pb[:, None] - tb[None]).abs().sum(-1)
        e_bbox = 4 * U32 * c_bbox
        P, Tt = xyxy(pb)[:, None], xyxy(tb)[None]                                  # (Q, 1, 4), (1, n, 4)
        d = U32 * torch.maximum(P.abs().amax(-1), Tt.abs().amax(-1))               # (Q, n)

        def prod(s, t):
            return s * t, 2 * d * (s + t) + 3 * U32 * s * t + 4 * d * d
        a1, e_a1 = prod(P[..., 2] - P[..., 0], P[..., 3] - P[..., 1])
        a2, e_a2 = prod(Tt[..., 2] - Tt[..., 0], Tt[..., 3] - Tt[..., 1])
        iw = (torch.minimum(P[..., 2], Tt[..., 2]) - torch.maximum(P[..., 0], Tt[..., 0])).clamp(min=0)
        ih = (torch.minimum(P[..., 3], Tt[..., 3]) - torch.maximum(P[..., 1], Tt[..., 1])).clamp(min=0)
        inter, e_i = prod(iw, ih)
        union = a1 + a2 - inter
        e_u = e_a1 + e_a2 + e_i + 2 * U32 * (a1 + a2 + inter)
        iou = inter / union
        e_iou = e_i / union + inter * e_u / union ** 2 + U32 * iou
        ew = (torch.maximum(P[..., 2], Tt[..., 2]) - torch.minimum(P[..., 0], Tt[..., 0])).clamp(min=0)
        eh = (torch.maximum(P[..., 3], Tt[..., 3]) - torch.minimum(P[..., 1], Tt[..., 1])).clamp(min=0)
        enc, e_enc = prod(ew, eh)
        excess = (enc - union) / enc
        e_excess = ((e_enc + e_u + U32 * (enc - union).abs()) / enc + (enc - union).abs() * e_enc / enc ** 2
                    + U32 * excess.abs())
        giou = iou - excess
        e_giou = e_iou + e_excess + U32 * (iou.abs() + excess.abs())
        terms = abs(w_bbox) * c_bbox + abs(w_class) * c_class.abs() + abs(w_giou) * giou.abs()
        cost[:, o:o + n] = w_bbox * c_bbox + w_class * c_class + w_giou * -giou
        tol[:, o:o + n] = SLACK * (abs(w_bbox) * e_bbox + abs(w_class) * e_class + abs(w_giou) * e_giou
                                   + 3 * U32 * terms) + TINY
        o += n
    return cost, tol


def boxes_ok_ref(boxes, tboxes):
    """util/box_ops.py:44-45 over every prediction and target box."""
    a, b = xyxy(boxes.reshape(-1, 4)), xyxy(tboxes.reshape(-1, 4))
    return bool((a[:, 2:] >= a[:, :2]).all()) and bool((b[:, 2:] >= b[:, :2]).all())


# --------------------------------------------------------------------------- focal set loss
FL_VEC_PER_BLOCK, FL_MAX_BLOCKS = 2048, 1024      # csrc/criterion.hip


def focal_blocks(total):
    nvec = total // 4
    per = max(FL_VEC_PER_BLOCK, -(-nvec // FL_MAX_BLOCKS))
    return max(1, -(-nvec // per)), per


def focal_elements(x, t, alpha=ALPHA, gamma=GAMMA):
    """util/misc.py:634-665 per element in the dtype of x, in the stable form (no reduction)."""
    p, q, sp_pos, sp_neg = logit_terms(x)
    a1, a0 = (alpha, 1 - alpha) if alpha >= 0 else (1.0, 1.0)
    return torch.where(t > 0, a1 * sp_neg * q ** gamma, a0 * sp_pos * p ** gamma)


def focal_set_ref(logits, pos_rows, pos_cls, num_boxes, alpha=ALPHA, gamma=GAMMA, dloss=1.0):
    """(loss, tol_loss, dlogits (R, C), tol_dlogits) in f64 (the gradient by autograd).

    An element: exp and log1p at 2 u, 1 + e, the division, e * inv, the power and three products: 16 u of
    the term (24 u of its derivative, which has one more sum and three more products).  Every element is
    summed once with its own target (no term is added and taken back), all terms are >= 0: a thread adds
    4 * ceil(per / 256) of them (+ 1 of the tail), then the butterfly (6), the waves (3), ceil(blocks / 256)
    partials, the butterfly and waves again and the scale: depth = 4 ceil(per / 256) + ceil(blocks / 256) + 21."""
    R, C = logits.shape
    x = logits.double().requires_grad_(True)
    t = torch.zeros(R, C, dtype=torch.float64)
    t[pos_rows, pos_cls] = 1
    el = focal_elements(x, t, alpha, gamma)
    loss = el.sum() / num_boxes
    (loss * dloss).backward()
    blocks, per = focal_blocks(R * C)
    depth = 4 * math.ceil(per / 256) + math.ceil(blocks / 256) + 21
    tol_loss = SLACK * U32 * (depth + 16) * el.detach().sum() / num_boxes + TINY
    tol_grad = SLACK * 24 * U32 * x.grad.abs() + TINY
    return loss.detach(), tol_loss, x.grad, tol_grad


# --------------------------------------------------------------------------- the training-step fixture
# tests/golden/make_golden_two_stage_train.py -> two_stage_train.npz: case A of make_golden_two_stage.py
# (its two frames in one NestedTensor, 32x56 / 16x28 / 8x14 / 4x7 levels, S = 2380, 64 invalid and 890
# padded tokens), with_box_refine, dropout 0, 2 encoder and 2 decoder layers, 30 proposals, train mode.
TRAIN_FRAMES = ((2101, 256, 448), (2102, 224, 320))       # (generator seed, H, W)
TRAIN_SHAPES = ((32, 56), (16, 28), (8, 14), (4, 7))
TRAIN_S = 2380
TRAIN_K = 30
TRAIN_OVER = dict(two_stage=True, with_box_refine=True, dropout=0.0, enc_layers=2, dec_layers=2, num_queries=TRAIN_K)
TRAIN_TARGETS = ((5101, 3), (5102, 2))                    # (generator seed, boxes) per frame
TRAIN_GRADS = ('transformer.enc_output.weight', 'transformer.enc_output.bias', 'transformer.enc_output_norm.weight',
               'transformer.enc_output_norm.bias', 'transformer.pos_trans.weight', 'transformer.pos_trans.bias',
               'transformer.pos_trans_norm.weight', 'transformer.pos_trans_norm.bias',
               'class_embed.2.weight', 'class_embed.2.bias', 'bbox_embed.2.layers.0.weight',
               'bbox_embed.2.layers.2.weight', 'bbox_embed.2.layers.2.bias', 'class_embed.1.weight',
               'bbox_embed.0.layers.1.weight', 'transformer.encoder.layers.1.linear2.weight',
               'transformer.encoder.layers.0.self_attn.sampling_offsets.weight',
               'transformer.decoder.layers.1.linear2.weight',
               'transformer.decoder.layers.0.cross_attn.attention_weights.weight', 'input_proj.1.0.weight',
               'backbone.0.body.layer3.0.conv2.weight')
TRAIN_LOSSES = ('loss_ce', 'loss_bbox', 'loss_giou', 'cardinality_error', 'class_error')
TRAIN_SETS = ('', '_0', '_enc')                           # final, the one auxiliary layer, the proposals


def train_frames(dtype=torch.float32):
    return [torch.randn(3, h, w, generator=gen(s)).to(dtype) for s, h, w in TRAIN_FRAMES]


def train_targets(dtype=torch.float32):
    """Per frame: boxes with centres in (0.25, 0.75) and sides in (0.15, 0.45) of the frame, labels in [1, 90]
    (non-zero, so that the enc_outputs set's zeroed copies differ from them)."""
    out = []
    for seed, n in TRAIN_TARGETS:
        g = gen(seed)
        boxes = torch.cat([torch.rand(n, 2, generator=g) * 0.5 + 0.25, torch.rand(n, 2, generator=g) * 0.3 + 0.15], -1)
        out.append({'boxes': boxes.to(dtype), 'labels': torch.randint(1, 91, (n,), generator=g)})
    return out


def loss_keys():
    """Every key the two-stage criterion returns for this setup."""
    keys = []
    for s in TRAIN_SETS:
        keys += [k + s for k in TRAIN_LOSSES if not (k == 'class_error' and s)]
    return keys
