"""f64 references and error bounds for the direct tests of the mask-training kernels
(csrc/segm_train.hip; tests/test_segm_train_direct_gpu.py).  Every reference is torch autograd in
double on the CPU over the plain composition (F.interpolate, softmax, relu, F.conv2d) of the same
inputs the kernels read; nothing here is a hand-written derivative.

Bounds follow tests/segm_refs.py: per element, from the f64 sums of the ABSOLUTE terms of the sum
that element is, never from what the kernels return:
    (length of the f32 accumulation chain) * 2^-24 * sum |terms|  +  (input errors propagated),  times SLACK.
The sums of absolute terms come from the same autograd graphs run on absolute values (the adjoint
of a resize or a convolution with non-negative weights applied to |terms|).
"""
import math

import torch
import torch.nn.functional as F

from segm_refs import HEADS, SLACK, U32, gen, nearest_index

ALPHA, GAMMA = 0.25, 2.0

# |d^2 focal / dv^2| <= FOCAL_D2 and |d focal / dv| <= FOCAL_D1 for every logit v and both targets:
#   t = 0: focal = a0 sp(v) p^2,  f' = a0 p^2 (p + 2 q sp(v)),
#          f'' = a0 [2 p^2 q (p + 2 q sp) + p^2 (p q - 2 p q sp + 2 p q)]
#   with p, q <= 1, p q <= 1/4, q sp(v) <= 0.35, p q sp <= 0.35:  |f'| <= a0 * 1.7,  |f''| <= a0 * 2.3
#   (t = 1 is the mirror image v -> -v with a1).  max(a0, a1) <= 1.  test_segm_train_cpu.py checks both on a grid.
FOCAL_D1, FOCAL_D2 = 1.7, 2.3


# --------------------------------------------------------------------------- fused mask loss
def loss_case(n, h, w, H, W, seed):
    """logits (n, h, w) f32 of a few units (both tails of the sigmoid), target (n, H, W) uint8: row 0 all
    zero, row 1 all one (when n > 1), the rest a filled ellipse."""
    g = gen(seed)
    logits = torch.randn(n, h, w, generator=g) * 3.0
    ys = (torch.arange(H).view(-1, 1) + 0.5) / H
    xs = (torch.arange(W).view(1, -1) + 0.5) / W
    target = torch.zeros(n, H, W, dtype=torch.uint8)
    for r in range(n):
        if r == 0:
            continue
        if r == 1:
            target[r] = 1
            continue
        c = torch.rand(2, generator=g) * 0.4 + 0.3
        a = torch.rand(2, generator=g) * 0.2 + 0.15
        target[r] = ((((ys - c[0]) / a[0]) ** 2 + ((xs - c[1]) / a[1]) ** 2) <= 1).to(torch.uint8)
    return logits, target


def focal_terms(v, t, alpha=ALPHA, gamma=GAMMA):
    """util/misc.py:634-665 per element (no reduction)."""
    prob = v.sigmoid()
    ce = F.binary_cross_entropy_with_logits(v, t, reduction='none')
    p_t = prob * t + (1 - prob) * (1 - t)
    loss = ce * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * t + (1 - alpha) * (1 - t)) * loss
    return loss


def loss_composition(logits64, target, num_boxes):
    """detr.py:779-790 in the dtype of logits64: (loss_mask, loss_dice, sums (n, 4), v)."""
    n = logits64.shape[0]
    H, W = target.shape[1:]
    v = F.interpolate(logits64[:, None], size=(H, W), mode='bilinear', align_corners=False)[:, 0].flatten(1)
    t = target.flatten(1).to(logits64.dtype)
    focal = focal_terms(v, t)
    p = v.sigmoid()
    sums = torch.stack([focal.sum(1), (p * t).sum(1), p.sum(1), t.sum(1)], 1)
    loss_mask = focal.mean(1).sum() / num_boxes if n else logits64.sum() * 0
    dice = 1 - (2 * (p * t).sum(1) + 1) / (p.sum(1) + t.sum(1) + 1)
    loss_dice = dice.sum() / num_boxes
    return loss_mask, loss_dice, sums, v


def _dv(logits, h, w):
    """Bound on the error of one upsampled logit, per row (n, 1): the four products and three sums of the
    bilinear form (6 u M, M = max |logit| of the row) and the f32 source index -- real = scale * (dst + 0.5)
    - 0.5 carries 3 u real <= 3 u `in`, an error of the interpolation weight that moves v by at most that
    times the difference of two logits (<= 2 M); v is continuous across a source pixel, so a floor that
    lands on the other side of an integer changes nothing more.  The f64 reference forms its index in f64."""
    M = logits.double().abs().flatten(1).max(1)[0].view(-1, 1)
    return U32 * M * (6 + 6 * (h + w))


def loss_blocks(H, W):
    return math.ceil(((H * W + 6) // 4) / 1024)


def loss_ref(logits, target, num_boxes):
    """(loss (2,), sums (n, 4), tol_loss (2,), tol_sums (n, 4)) in f64.
    Chain of a row sum: a thread adds up to 16 pixels, then 6 butterfly steps, 3 waves and the row's blocks.
    A term's own error: its derivative w.r.t. v times dv (|focal'| <= FOCAL_D1, |p'| <= 1/4) plus the
    roundings of its evaluation (expf and log1pf at 2 ulp, a division, five products: 12 u |term|)."""
    n, h, w = logits.shape
    H, W = target.shape[1:]
    l64 = logits.double()
    loss_mask, loss_dice, sums, v = loss_composition(l64, target, num_boxes)
    t = target.flatten(1).double()
    focal, p = focal_terms(v, t), v.sigmoid()
    dv = _dv(logits, h, w)
    depth = 16 + 9 + loss_blocks(H, W)
    hw = float(H * W)
    tol_sums = torch.stack([
        depth * U32 * focal.sum(1) + FOCAL_D1 * dv[:, 0] * hw + 12 * U32 * focal.sum(1),
        depth * U32 * (p * t).sum(1) + 0.25 * dv[:, 0] * t.sum(1) + 4 * U32 * (p * t).sum(1),
        depth * U32 * p.sum(1) + 0.25 * dv[:, 0] * hw + 4 * U32 * p.sum(1),
        depth * U32 * t.sum(1)], 1) * SLACK
    # loss[0] = sum_r s0_r / HW / nb: the rows' bounds, two divisions per row and n additions
    tol0 = tol_sums[:, 0].sum() / hw / num_boxes + SLACK * (n + 3) * U32 * loss_mask.abs()
    # loss[1] = sum_r (1 - N_r / D_r) / nb with N = 2 s1 + 1, D = s2 + s3 + 1
    Nn, D = 2 * sums[:, 1] + 1, sums[:, 2] + sums[:, 3] + 1
    d_ratio = 2 * tol_sums[:, 1] / D + Nn / D ** 2 * (tol_sums[:, 2] + tol_sums[:, 3]) + SLACK * 5 * U32 * (Nn / D)
    tol1 = (d_ratio.sum() + SLACK * (n + 3) * U32 * (1 + Nn / D).sum()) / num_boxes
    return (torch.stack([loss_mask, loss_dice]).detach(), sums.detach(), torch.stack([tol0, tol1]).detach(),
            tol_sums.detach())


def loss_backward_ref(logits, target, dloss, num_boxes):
    """(dlogits (n, h, w), tol) in f64: autograd of dloss . (loss_mask, loss_dice) through F.interpolate.
    dlogits[y, x] = sum over the full-resolution pixels i of g_i W_i(y, x) (g = dL/dv, W the bilinear
    weight).  Errors: of g_i -- |dg/dv| dv with |dg/dv| <= gf FOCAL_D2 + |c| / 10 (|(p q)'| <= 0.1), 16 u
    |g_i| for its evaluation, and the dice constants c = gd (N - 2 t D) / D^2 formed from the f32 row sums
    (relative error eps_c, from loss_ref's bounds); of W_i -- the index error 3 u (h + w) (see _dv) on
    every pixel of the gather window, at most (2 ceil(H/h) + 5)(2 ceil(W/w) + 5) pixels of at most
    max |g|; and the chain of the gather, the window's length, times u sum |g_i| W_i."""
    n, h, w = logits.shape
    H, W = target.shape[1:]
    l64 = logits.double().requires_grad_(True)
    loss_mask, loss_dice, sums, v = loss_composition(l64, target, num_boxes)
    v.retain_grad()
    (dloss[0].double() * loss_mask + dloss[1].double() * loss_dice).backward()
    ref, g = l64.grad.detach(), v.grad.detach().abs().view(n, H, W)
    _, _, _, tol_sums = loss_ref(logits, target, num_boxes)
    sums = sums.detach()
    D = sums[:, 2] + sums[:, 3] + 1
    Nn = 2 * sums[:, 1] + 1
    gf = dloss[0].abs().double() / (H * W) / num_boxes
    gd = dloss[1].abs().double() / num_boxes
    c_abs = gd * (Nn + 2 * D) / D ** 2                                                  # >= |c0|, |c1|
    d_c = gd * ((2 * tol_sums[:, 1] + 2 * (tol_sums[:, 2] + tol_sums[:, 3])) / D ** 2
                + 2 * (Nn + 2 * D) / D ** 3 * (tol_sums[:, 2] + tol_sums[:, 3])) + SLACK * 6 * U32 * c_abs
    dv = _dv(logits, h, w)[:, 0]
    per_pixel = ((gf * FOCAL_D2 + c_abs * 0.1) * dv + d_c * 0.25).view(n, 1, 1) + 16 * U32 * g
    ky, kx = 2 * math.ceil(H / h) + 5, 2 * math.ceil(W / w) + 5
    z = torch.zeros(n, h, w, dtype=torch.float64, requires_grad=True)
    up = F.interpolate(z[:, None], size=(H, W), mode='bilinear', align_corners=False)[:, 0]
    (up * (per_pixel + ky * kx * U32 * g)).sum().backward()                             # sum_i W_i (.)
    window = 3 * U32 * (h + w) * ky * kx * g.flatten(1).max(1)[0].view(n, 1, 1)
    return ref, SLACK * (z.grad + window)


# --------------------------------------------------------------------------- attention map backward
def attention_backward_case(B, Q, h, w, d, seed, masked_cols=0):
    g = gen(seed)
    qp = torch.randn(B * Q, d, generator=g) * 1.5
    kp = torch.randn(B, h * w, d, generator=g) * 1.5
    datt = torch.randn(B * Q, h * w, HEADS, generator=g)
    mask = torch.zeros(B, h, w, dtype=torch.bool)
    if masked_cols:
        mask[B - 1, :, w - masked_cols:] = True
    return qp, kp, datt, mask.flatten(1)


def attention_backward_ref(qp, kp, datt, mask, Q, heads=HEADS):
    """(att f64, dqp, dkp, tol_q, tol_k): autograd of sum(att * datt) through the joint softmax in f64.
    The kernel reads att rounded to f32 (u att).  s = sum att datt over T = ceil(HW heads / 256) terms a
    thread + 9 merges; dl = att (datt - s) then errs by att (ds + 3 u (|datt| + |s|)); dqp sums HW
    products, dkp Q products."""
    B, HW, d = kp.shape
    D = d // heads
    scale = float(D) ** -0.5
    q64 = qp.double().requires_grad_(True)
    k64 = kp.double().requires_grad_(True)
    logits = torch.einsum('bqnc,bpnc->bqpn', q64.view(B, Q, heads, D) * scale, k64.view(B, HW, heads, D))
    logits = logits.masked_fill(mask.view(B, 1, HW, 1), float('-inf'))
    att = torch.softmax(logits.flatten(2), -1).view(B * Q, HW, heads)
    (att * datt.double()).sum().backward()
    a, g = att.detach(), datt.double()
    s = (a * g).sum((1, 2), keepdim=True)
    T = math.ceil(HW * heads / 256)
    ds = (T + 11) * U32 * (a * g).abs().sum((1, 2), keepdim=True)
    dl = (a * (g - s)).abs()
    ddl = a * (ds + 3 * U32 * (g.abs() + s.abs()))
    ka = kp.double().abs().view(B, 1, HW, heads, D)
    qa = qp.double().abs().view(B, Q, 1, heads, D)
    e = (ddl + (HW + 2) * U32 * dl).view(B, Q, HW, heads, 1)
    tol_q = scale * (e * ka).sum(2).reshape(B * Q, d)
    e = (ddl + (Q + 2) * U32 * dl).view(B, Q, HW, heads, 1)
    tol_k = scale * (e * qa).sum(1).reshape(B, HW, d)
    return a, q64.grad, k64.grad, SLACK * tol_q, SLACK * tol_k


# --------------------------------------------------------------------------- ReLU + upsample + add
def relu_up_add_case(B, Q, h, w, H, W, C, seed, with_f=True):
    g = gen(seed)
    x = torch.randn(B * Q, h, w, C, generator=g)
    f = torch.randn(B, H, W, C, generator=g) if with_f else None
    dy = torch.randn(B * Q, H, W, C, generator=g)
    return x, f, dy


def relu_up_add_ref(x, f, dy, Q, H, W):
    """(y, dx, df, tol_y, tol_dx, tol_df) in f64 by autograd over relu -> legacy-nearest index -> add.
    y is one addition; dx sums its children (at most (ceil(H/h) + 1)(ceil(W/w) + 1)), df the frame's Q rows."""
    R, h, w, C = x.shape
    iy, ix = nearest_index(h, H), nearest_index(w, W)
    x64 = x.double().requires_grad_(True)
    f64 = f.double().requires_grad_(True) if f is not None else None

    def run(xx, ff):
        y = torch.relu(xx)[:, iy][:, :, ix]
        return y if ff is None else y + ff.repeat_interleave(Q, 0)
    y = run(x64, f64)
    y.backward(dy.double())
    xa = torch.ones_like(x64).requires_grad_(True)          # every child counted: the sum of |dy| over them
    fa = torch.zeros_like(f64).requires_grad_(True) if f is not None else None
    run(xa, fa).backward(dy.double().abs())
    kids = (math.ceil(H / h) + 1) * (math.ceil(W / w) + 1)
    tol_dx = SLACK * kids * U32 * xa.grad
    tol_df = SLACK * Q * U32 * fa.grad if f is not None else None
    return (y.detach(), x64.grad, f64.grad if f is not None else None, SLACK * U32 * y.detach().abs(), tol_dx,
            tol_df)


# --------------------------------------------------------------------------- out_lay backward
def out_backward_case(R, H, W, C, seed):
    g = gen(seed)
    x = torch.randn(R, H, W, C, generator=g).clamp(min=0)
    weight = torch.randn(1, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    dy = torch.randn(R, H, W, generator=g)
    return x, weight, dy


def out_backward_ref(x, weight, dy):
    """(dx (R, H, W, C), dw (1, C, 3, 3), db (1,), and their bounds) by autograd through F.conv2d in f64.
    dx: nine products.  dw / db: a block owns max(1024, ceil(P / 2048)) of the P = R H W pixels, a thread
    every (256 // C)-th of them, then the 256 // C lanes and the blocks in order."""
    R, H, W, C = x.shape

    def grads(xx, ww, gg):
        xx = xx.permute(0, 3, 1, 2).requires_grad_(True)
        ww = ww.clone().requires_grad_(True)
        b = torch.zeros(1, dtype=torch.float64, requires_grad=True)
        F.conv2d(xx, ww, b, padding=1)[:, 0].backward(gg)
        return xx.grad.permute(0, 2, 3, 1).contiguous(), ww.grad, b.grad
    dx, dw, db = grads(x.double(), weight.double(), dy.double())
    ax, aw, ab = grads(x.double().abs(), weight.double().abs(), dy.double().abs())
    P = R * H * W
    ppb = max(1024, math.ceil(P / 2048))
    PP = 256 // C
    depth = math.ceil(ppb / PP) + PP + math.ceil(P / ppb) + 2
    return dx, dw, db, SLACK * 10 * U32 * ax, SLACK * depth * U32 * aw, SLACK * depth * U32 * ab


# --------------------------------------------------------------------------- the training-step fixture
# tests/golden/make_golden_segm_train.py -> segm_train.npz: case A of make_golden_segm.py (non-tracking),
# dropout 0, 2 encoder / 3 decoder layers, 12 queries, train mode.  3x106x202 and 3x90x138: the stride-4
# map is 27x51 (not H / 4), the second frame is padded, and the loss upsamples 27x51 -> 106x202 (~3.93x).
TRAIN_FRAMES = ((4201, 106, 202), (4202, 90, 138))       # (generator seed, H, W)
TRAIN_BOXES = (((0.30, 0.40, 0.30, 0.45), (0.70, 0.55, 0.35, 0.50), (0.50, 0.25, 0.50, 0.30)),
               ((0.35, 0.50, 0.40, 0.60), (0.72, 0.40, 0.30, 0.40)))       # cxcywh, inside the image
TRAIN_OVER = dict(dropout=0.0, enc_layers=2, dec_layers=3)
TRAIN_DETECTOR_GRADS = ('transformer.decoder.layers.2.linear2.weight', 'transformer.encoder.layers.1.linear2.weight',
                        'input_proj.1.0.weight', 'backbone.0.body.layer3.0.conv2.weight')
GRAD_GATE, GRAD_GATE_BACKBONE, GRAD_ATOL = 2e-3, 5e-3, 1e-5               # tests/test_train_gpu.py's gates
LATTICE_MAX = 8192      # a gradient with more elements is stored on flatten()[::ceil(numel / LATTICE_MAX)]


def ellipse_masks(boxes, H, W):
    """uint8 (n, H, W): the ellipse inscribed in each cxcywh box (normalised to the H x W frame)."""
    ys = (torch.arange(H, dtype=torch.float64).view(1, -1, 1) + 0.5) / H
    xs = (torch.arange(W, dtype=torch.float64).view(1, 1, -1) + 0.5) / W
    b = torch.as_tensor(boxes, dtype=torch.float64)
    cx, cy, bw, bh = (b[:, i].view(-1, 1, 1) for i in range(4))
    return ((((xs - cx) / (bw / 2)) ** 2 + ((ys - cy) / (bh / 2)) ** 2) <= 1).to(torch.uint8)


def train_targets(dtype=torch.float32):
    out = []
    for (_, H, W), boxes in zip(TRAIN_FRAMES, TRAIN_BOXES):
        out.append({'boxes': torch.tensor(boxes, dtype=dtype), 'labels': torch.zeros(len(boxes), dtype=torch.long),
                    'masks': ellipse_masks(boxes, H, W)})
    return out


def train_frames(dtype=torch.float32):
    return [torch.randn(3, h, w, generator=gen(s)).to(dtype) for s, h, w in TRAIN_FRAMES]


def lattice(t):
    """The stored part of a gradient: all of it up to LATTICE_MAX elements, else an evenly strided lattice
    of its flattened elements (its L2 norm is stored beside it)."""
    flat = t.detach().reshape(-1)
    return flat[::max(1, math.ceil(flat.numel() / LATTICE_MAX))]


def grad_gate(name, ref_max):
    return (GRAD_GATE_BACKBONE if 'backbone' in name else GRAD_GATE) * ref_max + GRAD_ATOL
