"""Direct tests of the kernels of csrc/criterion.hip against f64 references (tests/two_stage_train_refs.py),
each at the smallest shapes that reach its edges.

Tolerances are the operation-count bounds derived beside the references (match_cost_ref, focal_set_ref):
they are formed from the f64 values only.  Both numbers per kernel, measured on MI355X (the tests print them):
  cost   (2, 2380, 1) x [5, 7] and (2, 257, 91) x [5, 7]: bound at most 4.9e-5 on costs of magnitude up to ~20; the
         kernel sits 3.5e-6 from f64 (at most 0.13 of the bound on any element), the torch composition it
         replaces 1.6e-3 .. 5.3e-3 (it forms 1 - p by subtraction under the log);
  focal  (4760, 91): bound 8e-6 of the loss and 24 u of each gradient element; the kernel sits 5e-8 of the loss
         and at most 0.22 of the gradient bound from f64, the torch composition 5e-8 of the loss as well.
"""
import pytest
import torch

import two_stage_train_refs as T

pytestmark = pytest.mark.gpu
W = (2.0, 5.0, 2.0)      # class, bbox, giou: the deformable configs' set_cost_*


def _start(sizes):
    return torch.tensor([0] + torch.tensor(sizes).cumsum(0).tolist(), dtype=torch.int32).cuda()


def _cost(logits, boxes, labels, tboxes, sizes, want_check=True):
    from kinet_amd import kernels as K
    cost, ok = K.match_cost_focal(logits.cuda(), boxes.cuda(), labels.cuda(), tboxes.cuda(), _start(sizes), *W,
                                  alpha=T.ALPHA, gamma=T.GAMMA, want_check=want_check)
    torch.cuda.synchronize()
    return cost.cpu(), (None if ok is None else bool(ok.cpu()))


def _composition_cost(logits, boxes, labels, tboxes, sizes):
    from kinet_amd.models.matcher import HungarianMatcher
    m = HungarianMatcher(*W, focal_loss=True, focal_alpha=T.ALPHA, focal_gamma=T.GAMMA)
    targets, o = [], 0
    for n in sizes:
        targets.append({'labels': labels[o:o + n], 'boxes': tboxes[o:o + n]})
        o += n
    full = m.cost_matrix({'pred_logits': logits, 'pred_boxes': boxes}, targets)
    return torch.cat([full[b][:, o:o + n] for b, (o, n) in
                      enumerate(zip([0] + torch.tensor(sizes).cumsum(0).tolist()[:-1], sizes))], 1)


@pytest.mark.parametrize('B,Q,C,sizes', [(1, 1, 1, [1]), (1, 1, 1, [0]), (3, 63, 20, [3, 0, 2]), (2, 257, 91, [5, 7]),
                                         (2, 2380, 1, [5, 7])])
def test_match_cost_against_f64(B, Q, C, sizes):
    logits, boxes, labels, tboxes = T.cost_case(B, Q, C, sizes, seed=100 + Q + C)
    ref, tol = T.match_cost_ref(logits, boxes, labels, tboxes, sizes, *W)
    got, ok = _cost(logits, boxes, labels, tboxes, sizes)
    assert got.shape == (Q, sum(sizes)) and got.dtype == torch.float32
    assert ok is True
    if sum(sizes) == 0:
        return
    err = (got.double() - ref).abs()
    comp = (_composition_cost(logits, boxes, labels, tboxes, sizes).double() - ref).abs().max().item()
    print(f'[cost] {(B, Q, C)} x {sizes}: max err {err.max().item():.3e} (bound max {tol.max().item():.3e}, worst '
          f'err / bound {(err / tol).max().item():.3f}); the torch composition: {comp:.3e}')
    assert (err <= tol).all()


def test_match_cost_edges():
    """A row of exact (1, 1, 1, 1) boxes (the reference's value on every invalid proposal), logits of +-100,
    an image without targets in the middle, Q not a multiple of the workgroup's 16 rows."""
    B, Q, C, sizes = 3, 37, 2, [3, 0, 2]
    logits, boxes, labels, tboxes = T.cost_case(B, Q, C, sizes, seed=7)
    boxes[0, 5] = 1.0
    boxes[2, 36] = 1.0
    boxes[1] = 1.0
    logits[0, 1] = 100.0
    logits[0, 2] = -100.0
    logits[2, 35] = torch.tensor([100.0, -100.0])
    ref, tol = T.match_cost_ref(logits, boxes, labels, tboxes, sizes, *W)
    got, ok = _cost(logits, boxes, labels, tboxes, sizes)
    assert ok is True and torch.isfinite(got).all()
    assert ((got.double() - ref).abs() <= tol).all()
    # without the flag byte: the same costs
    again, none = _cost(logits, boxes, labels, tboxes, sizes, want_check=False)
    assert none is None and torch.equal(again, got)


@pytest.mark.parametrize('where', ['prediction', 'prediction_of_image_without_targets', 'target', 'nan'])
def test_match_cost_degenerate_box_byte(where):
    B, Q, C, sizes = 3, 40, 3, [3, 0, 2]
    logits, boxes, labels, tboxes = T.cost_case(B, Q, C, sizes, seed=9)
    assert _cost(logits, boxes, labels, tboxes, sizes)[1] is True
    if where == 'prediction':
        boxes[2, 39, 2] = -0.01            # x1 < x0
    elif where == 'prediction_of_image_without_targets':
        boxes[1, 17, 3] = -0.5             # y1 < y0 (the reference checks every prediction box)
    elif where == 'target':
        tboxes[4, 3] = -0.2
    else:
        boxes[0, 0, 0] = float('nan')
    assert T.boxes_ok_ref(boxes, tboxes) is False
    assert _cost(logits, boxes, labels, tboxes, sizes)[1] is False


def test_match_cost_rejects_bad_arguments():
    from kinet_amd import kernels as K
    logits, boxes, labels, tboxes = (t.cuda() for t in T.cost_case(2, 8, 3, [1, 2], seed=1))
    st = _start([1, 2])
    with pytest.raises(RuntimeError, match='f32'):
        K.match_cost_focal(logits.half(), boxes, labels, tboxes, st, *W)
    with pytest.raises(RuntimeError, match='f32'):
        K.match_cost_focal(logits, boxes[:, :7], labels, tboxes, st, *W)
    with pytest.raises(RuntimeError, match='int32'):
        K.match_cost_focal(logits, boxes, labels, tboxes, st.long(), *W)
    with pytest.raises(RuntimeError, match='int32'):
        K.match_cost_focal(logits, boxes, labels.int(), tboxes, st, *W)
    with pytest.raises(RuntimeError, match='gamma'):
        K.match_cost_focal(logits, boxes, labels, tboxes, st, *W, gamma=-1.0)
    with pytest.raises(RuntimeError, match='GPU only'):
        K.match_cost_focal(logits.cpu(), boxes, labels, tboxes, st, *W)


# --------------------------------------------------------------------------- focal set loss
def _focal_case(R, C, n, seed, scale=3.0):
    g = T.gen(seed)
    logits = torch.randn(R, C, generator=g) * scale
    rows = torch.randperm(R, generator=g)[:n]
    cls = torch.randint(0, C, (n,), generator=g)
    return logits, rows, cls


def _composition_focal(logits, rows, cls, num_boxes):
    """loss_labels_focal's arithmetic (one-hot, sigmoid_focal_loss) in the dtype of logits."""
    from kinet_amd.models.criterion import sigmoid_focal_loss
    x = logits.clone().requires_grad_(True)
    onehot = torch.zeros_like(logits)
    onehot[rows, cls] = 1
    loss = sigmoid_focal_loss(x[None], onehot[None], num_boxes, alpha=T.ALPHA, gamma=T.GAMMA) * logits.shape[0]
    loss.backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize('R', [1, 255, 4760])
@pytest.mark.parametrize('C', [1, 20, 91])
@pytest.mark.parametrize('n', [0, 1, 5])
def test_focal_set_loss_against_f64(R, C, n):
    from kinet_amd import kernels as K
    n = min(n, R)
    logits, rows, cls = _focal_case(R, C, n, seed=R + 7 * C + n)
    num_boxes, dloss = 5.0, 0.7
    ref, tol, gref, gtol = T.focal_set_ref(logits, rows, cls, num_boxes, dloss=dloss)
    lg, r, c = logits.cuda(), rows.cuda(), cls.cuda()
    got = K.focal_set_loss(lg, r, c, num_boxes, T.ALPHA, T.GAMMA)
    d = K.focal_set_loss_backward(lg, r, c, torch.tensor([dloss]).cuda(), num_boxes, T.ALPHA, T.GAMMA)
    again = K.focal_set_loss(lg, r, c, num_boxes, T.ALPHA, T.GAMMA)
    d_again = K.focal_set_loss_backward(lg, r, c, torch.tensor([dloss]).cuda(), num_boxes, T.ALPHA, T.GAMMA)
    torch.cuda.synchronize()
    assert got.shape == () and d.shape == (R, C)
    assert torch.equal(got, again) and torch.equal(d, d_again)            # fixed-order sums: bit-equal reruns
    err = abs(got.item() - ref.item())
    gerr = (d.cpu().double() - gref).abs()
    c32, cg32 = _composition_focal(logits, rows, cls, num_boxes)
    print(f'[focal] R {R} C {C} n {n}: loss {ref.item():.6g} err {err:.3e} (bound {tol.item():.3e}); grad worst err / '
          f'bound {(gerr / gtol).max().item():.3f}; the torch composition: loss {abs(c32.item() - ref.item()):.3e}, '
          f'grad {(cg32.double() * dloss - gref).abs().max().item():.3e}')
    assert err <= tol.item()
    assert (gerr <= gtol).all()


def test_focal_set_loss_extreme_logits_are_finite():
    """+-100 everywhere, positives at both signs; every positive in one workgroup's range and more of them
    than the workgroup keeps in LDS (64), so the search of the global list runs too."""
    from kinet_amd import kernels as K
    R, C = 300, 4
    logits = torch.full((R, C), 100.0)
    logits[::2] = -100.0
    rows = torch.arange(0, 140, 2)                                         # 70 positives, rows even and odd below
    rows = torch.cat([rows, torch.tensor([1, 3])])
    cls = torch.arange(rows.numel()) % C
    ref, tol, gref, gtol = T.focal_set_ref(logits, rows, cls, 2.0)
    got = K.focal_set_loss(logits.cuda(), rows.cuda(), cls.cuda(), 2.0)
    d = K.focal_set_loss_backward(logits.cuda(), rows.cuda(), cls.cuda(), torch.ones(1).cuda(), 2.0)
    torch.cuda.synchronize()
    assert torch.isfinite(got) and torch.isfinite(d).all()
    assert abs(got.item() - ref.item()) <= tol.item()
    assert ((d.cpu().double() - gref).abs() <= gtol).all()


def test_focal_set_loss_autograd_and_shapes():
    """A.focal_set_loss on (B, S, C) logits, gradient through the Function; a general gamma and alpha < 0."""
    from kinet_amd import autograd as A
    B, S, C = 2, 131, 3
    logits, rows, cls = _focal_case(B * S, C, 4, seed=3)
    for alpha, gamma in ((T.ALPHA, T.GAMMA), (-1.0, 1.5), (0.4, 0.0)):
        ref, tol, gref, gtol = T.focal_set_ref(logits, rows, cls, 3.0, alpha, gamma, dloss=2.0)
        x = logits.view(B, S, C).cuda().requires_grad_(True)
        loss = A.focal_set_loss(x, rows.cuda(), cls.cuda(), 3.0, alpha, gamma)
        (loss * 2.0).backward()
        torch.cuda.synchronize()
        assert abs(loss.item() - ref.item()) <= 4 * tol.item()              # (powf: a few ulp more than a product)
        assert ((x.grad.view(-1, C).cpu().double() - gref).abs() <= 4 * gtol).all()


def test_focal_set_loss_rejects_bad_arguments():
    from kinet_amd import kernels as K
    logits, rows, cls = (t.cuda() for t in _focal_case(16, 4, 2, seed=1))
    with pytest.raises(RuntimeError, match='f32'):
        K.focal_set_loss(logits.half(), rows, cls, 1.0)
    with pytest.raises(RuntimeError, match='int64'):
        K.focal_set_loss(logits, rows.int(), cls, 1.0)
    with pytest.raises(RuntimeError, match='one length'):
        K.focal_set_loss(logits, rows, cls[:1], 1.0)
    with pytest.raises(RuntimeError, match='gamma'):
        K.focal_set_loss(logits, rows, cls, 1.0, gamma=-2.0)
    with pytest.raises(RuntimeError, match='num_boxes'):
        K.focal_set_loss(logits, rows, cls, -1.0)
    with pytest.raises(RuntimeError, match='one f32'):
        K.focal_set_loss_backward(logits, rows, cls, torch.ones(2).cuda(), 1.0)
    # a pair outside the matrix is ignored, not dereferenced
    far = torch.tensor([10 ** 9, -1]).cuda()
    a = K.focal_set_loss(logits, far, cls, 1.0)
    b = K.focal_set_loss(logits, rows[:0], cls[:0], 1.0)
    assert torch.equal(a, b)


# --------------------------------------------------------------------------- proposal-stage glue
@pytest.mark.parametrize('keep_kind', ['none', 'all', 'mixed'])
def test_mask_rows(keep_kind):
    from kinet_amd import autograd as A
    g = T.gen(4)
    x = torch.randn(3, 515, 256, generator=g)
    x[0, 3] = float('nan')                 # a dropped row is exactly 0 whatever it holds
    x[1, 7, 5] = float('inf')
    keep = {'none': torch.zeros(3, 515), 'all': torch.ones(3, 515), 'mixed': (torch.rand(3, 515, generator=g) < 0.7).float()}[keep_kind]
    keep = keep.to(torch.uint8)
    if keep_kind == 'mixed':
        keep[0, 3], keep[1, 7] = 0, 0
    if keep_kind == 'all':
        x = torch.nan_to_num(x, nan=1.0, posinf=2.0)
    xc = x.cuda().requires_grad_(True)
    y = A.two_stage_mask_rows(xc, keep.cuda())
    dy = torch.randn(3, 515, 256, generator=g)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    k = keep.bool().unsqueeze(-1)
    zero = torch.zeros(())
    assert torch.equal(y.detach().cpu(), torch.where(k, x, zero))
    assert torch.equal(xc.grad.cpu(), torch.where(k, dy, zero))


def test_two_stage_boxes_backward():
    """d_tmp = d_boxes b (1 - b) + d_coord_unact against f64 autograd of sigmoid(tmp + proposals); the +inf
    proposals' rows get exactly 0 and no NaN, also where the incoming gradient is inf or NaN."""
    from kinet_amd import autograd as A
    from kinet_amd import kernels as K
    g = T.gen(10)
    tmp = torch.randn(2, 515, 4, generator=g)
    prop = torch.randn(2, 515, 4, generator=g)
    prop[0, 7] = float('inf')
    prop[1, ::5] = float('inf')
    d_boxes = torch.randn(2, 515, 4, generator=g)
    d_unact = torch.randn(2, 515, 4, generator=g)
    t = tmp.cuda().requires_grad_(True)
    unact, boxes = A.two_stage_boxes(t, prop.cuda())
    (boxes * d_boxes.cuda()).sum().backward()
    torch.cuda.synchronize()
    t64 = tmp.double().requires_grad_(True)
    b64 = torch.sigmoid(t64 + prop.double())
    (b64 * d_boxes.double()).sum().backward()
    inf_rows = torch.isinf(prop)
    assert (t.grad.cpu()[inf_rows] == 0).all() and not torch.isnan(t.grad).any()
    # b (1 - b): the forward's b carries 4 u and the rounding of x = tmp + proposals (u |x| on the argument, as
    # much relative on b (1 - b)); 1 - b is one rounding of a value whose error is 4 u b -> relative
    # (4 u b) / (1 - b) + u; two products
    b = b64.detach()
    x = torch.nan_to_num((tmp.double() + prop.double()).abs(), posinf=0.0)
    tol = T.SLACK * T.U32 * d_boxes.double().abs() * (b * (1 - b) * (8 + x) + 4 * b * b) + T.TINY
    err = (t.grad.cpu().double() - t64.grad).abs()
    print(f'[boxes bwd] worst err / bound {(err / tol)[~inf_rows].max().item():.3f}')
    assert (err[~inf_rows] <= tol[~inf_rows]).all()
    # both gradients, either alone, and hostile incoming values on the +inf rows
    bx = boxes.detach()
    both = K.two_stage_boxes_backward(d_boxes.cuda(), d_unact.cuda(), bx)
    only_u = K.two_stage_boxes_backward(None, d_unact.cuda(), bx)
    only_b = K.two_stage_boxes_backward(d_boxes.cuda(), None, bx)
    assert torch.equal(only_u.cpu(), d_unact) and torch.equal(only_b, t.grad)
    assert ((both.cpu().double() - (only_b.cpu().double() + d_unact.double())).abs() <= T.U32 * both.cpu().abs().double()).all()
    bad = d_boxes.clone()
    bad[0, 7] = float('inf')
    bad[1, 0] = float('nan')
    out = K.two_stage_boxes_backward(bad.cuda(), None, bx).cpu()
    assert (out[inf_rows] == 0).all() and not torch.isnan(out).any()
    with pytest.raises(RuntimeError, match='both'):
        K.two_stage_boxes_backward(None, None, bx)
