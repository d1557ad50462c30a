"""Direct tests of the mask-training kernels (csrc/segm_train.hip, include/kinet_segm.h): each runs one
kernel against torch autograd in double on the CPU over the plain composition of the same inputs
(tests/segm_train_refs.py, with the bounds' derivation), at the smallest shapes that reach every
path: exact 4x, identity, non-integer (~3.93x) and just-above-1x loss upsampling, more than one
block per row, target rows that start at every byte of a 4-byte word, an all-zero and an all-one
target, a padded second frame, rows split over calls.  Every kernel is also rerun: the same bits."""
import pytest
import torch

import segm_refs as R
import segm_train_refs as T

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


# --------------------------------------------------------------------------- fused mask loss
LOSS_SHAPES = [(h, w, H, W) for (h, w) in ((7, 13), (27, 51)) for (H, W) in ((28, 52), (27, 51), (106, 202), (29, 53))]
LOSS_IDS = [f'{h}x{w}-to-{H}x{W}' for h, w, H, W in LOSS_SHAPES]     # 4x, identity, 3.93x, 1.07x among them


@pytest.mark.parametrize('h,w,H,W', LOSS_SHAPES, ids=LOSS_IDS)
def test_mask_loss_forward_backward(K, h, w, H, W):
    n, num_boxes = 3, 2.5
    logits, target = T.loss_case(n, h, w, H, W, seed=31)
    assert target[0].sum() == 0 and target[1].all() and 0 < target[2].sum() < H * W
    ref, ref_sums, tol, tol_sums = T.loss_ref(logits, target, num_boxes)
    lg, tg = logits.cuda(), target.cuda()
    loss, sums = K.segm_mask_loss(lg, tg, num_boxes)
    assert loss.shape == (2,) and sums.shape == (n, 4) and loss.dtype == F32
    e_s = R.within(sums, ref_sums, tol_sums, F32, ('mask loss sums', h, w, H, W))
    e_l = R.within(loss, ref, tol, F32, ('mask loss', h, w, H, W))
    assert sums[0, 3] == 0 and sums[0, 1] == 0 and sums[1, 3] == H * W       # the counts are exact
    loss2, sums2 = K.segm_mask_loss(lg, tg, num_boxes)
    assert torch.equal(loss, loss2) and torch.equal(sums, sums2)
    print(f'mask_loss {h}x{w}->{H}x{W}: loss {ref.tolist()}, err {e_l:.3e} (bound {tol.tolist()}), sums err {e_s:.3e}')
    # backward, with two different weights on the two losses
    dloss = torch.tensor([0.7, -1.3])
    dref, dtol = T.loss_backward_ref(logits, target, dloss, num_boxes)
    assert dref.abs().max() > 0
    d = K.segm_mask_loss_backward(lg, tg, sums, dloss.cuda(), num_boxes)
    assert d.shape == (n, h, w)
    e_d = R.within(d, dref, dtol, F32, ('mask loss backward', h, w, H, W))
    assert torch.equal(d, K.segm_mask_loss_backward(lg, tg, sums, dloss.cuda(), num_boxes))
    print(f'mask_loss_backward {h}x{w}->{H}x{W}: max |ref| {dref.abs().max():.3e}, err {e_d:.3e}, '
          f'bound at worst element {dtol.max():.3e}')


def test_mask_loss_rows_at_every_byte_offset(K):
    """H*W = 29*53 is odd, so rows 0..3 of a contiguous target start at all four bytes of a word: the
    aligned 32-bit loads and the byte-wise row ends must tile each row exactly once."""
    n, h, w, H, W = 5, 7, 13, 29, 53
    logits, target = T.loss_case(n, h, w, H, W, seed=32)
    assert len({(r * H * W) % 4 for r in range(n)}) == 4
    _, ref_sums, _, tol_sums = T.loss_ref(logits, target, 1.0)
    _, sums = K.segm_mask_loss(logits.cuda(), target.cuda(), 1.0)
    R.within(sums, ref_sums, tol_sums, F32, 'byte offsets')
    assert torch.equal(sums[:, 3].cpu(), target.flatten(1).sum(1).float())


def test_mask_loss_no_rows(K):
    logits = torch.empty(0, 7, 13, device='cuda')
    target = torch.empty(0, 28, 52, dtype=torch.uint8, device='cuda')
    loss, sums = K.segm_mask_loss(logits, target, 1.0)
    assert loss.tolist() == [0.0, 0.0] and sums.shape == (0, 4)
    d = K.segm_mask_loss_backward(logits, target, sums, torch.ones(2, device='cuda'), 1.0)
    assert d.shape == (0, 7, 13)


def test_mask_loss_argument_errors(K):
    logits, target = T.loss_case(2, 7, 13, 28, 52, seed=33)
    with pytest.raises(RuntimeError, match='gamma'):
        K.segm_mask_loss(logits.cuda(), target.cuda(), 1.0, gamma=1.5)
    with pytest.raises(RuntimeError, match='at least'):      # downsampling is not the loss's direction
        K.segm_mask_loss(logits.cuda(), target[:, :6, :12].contiguous().cuda(), 1.0)
    with pytest.raises(RuntimeError, match='GPU'):
        K.segm_mask_loss(logits, target, 1.0)


def test_mask_loss_function_autograd(K):
    """autograd.segm_mask_loss wires the two kernels: the gradient of a weighted sum of the two scalars."""
    from kinet_amd import autograd as A
    logits, target = T.loss_case(3, 7, 13, 28, 52, seed=34)
    dloss = torch.tensor([2.0, 0.5])
    dref, dtol = T.loss_backward_ref(logits, target, dloss, 4.0)
    lg = logits.cuda().requires_grad_(True)
    lm, ld = A.segm_mask_loss(lg, target.cuda(), 4.0)
    (2.0 * lm + 0.5 * ld).backward()
    R.within(lg.grad, dref, dtol, F32, 'segm_mask_loss Function')


# --------------------------------------------------------------------------- attention map backward
@pytest.mark.parametrize('Q', [5, 3])
def test_attention_backward(K, Q):
    B, h, w, d = 2, 7, 13, 256
    qp, kp, datt, mask = T.attention_backward_case(B, Q, h, w, d, seed=41, masked_cols=4)
    att, dq, dk, tol_q, tol_k = T.attention_backward_ref(qp, kp, datt, mask, Q)
    att32 = att.float().cuda()
    gq, gk = K.segm_attention_backward(datt.cuda(), att32, qp.cuda(), kp.cuda(), Q, R.HEADS)
    e_q = R.within(gq, dq, tol_q, F32, 'attention dqp')
    e_k = R.within(gk, dk, tol_k, F32, 'attention dkp')
    m = mask.view(B, h * w)
    assert m[1].sum() == 4 * h and (gk.cpu()[m] == 0).all() and (dk[m] == 0).all()      # masked pixels: exactly 0
    assert (gk.cpu()[~m] != 0).any()
    gq2, gk2 = K.segm_attention_backward(datt.cuda(), att32, qp.cuda(), kp.cuda(), Q, R.HEADS)
    assert torch.equal(gq, gq2) and torch.equal(gk, gk2)
    only_q, none_k = K.segm_attention_backward(datt.cuda(), att32, qp.cuda(), kp.cuda(), Q, R.HEADS, need_k=False)
    assert none_k is None and torch.equal(only_q, gq)
    print(f'attention_backward Q={Q}: dqp err {e_q:.3e} (max {dq.abs().max():.3e}), dkp err {e_k:.3e} '
          f'(max {dk.abs().max():.3e})')


# --------------------------------------------------------------------------- ReLU + upsample + add
@pytest.mark.parametrize('h,w,H,W,C,with_f', [(7, 13, 13, 25, 64, True), (13, 25, 26, 50, 32, True),
                                              (13, 25, 13, 25, 16, False)], ids=['7x13-up', '13x25-up', 'identity'])
def test_relu_up_add(K, h, w, H, W, C, with_f):
    B, Q = 2, 3
    x, f, dy = T.relu_up_add_case(B, Q, h, w, H, W, C, seed=51, with_f=with_f)
    y, dx, df, tol_y, tol_dx, tol_df = T.relu_up_add_ref(x, f, dy, Q, H, W)
    xg, fg, dyg = x.cuda(), f.cuda() if with_f else None, dy.cuda()
    got = K.segm_relu_up_add(xg, fg, 0, Q)
    R.within(got, y, tol_y, F32, 'relu_up_add')
    gdx, gdf = K.segm_relu_up_add_backward(dyg, xg, tuple(f.shape) if with_f else None, 0, Q)
    e_x = R.within(gdx, dx, tol_dx, F32, 'relu_up_add dx')
    assert (gdx.cpu()[x <= 0] == 0).all()
    if with_f:
        e_f = R.within(gdf, df, tol_df, F32, 'relu_up_add df')
    else:
        assert gdf is None
        e_f = 0.0
    # rows in two chunks (the second starts inside frame 0): the same y and dx bits; df adds over the chunks
    cut = 2
    y2 = torch.cat([K.segm_relu_up_add(xg[:cut], fg, 0, Q), K.segm_relu_up_add(xg[cut:], fg, cut, Q)])
    assert torch.equal(got, y2)
    a = K.segm_relu_up_add_backward(dyg[:cut], xg[:cut], tuple(f.shape) if with_f else None, 0, Q)
    b = K.segm_relu_up_add_backward(dyg[cut:], xg[cut:], tuple(f.shape) if with_f else None, cut, Q)
    assert torch.equal(torch.cat([a[0], b[0]]), gdx)
    if with_f:
        R.within(a[1] + b[1], df, tol_df + R.U32 * df.abs(), F32, 'relu_up_add df in chunks')
        assert torch.equal(a[1][1], torch.zeros_like(a[1][1]))              # no row of frame 1 in the first chunk
    r = K.segm_relu_up_add_backward(dyg, xg, tuple(f.shape) if with_f else None, 0, Q)
    assert torch.equal(r[0], gdx) and (not with_f or torch.equal(r[1], gdf))
    print(f'relu_up_add {h}x{w}->{H}x{W} C={C}: dx err {e_x:.3e}, df err {e_f:.3e}')


# --------------------------------------------------------------------------- out_lay backward
def test_out_conv_backward(K):
    rows, H, W, C = 5, 26, 50, 16
    x, weight, dy = T.out_backward_case(rows, H, W, C, seed=61)
    dx, dw, db, tol_x, tol_w, tol_b = T.out_backward_ref(x, weight, dy)
    wt = K.segm_out_weights(weight.cuda())
    gx, gw, gb = K.segm_out_conv_backward(dy.cuda(), x.cuda(), wt)
    e_x = R.within(gx, dx, tol_x, F32, 'out_conv dx')
    e_w = R.within(gw.permute(2, 0, 1).unsqueeze(0), dw, tol_w, F32, 'out_conv dw')
    e_b = R.within(gb, db, tol_b, F32, 'out_conv dbias')
    again = K.segm_out_conv_backward(dy.cuda(), x.cuda(), wt)
    assert all(torch.equal(p, q) for p, q in zip((gx, gw, gb), again))
    print(f'out_conv_backward: dx err {e_x:.3e}, dw err {e_w:.3e} (max {dw.abs().max():.3e}), db err {e_b:.3e}')


def test_head_functions_autograd():
    """The three head Functions end to end: gradients of a small chain against the f64 composition."""
    from kinet_amd import autograd as A
    B, Q, h, w, H, W, C = 1, 2, 7, 13, 13, 25, 16
    x, f, dy = T.relu_up_add_case(B, Q, h, w, H, W, C, seed=71)
    _, weight, _ = T.out_backward_case(1, H, W, C, seed=72)
    bias = torch.tensor([0.3])
    g = torch.randn(B * Q, H, W, generator=R.gen(73))
    leaves = [t.double().requires_grad_(True) for t in (x, f, weight, bias)]
    iy, ix = R.nearest_index(h, H), R.nearest_index(w, W)
    y = torch.relu(leaves[0])[:, iy][:, :, ix] + leaves[1].repeat_interleave(Q, 0)
    out = torch.nn.functional.conv2d(y.permute(0, 3, 1, 2), leaves[2], leaves[3], padding=1)[:, 0]
    out.backward(g.double())
    dev = [t.cuda().requires_grad_(True) for t in (x, f, weight, bias)]
    got = A.segm_out_conv(A.segm_relu_up_add(dev[0], dev[1], 0, Q), dev[2], dev[3])
    assert (got.double().cpu() - out.detach()).abs().max() <= 1e-5 * out.detach().abs().max()
    got.backward(g.cuda())
    for a, b, name in zip(dev, leaves, ('x', 'f', 'weight', 'bias')):
        # a chain of two kernels: each gradient within 200 u of the sum of its absolute terms' scale
        err = (a.grad.double().cpu() - b.grad).abs().max().item()
        assert a.grad.shape == b.grad.shape and err <= 200 * R.U32 * max(b.grad.abs().max().item(), 1.0) * 9 * C, (name, err)
