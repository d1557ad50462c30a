"""Direct tests of the segmentation-head kernels (csrc/segm.hip, include/kinet_segm.h): each runs one
kernel against an f64 reference computed here from the same inputs (tests/segm_refs.py, with the
bounds' derivation), at the smallest shapes that reach every path: 7x13 / 13x25 / 26x50 maps (no
multiple of a tile, non-integer upsampling ratios), 33 channels per group, two frames x several
queries (the per-frame operand is broadcast by row // Q), a padded second frame."""
import os

import numpy as np
import pytest
import torch

import segm_refs as R

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
IDS = ['f32', 'bf16', 'f16']


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


# --------------------------------------------------------------------------- attention map
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('B,Q,h,w,masked', [(2, 5, 7, 13, 4), (1, 2, 3, 5, 0)], ids=['7x13-masked', '3x5'])
def test_attention_map_joint_softmax(K, B, Q, h, w, masked, dtype):
    qp, kp, mask = R.attention_case(B, Q, h, w, 256, dtype, seed=11, masked_cols=masked)
    ref, tol = R.attention_ref(qp, kp, mask, Q)
    out = K.segm_attention(qp.cuda(), kp.cuda(), mask.cuda() if masked else None, Q, R.HEADS)
    assert out.shape == (B * Q, h * w, R.HEADS) and out.dtype == dtype
    err = R.within(out, ref, tol, dtype, ('attention', dtype))
    got = out.double().cpu()
    m = mask.view(B, 1, h * w, 1).expand(B, Q, h * w, R.HEADS).reshape(B * Q, h * w, R.HEADS)
    assert (got[m] == 0).all()                                  # masked pixels: exactly 0
    assert (got[~m] > 0).any()
    # each row sums to 1 over heads AND pixels (one joint softmax), within the sum of the elements' bounds
    total = got.sum((1, 2))
    slack = (tol + R.OUT_ROUND[dtype] * ref + R.OUT_TINY[dtype]).sum((1, 2))
    assert ((total - 1).abs() <= slack).all(), (total, slack)
    # ... and not per head: with these logits the heads' shares differ from 1/8 by far more than that
    shares = ref.sum(1)
    assert (shares - 1.0 / R.HEADS).abs().max() > 0.05
    assert ((got.sum(1) - shares).abs() <= (tol + R.OUT_ROUND[dtype] * ref + R.OUT_TINY[dtype]).sum(1)).all()
    assert torch.equal(out, K.segm_attention(qp.cuda(), kp.cuda(), mask.cuda() if masked else None, Q, R.HEADS))
    print(f'segm_attention {B}x{Q} {h}x{w} {dtype}: max err {err:.3e}, peak {ref.max():.3f}')


def test_attention_map_fully_masked_frame_is_nan(K):
    """softmax of a row of -inf is NaN in torch; the kernel says so too instead of dividing silently."""
    qp, kp, mask = R.attention_case(1, 2, 3, 5, 256, F32, seed=12)
    out = K.segm_attention(qp.cuda(), kp.cuda(), torch.ones_like(mask).cuda(), 2, R.HEADS)
    assert torch.isnan(out).all()


# --------------------------------------------------------------------------- lay1
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_lay1_split_equals_full_convolution(K, dtype):
    """frame part (f32 kinet_conv2d of src, once per frame) + per-query 8-channel part against lay1 of
    the concatenated 264-channel input; the plain composition (concatenate, one 264 -> 264
    kinet_conv2d) is held to the same f64 result."""
    B, Q, h, w, d = 2, 3, 7, 13, 256
    src, att, weight, bias = R.lay1_case(B, Q, h, w, d, dtype, seed=21)
    ref, tol = R.lay1_ref(src, att, weight, bias, Q)
    wg, bg = weight.cuda(), bias.cuda()
    frame = K.conv2d_nhwc(src.cuda().float(), K.pack_segm_lay1_src(wg, d, F32), 1, 1, bias=bg, ksplit=1)
    assert frame.dtype == F32 and frame.shape == (B, h, w, d + R.HEADS)
    w_att = K.segm_lay1_weights(wg, d)
    y = K.segm_lay1(att.cuda(), w_att, frame, 0, Q)
    assert y.dtype == dtype and y.shape == ref.shape
    err = R.within(y, ref, tol, dtype, ('lay1 split', dtype))
    # rows in two chunks: the frame index comes from row0, and the values are the same bits
    y2 = torch.cat([K.segm_lay1(att[:2].cuda(), w_att, frame, 0, Q), K.segm_lay1(att[2:].cuda(), w_att, frame, 2, Q)])
    assert torch.equal(y, y2)
    # the query path matters in this case: dropping it misses the bound
    assert ((frame.double().cpu().repeat_interleave(Q, 0) - ref).abs() > tol + R.OUT_ROUND[dtype] * ref.abs()).any()
    cat = torch.cat([src.repeat_interleave(Q, 0), att], -1).cuda()
    plain = K.conv2d_nhwc(cat, K.pack_conv_weight(wg, dtype), 1, 1, bias=bg, ksplit=1)
    ref_p, tol_p = R.lay1_ref(src, att, weight, bias, Q, w_dtype=dtype)
    err_p = R.within(plain, ref_p, tol_p, dtype, ('lay1 plain', dtype))
    print(f'segm_lay1 {dtype}: split max err {err:.3e}, plain max err {err_p:.3e}')


# --------------------------------------------------------------------------- GroupNorm + ReLU (+ upsample + add)
GN_CASES = [(264, 7, 13, 7, 13, True), (128, 7, 13, 7, 13, True), (64, 7, 13, 13, 25, True),
            (32, 13, 25, 26, 50, True), (16, 26, 50, 26, 50, False)]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('C,h,w,H,W,fpn', GN_CASES, ids=[f'C{c[0]}-{c[1]}x{c[2]}-to-{c[3]}x{c[4]}' for c in GN_CASES])
def test_gn_relu_upsample_add(K, C, h, w, H, W, fpn, dtype):
    B, Q, G, eps = 2, 3, 8, 1e-5
    x, gamma, beta, f = R.gn_case(B, Q, h, w, H, W, C, dtype, seed=31 + C, with_fpn=fpn)
    ref, tol = R.gn_relu_ref(x, gamma, beta, f, Q, G, eps, H, W)
    fg = f.cuda() if fpn else None
    y = K.segm_gn_relu(x.cuda(), gamma.cuda(), beta.cuda(), G, eps, fpn=fg, row0=0, Q=Q)
    assert y.shape == (B * Q, H, W, C) and y.dtype == dtype
    err = R.within(y, ref, tol, dtype, ('gn', C, dtype))
    assert torch.equal(y, K.segm_gn_relu(x.cuda(), gamma.cuda(), beta.cuda(), G, eps, fpn=fg, row0=0, Q=Q))
    # the second frame's rows alone (row0 = Q): the same bits, so the frame operand follows row0
    y1 = K.segm_gn_relu(x[Q:].cuda(), gamma.cuda(), beta.cuda(), G, eps, fpn=fg, row0=Q, Q=Q)
    assert torch.equal(y[Q:], y1)
    print(f'segm_gn_relu C={C} {h}x{w}->{H}x{W} {dtype}: max err {err:.3e}')


@pytest.mark.parametrize('n_in,n_out', [(84, 167), (50, 100), (13, 25), (7, 13), (167, 334), (68, 135)])
def test_nearest_rule_is_torch_legacy_nearest(n_in, n_out):
    """segm_refs.nearest_index (the rule the reference above applies) against F.interpolate."""
    src = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
    want = torch.nn.functional.interpolate(src, size=(1, n_out), mode='nearest').view(-1).long()
    assert torch.equal(R.nearest_index(n_in, n_out), want)


# --------------------------------------------------------------------------- out_lay
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_out_conv(K, dtype):
    x, weight, bias = R.out_case(3, 26, 50, 16, dtype, seed=41)
    ref, tol = R.out_ref(x, weight, bias)
    y = K.segm_out_conv(x.cuda(), K.segm_out_weights(weight.cuda()), bias.cuda())
    assert y.dtype == F32 and y.shape == (3, 26, 50)
    err = R.within(y, ref, tol, F32, ('out_conv', dtype))
    print(f'segm_out_conv {dtype}: max err {err:.3e}')


# --------------------------------------------------------------------------- post-process
def test_postprocess_against_reference(K, golden_dir):
    from kinet_amd.models.segmentation import PostProcessSegm
    d = np.load(os.path.join(golden_dir, 'segm_a.npz'))
    pred = torch.from_numpy(d['pred_masks']).cuda()
    post = PostProcessSegm()
    shares = R.check_post(post, pred, d)
    R.check_post(post, pred, d, on_device=True)
    orig, max_sizes = torch.from_numpy(d['orig_sizes']), torch.from_numpy(d['max_sizes'])
    probs = post([{}, {}], {'pred_masks': pred}, orig, max_sizes, return_probs=True)
    errs = []
    for i in range(2):
        got = probs[i]['masks']
        assert got.dtype == F32 and not got.is_cuda and got.shape == (pred.shape[1], 1) + tuple(orig[i].tolist())
        errs.append((got[:, :, ::3, ::3] - torch.from_numpy(d[f'post{i}_probs3'])).abs().max().item())
        # the binary masks are this probability map's threshold
        assert torch.equal(post([{}, {}], {'pred_masks': pred}, orig, max_sizes)[i]['masks'], (got > 0.5).byte())
    print(f'segm_postprocess: max prob err {max(errs):.3e}, excluded share {shares}')
    assert max(errs) <= 2e-6
    # results_mask keeps the reference's meaning: a per-frame selection of queries
    keep = torch.zeros(pred.shape[1], dtype=torch.bool)
    keep[[1, 4]] = True
    sel = post([{}, {}], {'pred_masks': pred}, orig, max_sizes, return_probs=True, results_mask=[keep, keep])
    assert torch.equal(sel[0]['masks'], probs[0]['masks'][keep])
