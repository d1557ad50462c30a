"""CPU checks of tests/direct_refs.py: the references the direct kernel tests compare against,
so a wrong helper cannot be blamed on a kernel."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import direct_refs as R


def _pixelwise_sine(mask, npf, three_d=False, frame=0, frames=1, normalize=True, ft=np.float64):
    """The embedding one pixel at a time, from the formulas in the docstring of
    kinet_amd/models/position_encoding.py: count the unmasked pixels of the pixel's column down to
    its row and of its row up to its column (and, 3-d, of its frame stack up to `frame`), divide by
    the count of the whole column / row / stack (+ 1e-6) times 2 pi when normalising (2-d: after
    taking 0.5 off), then sin (even channels) / cos (odd) of count / dim_t.  Every step in `ft`
    arithmetic (np.float64 or np.float32); returns (B, H*W, C) f64."""
    B, H, W = mask.shape
    free = [[[0 if v else 1 for v in row] for row in img] for img in mask.tolist()]
    dim_t = R.sine_dim_t(npf).numpy().astype(ft)
    even = np.arange(npf) % 2 == 0
    two_pi, tiny, half = ft(2 * math.pi), ft(1e-6), ft(0.5)
    out = np.zeros((B, H * W, (3 if three_d else 2) * npf))
    for b in range(B):
        for h in range(H):
            for w in range(W):
                column = [free[b][i][w] for i in range(H)]
                axes = [(sum(column[:h + 1]), sum(column)), (sum(free[b][h][:w + 1]), sum(free[b][h]))]
                if three_d:
                    axes.insert(0, (free[b][h][w] * (frame + 1), free[b][h][w] * frames))
                blocks = []
                for count, whole in axes:
                    e = ft(count)
                    if normalize:
                        e = (e if three_d else e - half) / (ft(whole) + tiny) * two_pi
                    a = e / dim_t
                    blocks.append(np.where(even, np.sin(a), np.cos(a)))
                out[b, h * W + w] = np.concatenate(blocks)
    return torch.from_numpy(out)


GEO = R.sine_geometries()


@pytest.mark.parametrize('name', sorted(GEO))
@pytest.mark.parametrize('npf', [128, 144, 96])
@pytest.mark.parametrize('normalize', [True, False])
def test_sine_restatement_equals_pixelwise_2d(name, npf, normalize):
    mask = GEO[name]
    ref = R.sine_embed_ref(mask, npf, normalize=normalize)
    naive = _pixelwise_sine(mask, npf, normalize=normalize)
    keep = R.sine_compared(mask, npf, False, normalize)
    assert ref.shape == naive.shape == keep.shape
    # the same f64 arithmetic at every compared position (the excluded ones have arguments
    # ~ -3e6: bounded, not compared)
    assert (ref - naive)[keep].abs().max().item() <= 1e-12
    assert ref.abs().max().item() <= 1.0


@pytest.mark.parametrize('name', sorted(GEO))
@pytest.mark.parametrize('frames,npf', [(2, 96), (3, 128), (2, 144)])
@pytest.mark.parametrize('normalize', [True, False])
def test_sine_restatement_equals_pixelwise_3d(name, frames, npf, normalize):
    mask = GEO[name]
    for f in range(frames):
        ref = R.sine_embed_ref(mask, npf, True, f, frames, normalize)
        assert R.sine_compared(mask, npf, True, normalize).all()
        assert (ref - _pixelwise_sine(mask, npf, True, f, frames, normalize)).abs().max().item() <= 1e-12


def test_sine_dim_t_is_the_modules_own():
    from kinet_amd.models.position_encoding import PositionEmbeddingSine
    for npf in (128, 144, 96):
        assert torch.equal(R.sine_dim_t(npf), PositionEmbeddingSine(npf, normalize=True).dim_t('cpu'))


def test_sine_level_embed_is_added_per_channel():
    mask = GEO['main']
    le = torch.randn(256, generator=torch.Generator().manual_seed(2))
    a = R.sine_embed_ref(mask, 128)
    b = R.sine_embed_ref(mask, 128, level_embed=le)
    assert torch.equal(b, a + le.double())


@pytest.mark.parametrize('npf', [128, 144, 96])
def test_sine_f32_vs_f64_gap_on_main_masks(npf):
    """The same arithmetic evaluated step by step in f32 vs in f64, at the compared positions of
    the main mask set, normalised (arguments up to 2 pi): the f32 tolerance of the GPU test (5e-6)
    is several times this."""
    mask = GEO['main']
    keep = R.sine_compared(mask, npf, False, True)
    g2 = (_pixelwise_sine(mask, npf, ft=np.float32) - _pixelwise_sine(mask, npf))[keep].abs().max().item()
    g3 = max((_pixelwise_sine(mask, npf, True, f, 2, ft=np.float32)
              - _pixelwise_sine(mask, npf, True, f, 2)).abs().max().item() for f in (0, 1))
    print(f'sine f32-vs-f64 gap npf={npf}: 2-d {g2:.3e}, 3-d {g3:.3e}')
    assert g2 < 1e-6 and g3 < 1e-6


def test_sine_excluded_share_caps():
    """Nothing excluded for an unmasked image, <= 25 % for every other image the GPU test compares
    in 2-d normalised mode; the main set gives 20.9 % and 7.5 %."""
    for name, mask in GEO.items():
        share = R.sine_excluded_share(mask)
        for b in range(mask.shape[0]):
            if (name, b) in R.FULLY_MASKED:
                assert mask[b].all() and share[b].item() == 1.0
                continue
            if not mask[b].any():
                assert share[b].item() == 0.0
            assert share[b].item() <= 0.25, (name, b, share[b].item())
    main = R.sine_excluded_share(GEO['main'])
    assert main[0].item() == 0.0
    assert abs(main[1].item() - 0.209) < 1e-3 and abs(main[2].item() - 0.075) < 1e-3


def test_main_mask_set_has_holes_and_a_masked_row_and_column():
    m = GEO['main']
    assert not m[0].any()
    assert (~m[1, :9, :13]).all() and m[1, 9:].all() and m[1, :, 13:].all()
    assert m[2, 4].all() and m[2, :, 6].all()
    inner = m[2, 1:-1, 1:-1]
    assert inner.any() and not inner.all()
    # no other row or column of image 2 is fully masked
    assert m[2].all(1).sum().item() == 1 and m[2].all(0).sum().item() == 1


@pytest.mark.parametrize('KH,KW,stride,pad,H,W,C', [(3, 2, (2, 1), (1, 0), 5, 4, 4), (1, 3, (1, 2), (0, 1), 3, 5, 8)])
def test_unfold_fold_helpers_vs_naive_loop(KH, KW, stride, pad, H, W, C):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, H, W, C, generator=g, dtype=torch.float64)
    cols = R.unfold_nhwc(x, KH, KW, stride, pad)
    assert torch.equal(cols, R.unfold_naive(x, KH, KW, stride, pad))
    c = torch.randn(cols.shape, generator=g, dtype=torch.float64)
    dx = R.fold_nhwc(c, x.shape, KH, KW, stride, pad)
    assert (dx - R.fold_naive(c, x.shape, KH, KW, stride, pad)).abs().max().item() < 1e-12
    # and the two are adjoint
    assert abs((cols * c).sum().item() - (x * dx).sum().item()) < 1e-9


def test_inverse_sigmoid_matches_host_definition_at_clamp_points():
    from kinet_amd.models.misc import inverse_sigmoid
    x = torch.tensor([0.0, 1.0, 1e-7, 1 - 1e-7, -1e-3, 1.001, 1e-5, 1 - 1e-5, 2e-5, 0.5, 0.25], dtype=torch.float32)
    got = R.inverse_sigmoid_ref(x)
    host = inverse_sigmoid(x)                      # the CPU branch: torch f32
    assert (got - host.double()).abs().max().item() < 2e-6
    assert got[0].item() == pytest.approx(math.log(1e-5 / 1.0), abs=1e-12)
    assert got[1].item() == pytest.approx(math.log(1.0 / 1e-5), abs=1e-12)
    assert got[4].item() == got[0].item() and got[5].item() == got[1].item()
    assert got[9].item() == 0.0


def test_box_case_valid_ratios_make_a_wrong_index_visible():
    """The valid ratios of a case differ by far more than the tolerance (1e-5) between batches,
    levels and x / y, so a wrong index in the kernel cannot pass; the clamp points are in `ref`."""
    for B, L in ((1, 1), (1, 4), (3, 1), (3, 4)):
        _, ref, vr = R.box_case(B, 300, L, 4)
        flat = vr.reshape(-1)
        d = (flat[:, None] - flat[None, :]).abs() + torch.eye(flat.numel())
        assert d.min().item() > 1e-2
        for s in R.SPECIAL_REFS:
            assert (ref == torch.tensor(s, dtype=torch.float32)).any()


def test_box_refine_ref_pads_two_column_references():
    g = torch.Generator().manual_seed(4)
    tmp = torch.randn(2, 5, 4, generator=g)
    ref2 = torch.rand(2, 5, 2, generator=g)
    vr = torch.rand(2, 3, 2, generator=g)
    new, rin = R.box_refine_ref(tmp, ref2, vr)
    assert torch.equal(new[..., 2:], torch.sigmoid(tmp[..., 2:].double()))
    assert rin.shape == (2, 5, 3, 4)
    assert torch.equal(rin[1, 2, 1], new[1, 2] * torch.stack([vr[1, 1, 0], vr[1, 1, 1]] * 2).double())


def test_layernorm_vec_eligibility_table():
    f32, bf = torch.float32, torch.bfloat16
    assert [d for d in (8, 36, 90, 256, 288, 512, 1024) if R.layernorm_vec_eligible(f32, d)] == [8, 36, 256]
    assert [d for d in (8, 36, 90, 256, 288, 512, 1024) if R.layernorm_vec_eligible(bf, d)] == [8, 256, 288, 512]


# =================================================== training path references (grad.hip, train_ops.hip)
M64 = (1 << 64) - 1


def _keep_bigint(seed, idx, thresh):
    """common.h's dropout_keep in Python integers, reduced mod 2^64 by hand."""
    z = ((seed & M64) + idx * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return (z >> 40) >= thresh


def test_dropout_thresh_rounds_p_to_f32_first():
    # f32(0.15) = 0.1500000059...: 2516582.5 + 0.5 rounds to ...83; the double 0.15 gives ...82
    assert R.dropout_thresh_ref(0.15) == 2516583 and int(0.15 * 2 ** 24 + 0.5) == 2516582
    assert R.dropout_thresh_ref(0.1) == 1677722         # 1677721.625 + 0.5 (the double 0.1 agrees here)
    assert R.dropout_thresh_ref(0.0) == 0 and R.dropout_thresh_ref(0.5) == 1 << 23
    assert R.dropout_thresh_ref(0.999) == int(float(np.float32(0.999)) * 2 ** 24 + 0.5)


@pytest.mark.parametrize('seed', [0, 1, -1, -(2 ** 63), 2 ** 63 - 1, 123456789])
def test_dropout_keep_ref_equals_bigint(seed):
    idx = [0, 1, 2, 63, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 12345, 2 ** 40 + 7, 2 ** 62]
    for p in (0.1, 0.5, 0.999):
        got = R.dropout_keep_ref(seed, np.array(idx, dtype=np.uint64), p)
        want = [_keep_bigint(seed, i, R.dropout_thresh_ref(p)) for i in idx]
        assert got.tolist() == want
    dense = R.dropout_keep_ref(seed, np.arange(5000, dtype=np.uint64), 0.3)
    assert dense.tolist() == [_keep_bigint(seed, i, R.dropout_thresh_ref(0.3)) for i in range(5000)]


def test_dropout_seed_for_draw_hits_the_threshold():
    """The hash is a bijection of the seed: seed_for_draw puts element idx's 24-bit draw on a chosen
    value, so a test can sit exactly on the threshold (kept) and one below it (dropped)."""
    for p in (0.1, 0.15, 0.5, 0.999):
        t = R.dropout_thresh_ref(p)
        for idx in (0, 5, 2 ** 33 + 1):
            s_keep, s_drop = R.dropout_seed_for_draw(t, idx), R.dropout_seed_for_draw(t - 1, idx)
            assert -(2 ** 63) <= s_keep < 2 ** 63
            assert _keep_bigint(s_keep, idx, t) and not _keep_bigint(s_drop, idx, t)
            assert R.dropout_keep_ref(s_keep, idx, p)[0] and not R.dropout_keep_ref(s_drop, idx, p)[0]


def test_dropout_keep_ref_rate_and_p0():
    n = 1 << 20
    assert R.keep_mask(5, (n,), 0.0).all()
    for p in (0.1, 0.5, 0.999):
        rate = R.keep_mask(-7, (n,), p).double().mean().item()
        q = 1 - float(np.float32(p))
        assert abs(rate - q) < 5 * (q * (1 - q) / n) ** 0.5, (p, rate)


def test_keep_mask_flat_index_conventions():
    rows, d, p = 5, 13, 0.4
    m = R.keep_mask(11, (rows, d), p)
    for r, c in [(0, 0), (1, 0), (4, 12), (2, 7)]:
        assert bool(m[r, c]) == bool(R.dropout_keep_ref(11, r * d + c, p)[0])
    B, H, Lq, Lk = 2, 3, 4, 5
    m = R.keep_mask(11, (B, H, Lq, Lk), p)
    for b, h, i, j in [(0, 0, 0, 0), (1, 2, 3, 4), (1, 0, 2, 1), (0, 2, 0, 3)]:
        assert bool(m[b, h, i, j]) == bool(R.dropout_keep_ref(11, ((b * H + h) * Lq + i) * Lk + j, p)[0])
    assert R.keep_scale32(0.5) == 2.0 and abs(R.keep_scale64(0.3) - R.keep_scale32(0.3)) < 3e-7


def test_colsum_chunks_restatement():
    assert R.colsum_chunks(0) == (1, 0) and R.colsum_chunks(63) == (1, 63) and R.colsum_chunks(128) == (2, 64)
    assert R.colsum_chunks(16389) == (256, 65)          # the 256-chunk cap binds
    assert R.gn_blocks(127) == (1, 127) and R.gn_blocks(257) == (2, 129) and R.gn_blocks(66000) == (512, 129)


@pytest.mark.parametrize('rows,d', [(1, 1), (3, 65), (17, 288)])
def test_ln_ref_equals_f64_autograd(rows, d):
    x, dy, gamma, beta = (t.double() for t in R.ln_case(rows, d, torch.float32))
    xt, gt, bt = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    y = F.layer_norm(xt, (d,), gt, bt, R.eps32(1e-5))
    y.backward(dy)
    ref = R.ln_ref(x, gamma, beta, 1e-5, dy=dy)
    for got, want in [(ref['y'], y.detach()), (ref['dz'], xt.grad), (ref['dg'], gt.grad), (ref['db'], bt.grad)]:
        assert (got - want).abs().max().item() <= 1e-11 * (1 + want.abs().max().item())
    for n in ('dz', 'dg', 'db', 'y'):
        assert (ref[n + 'A'] >= ref[n].abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize('shape', [(2, 5, 30, 6), (1, 40, 8, 8), (2, 40, 8, 1), (2, 35, 36, 12)])
def test_gn_bwd_ref_equals_f64_autograd(shape):
    N_, HW, C, G = shape
    x, dy, gamma = (t.double() for t in R.gn_case(N_, HW, C, torch.float32))
    xt = x.permute(0, 2, 1).contiguous().requires_grad_()
    gt, bt = gamma.clone().requires_grad_(), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    F.group_norm(xt, G, gt, bt, R.eps32(1e-5)).backward(dy.permute(0, 2, 1).contiguous())
    ref = R.gn_bwd_ref(dy, x, gamma, G, 1e-5)
    assert (ref['dx'] - xt.grad.permute(0, 2, 1)).abs().max().item() <= 1e-11
    assert (ref['dg'] - gt.grad).abs().max().item() <= 1e-10 and (ref['db'] - bt.grad).abs().max().item() <= 1e-10
    for n in ('dx', 'dg', 'db'):
        assert (ref[n + 'A'] >= ref[n].abs() * (1 - 1e-12)).all()
    assert (ref['dx_c'] >= 4.5 * 8).all()


def _f32_formula_err(kind):
    """The kernels' norm-backward formulas evaluated step by step in f32 torch on the guards' inputs:
    (its dx / dgamma error, torch's own CPU f32 backward's error), both against the f64 reference."""
    if kind == 'ln':
        d = 288
        x, dy, gamma, beta = R.ln_case(64, d, torch.float32, seed=5, offset=100.0)
        ref = R.ln_ref(x, gamma, None, 1e-5, dy=dy)
        xt, gt = x.clone().requires_grad_(), gamma.clone().requires_grad_()
        F.layer_norm(xt, (d,), gt, beta, 1e-5).backward(dy)
        mean = x.mean(-1, keepdim=True)
        rstd = (((x - mean) ** 2).mean(-1, keepdim=True) + 1e-5).rsqrt()
        xh, g = (x - mean) * rstd, dy * gamma
        dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
        dg = (dy * xh).sum(0)
        return [((dx.double() - ref['dz']).abs().max().item(), (xt.grad.double() - ref['dz']).abs().max().item()),
                ((dg.double() - ref['dg']).abs().max().item(), (gt.grad.double() - ref['dg']).abs().max().item())]
    N_, HW, C, G = 2, 200, 32, 4
    x, dy, gamma = R.gn_case(N_, HW, C, torch.float32, seed=3, offset=30.0)
    ref = R.gn_bwd_ref(dy, x, gamma, G, 1e-5)
    xt, gt = x.permute(0, 2, 1).contiguous().requires_grad_(), gamma.clone().requires_grad_()
    F.group_norm(xt, G, gt, torch.zeros(C), 1e-5).backward(dy.permute(0, 2, 1).contiguous())
    cg = C // G
    X, DY, gm = x.view(N_, HW, G, cg), dy.view(N_, HW, G, cg), gamma.view(1, 1, G, cg)
    piv = R.gn_pivot(X)
    S = X - piv
    ms = S.mean((1, 3), keepdim=True)
    var = ((S * S).mean((1, 3), keepdim=True) - ms * ms).clamp(min=0)           # one pass, as the kernel
    rstd = (var + 1e-5).rsqrt()
    a = (DY * gm).mean((1, 3), keepdim=True)
    bx = rstd * ((DY * gm * S).mean((1, 3), keepdim=True) - ms * a)
    dx = (rstd * (DY * gm - a - (X - (piv + ms)) * rstd * bx)).reshape(N_, HW, C)
    dg = (rstd * ((DY * S).sum(1, keepdim=True) - ms * DY.sum(1, keepdim=True))).sum((0, 1)).reshape(C)
    return [((dx.double() - ref['dx']).abs().max().item(), (xt.grad.permute(0, 2, 1).double() - ref['dx']).abs().max().item()),
            ((dg.double() - ref['dg']).abs().max().item(), (gt.grad.double() - ref['dg']).abs().max().item())]


@pytest.mark.parametrize('kind', ['ln', 'gn'])
def test_norm_backward_guard_yardstick_is_attainable(kind):
    """The guards bound the kernels by 4x torch's CPU f32 error: an f32 evaluation of the kernels' own
    formulas sits inside that on the same inputs, so the yardstick asks nothing a correct f32 kernel
    cannot give."""
    for (formula, torch_f32), name in zip(_f32_formula_err(kind), ('dx', 'dgamma')):
        print(f'{kind} guard {name}: f32 formula err {formula:.3e}, torch CPU f32 err {torch_f32:.3e}')
        assert formula <= 4 * torch_f32, (kind, name, formula, torch_f32)


@pytest.mark.parametrize('mask,p', [('none', 0.0), ('some', 0.0), ('some', 0.5), ('batch', 0.0)])
def test_attn_ref_equals_f64_autograd(mask, p):
    B, H, D, Lq, Lk = 2, 2, 5, 7, 9
    q, k, v, do = (t.double() for t in R.attn_case(B, H, D, Lq, Lk))
    km = None
    if mask != 'none':
        km = torch.zeros(B, Lk, dtype=torch.bool)
        km[0, 3:6] = True
        km[1, -2:] = True
        if mask == 'batch':
            km[1] = True
    keep = R.keep_mask(3, (B, H, Lq, Lk), p) if p > 0 else None
    scale = D ** -0.5
    ref = R.attn_ref(q, k, v, do, H, scale, km, keep, p)
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    Q, K_, V = (t.view(B, -1, H, D).transpose(1, 2) for t in leaves)
    S = Q @ K_.transpose(-1, -2) * scale
    if km is not None:
        S = S.masked_fill(km[:, None, None, :], float('-inf'))
    P = S.softmax(-1)
    if mask == 'batch':     # a fully masked row: softmax is 0/0 there, the operation defines P = 0
        S2 = S.masked_fill(km.all(-1)[:, None, None, None], 0.0)
        P = S2.softmax(-1) * (~km.all(-1))[:, None, None, None]
    if keep is not None:
        P = P * keep.double() * R.keep_scale64(p)
    o = (P @ V).transpose(1, 2).reshape(B, Lq, H * D)
    o.backward(do)
    for n, want in zip(('o', 'dq', 'dk', 'dv'), [o.detach()] + [t.grad for t in leaves]):
        assert (ref[n] - want).abs().max().item() <= 1e-12, n
        assert (ref[n + 'A'] >= ref[n].abs() * (1 - 1e-12)).all()
    if mask == 'batch':
        assert all((ref[n][1] == 0).all() and (ref[n + 'A'][1] == 0).all() for n in ('dq', 'dk', 'dv'))
    if mask == 'none' and p == 0:
        sd = F.scaled_dot_product_attention(*(t.detach() for t in (Q, K_, V))).transpose(1, 2).reshape(B, Lq, H * D)
        assert (ref['o'] - sd).abs().max().item() <= 1e-12
    f32 = R.attn_ref(q.float(), k.float(), v.float(), do.float(), H, scale, km, keep, p, dtype=torch.float32)
    assert f32['dq'].dtype == torch.float32 and R.attn_yardstick(ref, f32, ['dq', 'dk', 'dv']) < 1e-5


@pytest.mark.parametrize('rd', [2, 4])
@pytest.mark.parametrize('M,L,P', [(2, 3, 2), (4, 2, 4)])
def test_msda_prep_refs_equal_f64_autograd(rd, M, L, P):
    Nb, Lq = 2, 5
    offlog, refs, shapes, gloc, gattw = R.msda_case(Nb, Lq, M, L, P, rd)
    qm = torch.zeros(Nb, Lq, dtype=torch.bool)
    qm[0, 1] = qm[1, 4] = True
    n = M * L * P
    ol, rf = offlog.double().requires_grad_(), refs.double().requires_grad_()
    # the module's own expressions (ms_deform_attn.py), in f64
    off = ol[..., :2 * n].view(Nb, Lq, M, L, P, 2)
    aw = ol[..., 2 * n:].view(Nb, Lq, M, L * P).softmax(-1).view(Nb, Lq, M, L, P)
    aw = aw.masked_fill(qm[:, :, None, None, None], 0.0)
    if rd == 2:
        loc = rf[:, :, None, :, None, :] + off / shapes.double()[None, None, None, :, None, :]
    else:
        loc = rf[:, :, None, :, None, :2] + off / P * rf[:, :, None, :, None, 2:] * 0.5
    ref = R.msda_prep_ref(offlog, refs, shapes, qm, M, L, P)
    assert (ref['loc'] - loc.detach()).abs().max().item() <= 1e-13
    assert (ref['attw'] - aw.detach()).abs().max().item() <= 1e-15
    assert shapes[:, 0].ne(shapes[:, 1]).all()
    ((loc * gloc.double()).sum() + (aw * gattw.double()).sum()).backward()
    b = R.msda_prep_bwd_ref(gloc, gattw, ref['attw'], offlog, refs, shapes, M, L, P)
    assert (b['dol'] - ol.grad).abs().max().item() <= 1e-13 and (b['dref'] - rf.grad).abs().max().item() <= 1e-13
    assert (b['dolA'] >= b['dol'].abs() * (1 - 1e-12)).all() and (b['drefA'] >= b['dref'].abs() * (1 - 1e-12)).all()


def test_inv_sigmoid_ref_equals_f64_autograd():
    x = R.inv_sigmoid_inputs()
    dy = torch.randn(x.numel(), generator=torch.Generator().manual_seed(6))
    y, dx = R.inv_sigmoid_fwd_bwd_ref(x, dy)
    xt = x.double().requires_grad_()
    e = R.eps32(1e-5)
    xc = xt.clamp(min=0, max=1)
    yt = torch.log(xc.clamp(min=e) / (1 - xc).clamp(min=e))
    yt.backward(dy.double())
    assert torch.equal(y, yt.detach()) and (dx - xt.grad).abs().max().item() <= 1e-9 * dx.abs().max().item()
    assert (R.inverse_sigmoid_ref(x, e) - y).abs().max().item() == 0


# -------------------------------------------- GroupNorm forward / fused LayerNorm epilogues
GN_FWD_TABLE = [(s, d, p) for p in ('scalar', 'vector', 'straddle') for s, d in R.gn_fwd_cases(p)]


@pytest.mark.parametrize('shape,dtype,path', GN_FWD_TABLE, ids=lambda v: str(v).replace('torch.', '').replace(' ', ''))
def test_gn_fwd_path_table(shape, dtype, path):
    N_, HW, C, G = shape
    assert R.gn_fwd_path(dtype, C, G, HW=HW) == path
    assert R.gn_fwd_path(dtype, C, G, aligned=False, HW=HW) == 'scalar'
    assert R.gn_fwd_chain(path, dtype, HW, C, G) >= 3


def test_gn_fwd_path_conditions():
    f32, bf16 = torch.float32, torch.bfloat16
    assert R.gn_fwd_path(torch.float64, 32, 4) == 'scalar'
    assert R.gn_fwd_path(f32, 32, 4, y_stride=129 * 32 + 64, HW=129) == 'vector'
    assert R.gn_fwd_path(f32, 32, 4, y_stride=129 * 32 + 3, HW=129) == 'scalar'
    assert R.gn_fwd_path(bf16, 32, 4, y_stride=129 * 32 + 4, HW=129) == 'scalar'       # V = 8
    assert R.gn_fwd_path(f32, 1028, 4) == 'scalar' and R.gn_fwd_path(f32, 1024, 4) == 'vector'   # C / V <= 256
    assert R.gn_fwd_path(bf16, 2048, 4) == 'vector' and R.gn_fwd_path(bf16, 2056, 4) == 'scalar'
    assert R.gn_fwd_path(f32, 24, 8) == 'scalar' and R.gn_fwd_path(f32, 24, 4) == 'straddle'     # groups of 3, 6
    for N_, HW, C, G, path in R.GN_GUARD:
        assert R.gn_fwd_path(f32, C, G, HW=HW) == path
    # the chains, by hand: (2, 35, 36, 12) scalar: 35 pixels + 3 channels, 1 block on tpo = 10 threads
    assert R.gn_fwd_chain('scalar', f32, 35, 36, 12) == 35 + 3 + 1 + 10
    # (3, 273, 256, 32) f32 vector: nslot = 4, 32 pixels x 4 elements, 4 slots x 2 vectors; 3 blocks on tpo = 4
    assert R.gn_fwd_chain('vector', f32, 273, 256, 32) == 32 * 4 + 4 * 2 + 1 + 4
    # (1, 300, 288, 32) f32 straddle: nslot = 3, 43 pixels, 3 slots x 9 channels; 3 blocks on tpo = 4
    assert R.gn_fwd_chain('straddle', f32, 300, 288, 32) == 43 + 27 + 1 + 4
    # (1, 40, 320, 160) scalar: 40 + 2, one block, tpo = 1
    assert R.gn_fwd_chain('scalar', f32, 40, 320, 160) == 40 + 2 + 1 + 1


@pytest.mark.parametrize('shape', [(2, 5, 30, 6), (1, 40, 8, 8), (2, 40, 8, 1), (2, 35, 36, 6), (1, 1, 8, 2)])
def test_gn_fwd_ref_equals_f64_group_norm(shape):
    N_, HW, C, G = shape
    x, gamma, beta = (t.double() for t in R.gn_fwd_case(N_, HW, C, torch.float32))
    want = F.group_norm(x.permute(0, 2, 1).contiguous(), G, gamma, beta, R.eps32(1e-5)).permute(0, 2, 1)
    ref = R.gn_fwd_ref(x.float(), gamma, beta, G, 1e-5, R.gn_fwd_path(torch.float32, C, G, HW=HW))
    assert (ref['y'] - want).abs().max().item() <= 1e-11
    assert (ref['yA'] >= ref['y'].abs() * (1 - 1e-12)).all() and (ref['y_c'] >= 10).all()


@pytest.mark.parametrize('rows,d,offset', [(5, 256, 0.0), (7, 200, 100.0), (3, 288, 100.0)])
def test_ln_epilogue_ref_equals_f64_layer_norm(rows, d, offset):
    g = torch.Generator().manual_seed(rows + d)
    pre = offset + torch.randn(rows, d, generator=g, dtype=torch.float64)
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
    ref = R.ln_epilogue_ref(pre, gamma, beta, 1e-5)
    want = F.layer_norm(pre, (d,), gamma.double(), beta.double(), R.eps32(1e-5))
    assert (ref['y'] - want).abs().max().item() <= 1e-11
    assert (ref['yA'] >= ref['y'].abs() * (1 - 1e-12)).all()
    y, t = R.ln_epilogue_yardstick(pre, gamma, beta)
    assert torch.equal(y, ref['y']) and 0 < t < 1e-4


def _gn_fwd_emulate(x, gamma, beta, G, eps, ppb, shifted):
    """kinet_groupnorm's arithmetic in f32 numpy: per block of ppb pixels the per-channel serial sums of
    s and s^2, the group's channels in order, the blocks in order; mean = pivot + mean_s, the one-pass
    variance E[s^2] - mean_s^2.  s = x - pivot (the pivot formed as gn_pivot, in f32) or, shifted =
    False, the raw x."""
    f = np.float32
    N_, HW, C = x.shape
    cg = C // G
    X = x.numpy().astype(f).reshape(N_, HW, G, cg)
    if shifted:
        m, npx = min(cg, 8), min(HW, 4)
        piv = (np.cumsum(X[:, :npx, :, :m].transpose(0, 2, 1, 3).reshape(N_, G, npx * m), axis=-1, dtype=f)[..., -1]
               / f(m * npx)).reshape(N_, 1, G, 1)
    else:
        piv = np.zeros((N_, 1, G, 1), f)
    S = X - piv
    s = np.zeros((N_, G), f)
    q = np.zeros((N_, G), f)
    for p0 in range(0, HW, ppb):
        blk = S[:, p0:p0 + ppb]
        cs = np.cumsum(blk, axis=1, dtype=f)[:, -1]                      # (N, G, cg): a channel's pixels
        cq = np.cumsum(blk * blk, axis=1, dtype=f)[:, -1]
        s = s + np.cumsum(cs, axis=-1, dtype=f)[..., -1]                 # the group's channels, then the blocks
        q = q + np.cumsum(cq, axis=-1, dtype=f)[..., -1]
    cnt = f(HW * cg)
    ms = s / cnt
    var = np.maximum(q / cnt - ms * ms, f(0))
    rstd = (f(1) / np.sqrt(var + f(eps))).astype(f).reshape(N_, 1, G, 1)
    mean = piv + ms.reshape(N_, 1, G, 1)
    y = (X - mean) * rstd * gamma.numpy().astype(f).reshape(1, 1, G, cg) + beta.numpy().astype(f).reshape(1, 1, G, cg)
    assert y.dtype == f
    return torch.from_numpy(y.reshape(N_, HW, C))


@pytest.mark.parametrize('N_,HW,C,G,path', R.GN_GUARD)
def test_gn_fwd_guard_discriminates_raw_from_shifted_sums(N_, HW, C, G, path):
    """On the guard's inputs (x = 30 + randn) an f32 emulation of the one-pass variance of raw sums
    misses the guard's bound, 4x torch's CPU f32 error, and the same emulation summing x - pivot
    (gn_pivot) meets it: the guard tells the two apart, and asks nothing f32 cannot give."""
    x, gamma, beta = R.gn_fwd_case(N_, HW, C, torch.float32, R.GN_GUARD_SEED, R.GN_GUARD_OFFSET)
    ref = R.gn_fwd_ref(x, gamma, beta, G, 1e-5, path)
    t = (R.gn_fwd_torch_f32(N_, HW, C, G, R.GN_GUARD_SEED, R.GN_GUARD_OFFSET).double() - ref['y']).abs().max().item()
    ppb = 64 if path == 'scalar' else 128
    raw = (_gn_fwd_emulate(x, gamma, beta, G, 1e-5, ppb, False).double() - ref['y']).abs()
    shifted = (_gn_fwd_emulate(x, gamma, beta, G, 1e-5, ppb, True).double() - ref['y']).abs()
    print(f'gn fwd guard ({N_}, {HW}, {C}, {G}) {path}: torch CPU f32 err {t:.3e}, bound {4 * t:.3e}, raw sums '
          f'{raw.max().item():.3e}, shifted sums {shifted.max().item():.3e}')
    assert raw.max().item() > 4 * t
    assert shifted.max().item() <= 4 * t
    # the shifted emulation also sits inside the per-element bound of gn_fwd_ref
    assert (shifted <= ref['y_c'] * R.U32 * ref['yA']).all()


def _lane_sum(a):
    """Row sums in f32 the way a wavefront takes them: lane l adds elements l, l + 64, ... serially, then
    the 64 lane sums combine in a 6-level tree."""
    f = np.float32
    rows, d = a.shape
    nv = -(-d // 64)
    lanes = np.cumsum(np.pad(a, ((0, 0), (0, nv * 64 - d))).reshape(rows, nv, 64), axis=1, dtype=f)[:, -1]
    while lanes.shape[1] > 1:
        h = lanes.shape[1] // 2
        lanes = lanes[:, :h] + lanes[:, h:]
    assert lanes.dtype == f
    return lanes


def _ln_emulate(pre64, gamma, beta, eps, one_pass):
    """A row LayerNorm in f32 numpy with a wavefront's sums: two-pass (mean, then the sum of
    (v - mean)^2) or one-pass (the sums of v and v^2)."""
    f = np.float32
    v = pre64.numpy().astype(f)
    d = f(v.shape[-1])
    mean = _lane_sum(v) / d
    if one_pass:
        var = np.maximum(_lane_sum(v * v) / d - mean * mean, f(0))
    else:
        var = _lane_sum((v - mean) * (v - mean)) / d
    y = (v - mean) * (f(1) / np.sqrt(var + f(eps))).astype(f) * gamma.numpy().astype(f) + beta.numpy().astype(f)
    assert y.dtype == f
    return torch.from_numpy(y)


@pytest.mark.parametrize('d', [256, 288, 200])
def test_ln_epilogue_bounds_discriminate_one_pass_from_two_pass(d):
    """Rows of 100 + O(1): an f32 one-pass LayerNorm misses both the f32 bound (4x torch's CPU f32
    error) and the f16 bound (one output rounding of the f64 result + the same 4x term), even before
    its own output rounding; the two-pass form meets the f32 bound, and its f16 rounding the f16 one."""
    g = torch.Generator().manual_seed(d)
    pre = 100.0 + torch.randn(37, d, generator=g, dtype=torch.float64) * 1.5
    gamma, beta = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
    y, t = R.ln_epilogue_yardstick(pre, gamma, beta)
    one = _ln_emulate(pre, gamma, beta, 1e-5, True)
    two = _ln_emulate(pre, gamma, beta, 1e-5, False)
    e1, e2 = (one.double() - y).abs(), (two.double() - y).abs()
    print(f'ln epilogue d={d} offset 100: torch CPU f32 err {t:.3e}, bound {4 * t:.3e}, one-pass {e1.max().item():.3e}, '
          f'two-pass {e2.max().item():.3e}')
    assert e2.max().item() <= 4 * t < e1.max().item()
    tol16 = R.OUT_ROUND[torch.float16] * y.abs() + 4 * t
    assert (e1 > tol16).any()
    assert ((one.half().double() - y).abs() > tol16).any()
    assert ((two.half().double() - y).abs() <= tol16).all()


# ======================================= tiled GEMM / implicit convolution (csrc/gemm.hip)
def _f32_chunked(x, w, step, reverse):
    """x @ w.T in f32, K taken in chunks of `step` accumulated sequentially, forwards or backwards."""
    K = x.shape[1]
    acc = torch.zeros(x.shape[0], w.shape[0])
    starts = list(range(0, K, step))
    for k0 in (reversed(starts) if reverse else starts):
        acc = acc + x[:, k0:k0 + step] @ w[:, k0:k0 + step].T
        assert acc.dtype == torch.float32
    return acc


@pytest.mark.parametrize('M,N,K', [(33, 68, 72), (131, 124, 200), (95, 316, 104), (8, 1100, 1024), (5, 91, 2048)])
def test_gemm_exact_class_is_exact_in_f32(M, N, K):
    """The exact class: the operands lie on the grids the GPU module's docstring states, f32 sums of
    the products in two different orders both equal the f64 result, so does the f32 epilogue, and a
    16-bit output resolves one dropped product at every element."""
    x, w, acc, _ = R.gemm_case(M, N, K, torch.float32, 'exact')
    assert ((x * 2) == (x * 2).round()).all() and x.abs().max() <= 1
    assert ((w * 8) == (w * 8).round()).all() and w.abs().max() <= 0.25
    for dt in (torch.bfloat16, torch.float16):                 # representable in every compute type
        assert (x.to(dt).float() == x).all() and (w.to(dt).float() == w).all()
    # no (output column, 8-element K chunk) class is all zeros everywhere: a dropped chunk shows
    assert (w.view(N, K // 8, 8).abs().sum(-1) > 0).float().mean() > 0.3
    assert acc.abs().max() < 2 ** 9
    fwd, bwd = _f32_chunked(x, w, 8, False), _f32_chunked(x, w, 24, True)
    assert (fwd.double() == acc).all() and (bwd.double() == acc).all() and ((x @ w.T).double() == acc).all()
    g = torch.Generator().manual_seed(N)
    scale, bias = R.exact_epilogue(N, g)
    res = R.exact_res((M, N), g)
    assert set(scale.tolist()) <= {0.5, 1.0, 2.0} and ((bias * 4) == (bias * 4).round()).all()
    assert ((res * 4) == (res * 4).round()).all() and res.abs().max() <= 2
    assert (res.bfloat16().float() == res).all() and (res.half().float() == res).all()
    pre, _ = R.epilogue64(acc, scale, bias, res)
    assert ((fwd * scale + bias + res).double() == pre).all()          # the epilogue's three f32 operations
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        assert R.exact_headroom(pre, scale, dt).all()
        assert R.exact_headroom(acc, None, dt).all()
        # ... and the criterion means what it says: one product less changes the rounded output
        less, _ = R.epilogue64(acc - 1.0 / 16, scale, bias, res)
        assert (less.to(dt) != pre.to(dt)).all()
    # the criterion does reject a magnitude where bf16 would swallow the product
    assert not R.exact_headroom(torch.tensor([[40.0]], dtype=torch.float64), None, torch.bfloat16).all()


def test_conv_exact_class_is_exact_in_f32():
    for name in R.CONV_CASES:
        (KH, KW), stride, pad, B, H, W, Cin, Cout = R.CONV_CASES[name]
        x, w, acc, _ = R.conv_case(name, torch.float32, 'exact')
        cols = R.unfold_nhwc(x, KH, KW, stride, pad)
        wk = w.reshape(Cout, -1)
        assert ((cols @ wk.T).double() == acc).all()           # f32 im2col product == F.conv2d in f64
        assert (_f32_chunked(cols, wk, 8, True).double() == acc).all()
        assert R.exact_headroom(acc, None, torch.bfloat16).all()
    # C7b: the outermost ring of output windows lies wholly in the padding
    acc = R.conv_case('C7b', torch.float32, 'exact')[2].view(8, 9, -1)
    assert (acc[0] == 0).all() and (acc[-1] == 0).all() and (acc[:, 0] == 0).all() and (acc[:, -1] == 0).all()
    assert (R.conv_case('C7', torch.float32, 'exact')[2].view(6, 7, -1)[0, 0] != 0).any()


def test_x_add_exact_operand_needs_rounding():
    """The x_add case of the GPU module: the bf16 sum needs rounding (a truncating add differs), the
    rounded operand times exact-class W is still exact in f32."""
    g = torch.Generator().manual_seed(3)
    x = R.exact_x((33, 72), g)
    x2 = torch.randint(-7, 8, (33, 72), generator=g).float() / 512
    w = R.exact_w((68, 72), 72, g)
    assert (x2.bfloat16().float() == x2).all()
    s = x + x2
    rne = s.bfloat16().float()
    trunc = (s.view(torch.int32) & -65536).view(torch.float32)
    assert (rne != s).any() and (rne != trunc).any()
    a = rne.double()
    acc = a @ w.double().T
    assert ((rne @ w.T).double() == acc).all() and (_f32_chunked(rne, w, 8, True).double() == acc).all()
    assert ((trunc @ w.T).double() != acc).any()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize('M,N,K', [(67, 136, 200), (131, 124, 72), (95, 316, 104)])
def test_gemm_generic_bound_holds_for_torch_f32_and_rejects_defects(M, N, K, dtype):
    """torch's own f32 matmul + f32 epilogue + one output rounding stays inside the generic bound;
    the last 8-element K chunk dropped, and (f32 path) operands truncated to bf16, leave it."""
    x, w, acc, ap = R.gemm_case(M, N, K, dtype, 'generic')
    assert (x.to(dtype).float() == x).all() and (w.to(dtype).float() == w).all()
    g = torch.Generator().manual_seed(K)
    scale, bias = R.generic_epilogue(N, g)
    res = torch.randn(M, N, generator=g).to(dtype).float()
    pre, maj = R.epilogue64(acc, scale, bias, res, relu=True)
    bound = R.gemm_generic_bound(ap, K, maj, pre, dtype, scale)

    def f32_path(xx, ww):
        return torch.relu((xx @ ww.T) * scale + bias + res).to(dtype).double()
    err = (f32_path(x, w) - pre).abs()
    print(f'generic bound ({M}, {N}, {K}) {dtype}: torch f32 worst err / bound {(err / bound).max().item():.3f}')
    assert (err <= bound).all()
    dropped = (f32_path(x[:, :K - 8], w[:, :K - 8]) - pre).abs()
    assert (dropped > bound).float().mean() > 0.25
    if dtype == torch.float32:
        trunc = (f32_path(x.bfloat16().float(), w.bfloat16().float()) - pre).abs()
        assert (trunc > bound).float().mean() > 0.25
        # KINET_F32_X3's own bound is wider than the exact path's, and torch f32 is inside it too
        xb = R.gemm_generic_bound(R.x3_bound(x.double(), w.double().T), K, maj, pre, dtype, scale, x3=True)
        assert (bound <= xb).all() and (err <= xb).all() and (trunc > xb).any()


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=str)
@pytest.mark.parametrize('name', ['C1', 'C3'])
def test_conv_generic_bound_rejects_a_shifted_tap(name, dtype):
    """One filter tap reading its input one pixel to the right leaves the generic bound; torch's f32
    convolution stays inside it."""
    (KH, KW), stride, pad, B, H, W, Cin, Cout = R.CONV_CASES[name]
    x, w, acc, ap = R.conv_case(name, dtype, 'generic')
    K = KH * KW * Cin
    pre, maj = R.epilogue64(acc)
    bound = R.gemm_generic_bound(ap, K, maj, pre, dtype)
    xn, wn = x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2)
    good = F.conv2d(xn, wn, stride=stride, padding=pad).permute(0, 2, 3, 1).reshape(-1, Cout)
    assert ((good.to(dtype).double() - pre).abs() <= bound).all()
    tap = torch.zeros_like(wn)
    tap[:, :, KH // 2, KW // 2] = wn[:, :, KH // 2, KW // 2]
    bad = F.conv2d(xn, wn - tap, stride=stride, padding=pad) + F.conv2d(torch.roll(xn, -1, 3), tap, stride=stride, padding=pad)
    bad = bad.permute(0, 2, 3, 1).reshape(-1, Cout)
    assert ((bad.to(dtype).double() - pre).abs() > bound).float().mean() > 0.25


def test_gemm_table_covers_the_k_cycle():
    for bm, bn in R.GEMM_TILES:
        for four in (False, True):
            t = R.gemm_table(bm, bn, four)
            ks = R.GEMM_K32 if four else R.GEMM_K16
            step = 32 if four else 64
            assert sorted(-(-k // step) for k in ks) == [1, 1, 1, 2, 3, 4]
            for k in ks:
                assert len({(M, N) for M, N, kk in t if kk == k}) >= 2
            assert {(M, N) for M, N, _ in t} == set(R.gemm_shapes(bm, bn)) and len(R.gemm_shapes(bm, bn)) == 9
            assert all(k % 8 == 0 and k <= 392 for k in ks)
    # the 15-block grid of the XCD remap (15 = 8 + 7: both branches of the bijection)
    assert all(-(-(3 * bm - 1) // bm) * -(-(5 * bn - 4) // bn) == 15 for bm, bn in R.GEMM_TILES)


# ======================================= resident-weight GEMM (csrc/gemm_rw.hip)
# The configuration columns of R.RW_CASES (KC, NT, BMR, NS, NW, OCC, ng) state what the launchers are
# read to choose; without a GPU they can be cross-checked only as far as they are literal -- against
# each other and against the shapes -- which is what test_rw_tables_are_consistent does.  The rest
# checks the references and the acceptance of tests/test_gemm_rw_direct_gpu.py.
_RW_PLAIN = [c for c in R.RW_CASES if 'LN' not in R.rw_opts(c)]
_RW_LN = [c for c in R.RW_CASES if 'LN' in R.rw_opts(c)]
_rw_id = lambda c: c[0].replace(' ', '_')          # noqa: E731


def _rw_f32(inp, cdt, odt, x=None, w=None, res=None, mask=None):
    """The case in torch's own f32: (x [+ x2] rounded to cdt) @ w^T, the f32 epilogue, LayerNorm, the row
    mask, one output rounding.  x / w / res / mask override the case's operands (emulated defects)."""
    x = inp['x'] if x is None else x
    w = inp['w'] if w is None else w
    res = inp['res'] if res is None else res
    mask = inp['mask'] if mask is None else mask
    if inp['x2'] is not None:
        x = (x + inp['x2'][:, :x.shape[1]]).to(cdt).float()
    v = x @ w.T
    if inp['scale'] is not None:
        v = v * inp['scale']
    if inp['bias'] is not None:
        v = v + inp['bias']
    if res is not None:
        v = v + res
    if inp['relu']:
        v = torch.relu(v)
    if inp['ln'] is not None:
        v = F.layer_norm(v, (v.shape[-1],), inp['ln'][0], inp['ln'][1], 1e-5)
    assert v.dtype == torch.float32
    return R.rw_masked(v, mask).to(odt)


def _rw_accepts(got, inp, case, cls):
    """The GPU module's acceptance of an (M, N) output."""
    Kd, odt = case[1], case[6]
    if inp['ln'] is not None:
        return R.rw_ln_check(got, inp, odt)[1] == 0
    if cls == 'exact':
        return bool((got == R.rw_masked(inp['pre'], inp['mask']).to(odt)).all())
    return R.rw_generic_ratio(got, inp, Kd, odt) <= 1.0


def test_rw_tables_are_consistent():
    names = [c[0] for c in R.RW_CASES]
    assert len(set(names)) == len(names)
    combos = {}
    layouts = set()
    for name, K, N, flags, opts, cdt, odt, (KC, NT, BMR, NS, NW, OCC), ng in R.RW_CASES:
        o = R.rw_opts((name, K, N, flags, opts))
        GW = NW * NT * 16
        assert KC * 32 == K and K in (64, 128, 256, 512, 288) and N % 8 == 0, name
        assert ng == -(-N // GW), name
        assert BMR in (16, 32) and R.rw_rows(BMR) == {16: 267, 32: 539}[BMR] and 2 <= NS <= 4, name
        assert R.rw_rows(BMR) > 256 and -(-R.rw_rows(BMR) // BMR) == R.RW_TILES and R.rw_rows(BMR) % BMR, name
        assert (NW, OCC) in ((4, 2), (8, 1), (9, 1), (6, 1)), name
        # what the kernel accepts: a residual is of a 16-bit output type; LayerNorm rows fit one group
        assert 'R' not in o or odt != torch.float32, name
        assert 'LN' not in o or (ng == 1 and N <= (288 if K == 288 else 256) and 'relu' not in o), name
        assert 'A2' not in o or not (o & {'R', 'LN'}), name
        assert K != 512 or (N <= 256 and not (o & {'R', 'LN', 'A2'})), name
        assert (K == 64) <= (BMR == 32), name
        combos.setdefault(K, set()).add((cdt, odt if odt != torch.float32 else 'f32'))
        layouts |= {d for d in (0, -56, 8) if N % GW == d % GW} | ({'ld'} if 'ld' in o else set())
    B_, H_ = torch.bfloat16, torch.float16
    for K, seen in combos.items():
        assert {(B_, B_), (H_, H_), (B_, H_)} <= seen and any(t[1] == 'f32' for t in seen), (K, seen)
    assert layouts == {0, -56, 8, 'ld'}
    assert R.RW_CAPS == {0: 17, 1: 1, 3: 3, 16: 16}
    # cap 3: 6 / 6 / 5 tiles, the ragged tile (16) walked last by workgroup 1; cap 16: 2 tiles on workgroup 0
    assert [len(range(b, 17, 3)) for b in range(3)] == [6, 6, 5] and 16 in range(1, 17, 3)
    assert [len(range(b, 17, 16)) for b in range(16)] == [2] + [1] * 15
    for bmr in (16, 32):
        M = R.rw_rows(bmr)
        m = R.rw_mask(M, bmr)
        assert m[0] and m[M - 1] and m[6 * bmr:7 * bmr].all() and not m[5 * bmr:6 * bmr].any() and not m[7 * bmr]
        assert m[2 * bmr] and not m[2 * bmr - 1] and not m[2 * bmr + 1]         # a tile's first row
        assert m[4 * bmr - 1] and not m[4 * bmr - 2] and not m[4 * bmr]          # a tile's last row
        assert R.rw_hm_batch(bmr)[0] * R.rw_hm_batch(bmr)[1] == M
    for name, (KH, Cin, Cout, stride, pad_h, Hin, Win), flags, opts, cfg, ng in R.RW_CONV_CASES:
        Ho, Wo = R.out_size(Hin, Win, KH, 1, stride, (pad_h, 0))
        assert (Ho, Wo) == (4, 33) and R.RW_CONV_BATCH * Ho * Wo == R.RW_CONV_ROWS >= 256 and KH * Cin <= 256, name
        assert Wo >= cfg[2] and Wo % cfg[2] and (Ho * Wo) % cfg[2], name      # tiles straddle rows and the image
        assert ng == -(-Cout // (cfg[4] * cfg[1] * 16)) and cfg[0] == 8, name
    exp = R.rw_expected((8, 4, 16, 4, 8, 1), 2, True, False, False, torch.bfloat16, 3)
    assert tuple(exp) == R.RW_CONFIG_FIELDS and exp['P'] == 3 and exp['n_mtiles'] == 17 and exp['out_bytes'] == 2


def test_rw_config_fields_match_the_wrapper():
    from kinet_amd import kernels
    assert kernels.GEMM_RW_CONFIG_FIELDS == R.RW_CONFIG_FIELDS


@pytest.mark.parametrize('case', _RW_PLAIN, ids=_rw_id)
def test_rw_exact_cases_are_exact_with_headroom(case):
    """Every exact-class row: operands on their grids (x + x2 exact in the operand type), torch's f32
    evaluation equals the f64 one, and the output type resolves one dropped product everywhere."""
    name, K, N, _, _, cdt, odt, cfg, _ = case
    inp = R.rw_inputs(case, 'exact')
    a = inp['x'] if inp['x2'] is None else inp['x'] + inp['x2']
    assert (a.to(cdt).float() == a).all() and (inp['w'].to(cdt).float() == inp['w']).all()
    assert ((a * 2) == (a * 2).round()).all() and a.abs().max() <= (1 if inp['x2'] is None else 2)
    assert ((a @ inp['w'].T).double() == inp['acc']).all() and inp['acc'].abs().max() < 2 ** 9
    assert (_f32_chunked(a, inp['w'], 32, True).double() == inp['acc']).all()
    if inp['res'] is not None:
        assert (inp['res'].to(odt).float() == inp['res']).all()
    want = R.rw_masked(inp['pre'], inp['mask'])
    assert R.exact_headroom(inp['pre'], inp['scale'], odt).all(), name
    got = _rw_f32(inp, cdt, odt)
    assert (got == want.to(odt)).all() and _rw_accepts(got, inp, case, 'exact')
    less = R.epilogue64(inp['acc'] - 1.0 / 16, inp['scale'], inp['bias'], inp['res'], False)[0]
    assert (less.to(odt) != R.epilogue64(inp['acc'], inp['scale'], inp['bias'], inp['res'], False)[0].to(odt)).all()


@pytest.mark.parametrize('case', R.RW_CASES, ids=_rw_id)
def test_rw_generic_and_ln_bounds_hold_for_torch_f32(case):
    cdt, odt = case[5], case[6]
    if 'LN' in R.rw_opts(case):
        for offset in (100.0, 0.0):
            inp = R.rw_inputs(case, 'exact', offset)
            assert _rw_accepts(_rw_f32(inp, cdt, odt), inp, case, 'exact')
    else:
        inp = R.rw_inputs(case, 'generic')
        got = _rw_f32(inp, cdt, odt)
        print(f'{case[0]}: torch f32 worst err / bound {R.rw_generic_ratio(got, inp, case[1], odt):.3f}')
        assert _rw_accepts(got, inp, case, 'generic')


_RW_DEFECT_CASES = [c for c in R.RW_CASES if c[0] in (
    'k64 R', 'k64 R+LN', 'k128 R 8-wave', 'k128 LN', 'k256 plain ld', 'k256 R 8-wave', 'k256 R+LN', 'k256 A2',
    'k512 8-wave', 'k512 N=72', 'k288 R+LN 9-wave', 'k288 LN 6-wave', 'k288 R', 'k288 N=1728 4-wave', 'k288 A2 8-wave N=328')]


@pytest.mark.parametrize('case,cls', [(c, cls) for c in _RW_DEFECT_CASES for cls in ('exact', 'generic')
                                      if cls == 'exact' or 'LN' not in R.rw_opts(c)],
                         ids=lambda v: _rw_id(v) if isinstance(v, tuple) else v)
def test_rw_acceptance_rejects_emulated_defects(case, cls):
    """Defects of the kind this kernel can have, emulated on torch's f32 evaluation: each leaves the GPU
    module's acceptance (in both operand classes; LayerNorm rows have one class, at offset 0)."""
    name, K, N, _, _, cdt, odt, (KC, NT, BMR, NS, NW, OCC), _ = case
    o = R.rw_opts(case)
    inp = R.rw_inputs(case, cls)
    M = R.rw_rows(BMR)
    good = _rw_f32(inp, cdt, odt)
    assert _rw_accepts(good, inp, case, cls)
    # the last 8-element K chunk dropped
    assert not _rw_accepts(_rw_f32(inp, cdt, odt, x=inp['x'][:, :K - 8], w=inp['w'][:, :K - 8]), inp, case, cls)
    # a tile's rows computed from the tile NS earlier (a ring slot read before its DMA landed)
    t = NS + 1
    stale = good.clone()
    stale[t * BMR:(t + 1) * BMR] = _rw_f32(inp, cdt, odt, mask=torch.zeros(M, dtype=torch.bool))[(t - NS) * BMR:(t - NS + 1) * BMR]
    assert not _rw_accepts(stale, inp, case, cls)
    # ... and only that tile's A rows stale, residual and mask in place
    xs = inp['x'].clone()
    xs[t * BMR:(t + 1) * BMR] = inp['x'][(t - NS) * BMR:(t - NS + 1) * BMR]
    assert not _rw_accepts(_rw_f32(inp, cdt, odt, x=xs), inp, case, cls)
    if 'R' in o:        # the residual read one 8-column chunk off
        assert not _rw_accepts(_rw_f32(inp, cdt, odt, res=torch.roll(inp['res'], 8, 1)), inp, case, cls)
    if 'mask' in o:     # a mask byte applied to the neighbouring row
        assert not _rw_accepts(_rw_f32(inp, cdt, odt, mask=torch.roll(inp['mask'], 1)), inp, case, cls)


@pytest.mark.parametrize('case', R.RW_HM_CASES, ids=_rw_id)
def test_rw_headmajor_acceptance_rejects_a_plane_offset(case):
    """The head-major cases: exact with headroom, and planes stored one head off are not accepted."""
    name, d, hd, _, cdt, odt, cfg, _ = case
    M = R.rw_rows(cfg[2])
    x, w, acc, _ = R.gemm_case(M, d, d, cdt, 'exact')
    bias = R.exact_epilogue(d, torch.Generator().manual_seed(d + cfg[2] + len(name)))[1]
    pre = R.epilogue64(acc, None, bias)[0]
    assert R.exact_headroom(pre, None, odt).all()
    want = R.rw_masked(pre, R.rw_mask(M, cfg[2])).to(odt)
    h = 36 if hd == 'split' else hd
    B, S = R.rw_hm_batch(cfg[2])
    stored = R.rw_hm_layout(want, B, S, h)                 # (d // h, B, S, h), as the kernel writes it
    assert torch.equal(R.rw_hm_rows(stored), want)

    def rejected(y):    # the GPU test's acceptance: every element of the permuted-back output equal
        return float((R.rw_hm_rows(y) != want).any(1).float().mean())
    assert rejected(torch.roll(stored, 1, 0)) > 0.9         # every plane stored one head off
    assert rejected(torch.roll(stored, 1, 2)) > 0.9         # ... one row off inside its plane
    one = stored.clone()
    one[3] = stored[2]                                      # one plane holding its neighbour's values
    assert 0 < rejected(one) and (R.rw_hm_rows(one) != want).any(0).sum() == h
    if hd == 'split':   # the two planes of a 36-column head: only the 4-column tail planes one head off
        tail = stored.clone()
        tail[..., 32:] = torch.roll(stored[..., 32:], 1, 0)
        assert rejected(tail) > 0.9 and not (R.rw_hm_rows(tail) != want).view(M, d // h, h)[..., :32].any()


@pytest.mark.parametrize('name', [c[0] for c in R.RW_CONV_CASES])
def test_rw_conv_cases_exact_and_bounded(name):
    geo, opts = next((c[1], c[3]) for c in R.RW_CONV_CASES if c[0] == name)
    KH, Cin, Cout, stride, pad_h, Hin, Win = geo
    for dt in (torch.bfloat16, torch.float16):
        x, w, scale, bias, acc, ap = R.rw_conv_inputs(name, dt, 'exact')
        cols = R.unfold_nhwc(x, KH, 1, stride, (pad_h, 0))
        assert ((cols @ w.reshape(Cout, -1).T).double() == acc).all()
        pre, _ = R.epilogue64(acc, scale, bias, None, 'relu' in opts.split())
        assert R.exact_headroom(R.epilogue64(acc, scale, bias)[0], scale, dt).all()
        if KH == 3:
            assert (acc.view(2, 4, 33, Cout)[:, [0, 3]] == 0).all() and (acc.view(2, 4, 33, Cout)[:, 1:3] != 0).any()
        x, w, scale, bias, acc, ap = R.rw_conv_inputs(name, dt, 'generic')
        pre, maj = R.epilogue64(acc, scale, bias, None, 'relu' in opts.split())
        bound = R.gemm_generic_bound(ap, KH * Cin, maj, pre, dt, scale)
        cols = R.unfold_nhwc(x, KH, 1, stride, (pad_h, 0))
        v = cols @ w.reshape(Cout, -1).T
        v = v if scale is None else v * scale
        v = v if bias is None else v + bias
        v = torch.relu(v) if 'relu' in opts.split() else v
        assert ((v.to(dt).double() - pre).abs() <= bound).all()
        # the rows of one output row taken from the row above (a wrong carry at the row's end) leave it
        bad = torch.roll(v.view(2, 4, 33, Cout), 1, 1).reshape(-1, Cout)
        assert ((bad.to(dt).double() - pre).abs() > bound).float().mean() > 0.25


# ============================================================ MSDA forward sampling
def _shapes(a):
    return tuple((int(h), int(w)) for h, w in np.asarray(a).tolist())


@pytest.mark.parametrize('name', ['msda_kat_f32.npz', 'msda_kat_f64.npz', 'msda_mid_d32.npz', 'msda_mid_d36.npz'])
def test_msda_sample_ref_equals_both_oracles(golden_dir, name):
    import os
    from oracle import msda_oracle as O
    d = dict(np.load(os.path.join(golden_dir, name)))
    v, loc, aw = (torch.from_numpy(d[k]).double() for k in ('value', 'loc', 'attw'))
    r = R.msda_sample_ref(v, _shapes(d['shapes']), loc, aw)
    scale = r['A'].max().item()
    assert (r['out'] - torch.from_numpy(O.fwd(v.numpy(), d['shapes'], loc.numpy(), aw.numpy()))).abs().max().item() <= 1e-14 * scale
    assert (r['out'] - O.core_pytorch(v, d['shapes'], loc, aw)).abs().max().item() <= 1e-13 * scale
    assert (r['out'].abs() <= r['A'] * (1 + 1e-12)).all() and torch.allclose(r['A_lvl'].sum(0), r['A'])


def test_msda_sample_ref_on_the_padding_edges():
    """Samples exactly at h = -1, -0.5, H - 0.5 and H (and the same in w): the validity test's open
    ends and the half-outside footprints, against both oracles."""
    from oracle import msda_oracle as O
    shapes = ((5, 7), (3, 4))
    g = torch.Generator().manual_seed(3)
    S = sum(h * w for h, w in shapes)
    B, M, D, P = 1, 2, 4, 4
    v = torch.randn(B, S, M, D, generator=g).double()
    hs = [-1.0, -0.5, 0.0, 'H-0.5', 'H']
    loc = torch.zeros(B, len(hs) ** 2, M, 2, P, 2, dtype=torch.float64)
    for l, (H, W) in enumerate(shapes):
        for i, hh in enumerate(hs):
            for j, ww in enumerate(hs):
                h = {'H-0.5': H - 0.5, 'H': float(H)}.get(hh, hh)
                w = {'H-0.5': W - 0.5, 'H': float(W)}.get(ww, ww)
                loc[0, i * len(hs) + j, :, l, :, 0] = (w + 0.5) / W
                loc[0, i * len(hs) + j, :, l, :, 1] = (h + 0.5) / H
    aw = torch.rand(B, len(hs) ** 2, M, 2, P, generator=g).double()
    r = R.msda_sample_ref(v, shapes, loc, aw)
    ss = np.array(shapes, dtype=np.int64)
    assert (r['out'] - torch.from_numpy(O.fwd(v.numpy(), ss, loc.numpy(), aw.numpy()))).abs().max().item() <= 1e-14
    # grid_sample's own coordinate arithmetic (2 loc - 1, unnormalised again) moves a knot by an ulp: its
    # error is the slope times that, not f64 rounding of the sum
    assert ((r['out'] - O.core_pytorch(v, ss, loc, aw)).abs() <= r['G'] * 1e-13 + 1e-14).all()
    # h = -1 and h = H add nothing; h = -0.5 keeps half of row 0
    assert (r['out'][0, :len(hs)] == 0).all() and (r['out'][0, -len(hs):] == 0).all()
    assert (r['out'][0, len(hs) + 2] != 0).all()


def test_msda_slope_covers_a_location_error():
    """G d bounds the change under a perturbation of every tap by up to d pixels per axis, across cell
    borders and the padding edges: 1,000 random taps, d from 1e-6 to 0.9."""
    shapes = ((6, 9), (4, 5), (3, 3), (2, 2))
    g = torch.Generator().manual_seed(11)
    S = sum(h * w for h, w in shapes)
    B, Lq, M, D, P = 1, 63, 1, 3, 4            # 63 * 16 = 1,008 taps
    v = torch.randn(B, S, M, D, generator=g).double()
    loc = torch.rand(B, Lq, M, 4, P, 2, generator=g).double() * 1.6 - 0.3
    # a third of the taps on cell borders and the padding edges
    for l, (H, W) in enumerate(shapes):
        knots = (torch.randint(-1, H + 1, (B, Lq, M, P), generator=g).double() + 0.5) / H
        on = torch.rand(B, Lq, M, P, generator=g) < 0.33
        loc[:, :, :, l, :, 1] = torch.where(on, knots, loc[:, :, :, l, :, 1])
    aw = torch.rand(B, Lq, M, 4, P, generator=g).double()
    r = R.msda_sample_ref(v, shapes, loc, aw)
    size = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64).view(1, 1, 1, 4, 1, 2)
    for d in (1e-6, 1e-3, 0.124, 0.9):
        for _ in range(3):
            step = (torch.rand(loc.shape, generator=g).double() * 2 - 1) * d
            step = torch.where(torch.rand(loc.shape, generator=g) < 0.5, step.sign() * d, step)
            moved = R.msda_sample_ref(v, shapes, loc + step / size, aw)['out']
            assert ((moved - r['out']).abs() <= r['G'] * d * (1 + 1e-9) + 1e-14).all(), d
    # and it is not vacuous: a full pixel exceeds G * 1e-3 nearly everywhere
    moved = R.msda_sample_ref(v, shapes, loc + 1.0 / size, aw)['out']
    assert ((moved - r['out']).abs() > r['G'] * 1e-3).float().mean() > 0.9


@pytest.fixture
def strips():
    """msda_encoder_set_strips for one test, restored afterwards."""
    from kinet_amd import kernels as K
    old = K.msda_encoder_set_strips(0)
    yield K.msda_encoder_set_strips
    K.msda_encoder_set_strips(old)


@pytest.mark.parametrize('case', R.MSDA_ENC_CASES, ids=lambda c: '-'.join(map(str, c[:5])))
def test_msda_encoder_plan_table(strips, case):
    """Every literal row of MSDA_ENC_CASES against kinet_msda_encoder_plan_ex (no GPU: the planner
    assumes 256 compute units), and the windows' restatement against the plan's size."""
    from kinet_amd import kernels as K
    name, B, M, ch, forced, want = case
    shapes = R.MSDA_ENC_GEO[name]
    S = sum(h * w for h, w in shapes)
    strips(forced)
    got = K.msda_encoder_plan(shapes, B, M, S, ch)
    assert got is not None and got[:3] == want and got[3] == B * M * want[1], (got, want)
    fl, n, used = want
    caps = R.msda_enc_caps(shapes, fl, n)
    ceil16 = lambda x: (x + 15) // 16 * 16
    assert used == ceil16(max(w for _, w in shapes[fl:]) + 2) + sum(ceil16(c * w + 2) for c, (_, w) in zip(caps, shapes) if c)
    assert used <= (R.ENC_TAIL if ch == 36 else R.ENC_MAIN)
    strip_of, win = R.msda_enc_windows(shapes, fl, n)
    assert sorted(set(strip_of.tolist())) == list(range(n))
    for l in range(fl, 4):
        assert ((win[:, l] >= -1) & (win[:, l] + caps[l] - 1 <= shapes[l][0])).all()


def test_msda_encoder_plan_refusal(strips):
    from kinet_amd import kernels as K
    shapes = R.MSDA_ENC_REFUSED
    S = sum(h * w for h, w in shapes)
    for forced in (0, 4):
        strips(forced)
        assert K.msda_encoder_plan(shapes, 1, 8, S) is None and K.msda_encoder_plan(shapes, 1, 8, S, 36) is None


def test_msda_plan_table_reaches_every_plan():
    fls = {(c[5][0], c[3]) for c in R.MSDA_ENC_CASES}
    assert {(f, 32) for f in range(4)} <= fls and (3, 36) in fls and (1, 36) in fls
    # staged levels taller than their window (the far path is reachable) under fl = 0 and fl >= 1
    tall = {c[5][0] for c in R.MSDA_ENC_CASES
            if any(cap and cap < h for cap, (h, _) in zip(R.msda_enc_caps(R.MSDA_ENC_GEO[c[0]], c[5][0], c[5][1]),
                                                         R.MSDA_ENC_GEO[c[0]]))}
    assert {0, 1} <= tall
    # 8 and 10 fraction bits of the records
    assert max(w for _, w in R.MSDA_ENC_GEO['wide1']) > 128 >= max(w for _, w in R.MSDA_ENC_GEO['all'])


# ---- the tests can fail: emulated defects in a copy of the reference chain ----
def _defective_chain(case, shapes, M, defect, plan=None, P=4):
    """msda_prep_ref + msda_sample_ref restated with one defect switched on (None: the faithful copy)."""
    L = len(shapes)
    offlog, refs, qmask = case['offlog'].double(), case['refs'].double(), case.get('qmask')
    B, Lq = offlog.shape[:2]
    n = M * L * P
    o = offlog[..., :2 * n].reshape(B, Lq, M, L, P, 2)
    lg = offlog[..., 2 * n:].reshape(B, Lq, M, L, P)
    a = (torch.softmax(lg, -1) if defect == 'softmax4' else torch.softmax(lg.reshape(B, Lq, M, L * P), -1)).reshape(B, Lq, M, L, P)
    if qmask is not None and defect != 'mask':
        a = a.masked_fill(qmask[:, :, None, None, None], 0.0)
    if defect == 'drop23':
        a = a.clone()
        a[:, :, :, 2, 3] = 0
    sh = torch.tensor(shapes, dtype=torch.float64)
    div = sh.flip(1) if defect == 'xbyW' else sh
    rxy = refs[..., :2][:, :, None, :, None, :]
    loc = rxy + (o / div[None, None, None, :, None, :] if refs.shape[-1] == 2
                 else o / P * refs[..., 2:][:, :, None, :, None, :] * 0.5)
    value = case['value'].double()
    D = value.shape[-1]
    fl, ns = plan if plan is not None else (L, 1)
    caps = R.msda_enc_caps(shapes, fl, ns)
    strip_of, win = R.msda_enc_windows(shapes, fl, ns) if plan is not None else (None, None)
    bi, mi = torch.arange(B).view(B, 1, 1, 1), torch.arange(M).view(1, 1, M, 1)
    out = torch.zeros(B, Lq, M, D, dtype=torch.float64)
    start = 0
    for l, (H, W) in enumerate(shapes):
        s0 = start + (W if defect == 'start' and l else 0)
        v = value[:, s0:s0 + H * W]
        v = torch.cat([v, value[:, :H * W - v.shape[1]]], 1)            # (the shifted last level wraps)
        h = loc[:, :, :, l, :, 1] * H - 0.5
        w = loc[:, :, :, l, :, 0] * W - 0.5
        valid = (h > -1) & (w > -1) & (h < H) & (w < W)
        hl, wl = torch.floor(h), torch.floor(w)
        lh, lw = h - hl, w - wl
        if defect == 'swap':
            lw = 1 - lw
        far = short = torch.zeros_like(valid)
        if strip_of is not None and l >= fl:
            r0 = torch.as_tensor(win[strip_of[(torch.arange(Lq) // 16).numpy()], l]).double()[None, :, None, None]
            far = (hl < r0) | (hl >= r0 + caps[l] - 1)
            short = hl == r0 + caps[l] - 2
        for dy, wy in ((0, 1 - lh), (1, lh)):
            for dx, wx in ((0, 1 - lw), (1, lw)):
                r, c = hl + dy, wl + dx
                ok = valid & (r >= 0) & (r < H) & (c >= 0) & (c < W) if defect != 'clamp' else valid
                if defect == 'short' and dy == 1:
                    ok = ok & ~short
                idx = (r.clamp(0, H - 1) * W + c.clamp(0, W - 1)).long()
                if defect == 'far' and dy == 1 and dx == 1:
                    idx = torch.where(far, (idx + 1).clamp(max=H * W - 1), idx)
                vc = v[bi, idx, mi]
                if defect == 'tail':
                    vc = torch.cat([vc[..., :32], v[bi, (idx + 1).clamp(max=H * W - 1), mi][..., 32:]], -1)
                out += ((a[:, :, :, l] * wy * wx * ok)[..., None] * vc).sum(3)
        start += H * W
    return out.reshape(B, Lq, M * D)


# defect -> (class, head_dim, the named case): 'addr' = MSDA_ENC_GEO['all'] with 3 strips (Lq = S, B = 1,
# M = 8), 'generic' = the same geometry, 3-pixel offsets, randn logits, 10 % masked queries
DEFECTS = {'xbyW': ('addr', 32), 'start': ('addr', 32), 'short': ('addr', 32), 'swap': ('generic', 32),
           'clamp': ('addr', 32), 'drop23': ('addr', 32), 'tail': ('addr', 36), 'mask': ('generic', 32),
           'far': ('addr', 32), 'softmax4': ('generic', 32)}


@functools.lru_cache(maxsize=None)
def _defect_case(cls, D):
    shapes, M, plan = R.MSDA_ENC_GEO['all'], 8, (0, 3)
    S = sum(h * w for h, w in shapes)
    if cls == 'addr':
        case = R.msda_addr_case(shapes, 1, M, S, 2, D=D, plan=plan)
    else:
        case = R.msda_generic_case(shapes, 1, M, S, 2, 3.0, 'randn', torch.float16, D=D)
    prep, samp = R.msda_chain_ref(case, shapes, M)
    # the loosest bound a test of this class applies (the strip kernel's, bf16 output)
    bound = R.msda_addr_bound(samp, shapes, 'strip', prep['locA']) if cls == 'addr' else \
        R.msda_bound(samp, shapes, 'strip', torch.bfloat16, prep['locA'], prep['attw_c'])
    return case, shapes, M, plan, samp, bound


@pytest.mark.parametrize('defect', [None] + sorted(DEFECTS))
def test_msda_emulated_defects_are_caught(defect):
    cls, D = DEFECTS.get(defect, ('addr', 32))
    for c in ([cls] if defect else ['addr', 'generic']):
        case, shapes, M, plan, samp, bound = _defect_case(c, D)
        out = _defective_chain(case, shapes, M, defect, plan)
        bad = (out - samp['out']).abs() > bound
        if defect is None:
            assert (out - samp['out']).abs().max().item() <= 1e-12      # the copy is faithful
        else:
            assert bad.any(), defect
            print(defect, c, 'elements outside the bound:', int(bad.sum()), 'of', bad.numel())


@pytest.mark.parametrize('noise,logits', [(0.5, 'randn'), (3.0, 'pm8'), (25.0, 'randn')])
def test_msda_generic_bound_has_headroom(noise, logits):
    """torch's own f32 evaluation (softmax, locations, grid_sample) stays inside the TIGHTEST generic bound
    (f32 weights and accumulation, f32 output)."""
    from oracle import msda_oracle as O
    shapes, M = R.MSDA_ENC_GEO['all'], 8
    S = sum(h * w for h, w in shapes)
    case = R.msda_generic_case(shapes, 1, M, S, 2, noise, logits, torch.float32)
    prep, samp = R.msda_chain_ref(case, shapes, M)
    loc, aw = O.prep(case['offlog'], case['refs'], shapes, case['qmask'], M, 4, 4)
    out = O.core_pytorch(case['value'], shapes, loc, aw)
    bound = R.msda_bound(samp, shapes, 'f32', torch.float32, prep['locA'], prep['attw_c'])
    ratio = ((out.double() - samp['out']).abs() / bound).max().item()
    print('torch f32 err / bound:', ratio)
    assert ratio < 1


# ------------------------------------------ fused FFN / bottleneck pairs (test_ffn_direct_gpu.py)
_FFN_DT = [torch.bfloat16, torch.float16]
_FFN_MATS = {'ffn': ('W1', 'W2'), 'attn_out_ffn': ('Wo', 'W1', 'W2'), 'pair': ('W3', 'W1'), 'pair_ds': ('W3', 'Wds', 'W1')}
# the GEMMs of an entry point: name -> (left operand: input key or reference key, the value its sum feeds through a
# ReLU, if any).  A product counts as a probe only where that value is not clipped in the reference: below zero the
# ReLU hides a missing product from any test (the issue's rule for phase B, h != 0, extended to every ReLU).
_FFN_GEMMS = {'ffn': {'W1': ('x', 'h'), 'W2': ('h', None)},
              'attn_out_ffn': {'Wo': ('A', None), 'W1': ('x', 'h'), 'W2': ('h', None)},
              'pair': {'W3': ('X', 'preY'), 'W1': ('Y', 'preT')},
              'pair_ds': {'W3': ('X', 'preY'), 'Wds': ('X0', 'preY'), 'W1': ('Y', 'preT')}}
FFN_PROBES = 256


def _ffn_weight(case, d, key, dtype):
    """The weight matrix a GEMM multiplies by, as the kernel holds it."""
    if case[0] in ('pair', 'pair_ds'):
        return R.scaled_rows(d[key], d[{'W3': 's3', 'Wds': 'sds', 'W1': 's1'}[key]], dtype)
    return d[key].double()


@pytest.mark.parametrize('case', R.FFN_DIRECT_CASES, ids=R.ffn_case_id)
def test_ffn_exact_cases_are_exact_dense_and_resolve_every_product(case):
    """The exact class of every row of FFN_DIRECT_CASES, in both dtypes: every 16-bit operand, every rounded
    intermediate and the output are representable; every partial sum is exact in f32 in any order (all terms are
    multiples of 1/16 and the sums of their magnitudes stay below 2^20); every 1-KiB fragment of the packed stream
    holds at least 4 non-zero weights (through kinet_ffn_pack_map) and every 32-unit hidden chunk is live in every
    16-row tile; and 256 seeded single products per GEMM, taken out of the reference one at a time, each change the
    rounded output."""
    from kinet_amd import kernels as K
    kind, D, F_, DB, M = case[:5]
    d = R.ffn_direct_inputs(case, 'exact')
    mats = _FFN_MATS[kind]
    pm = K.ffn_pack_map(kind, D, F_, DB).long()
    nzw = torch.zeros(pm.shape[0], dtype=torch.bool)
    for i, key in enumerate(mats):
        sel = pm[:, 0] == i
        nzw[sel] = d[key][pm[sel, 1], pm[sel, 2]] != 0
    per_fragment = nzw.view(-1, 512).sum(1)
    assert int(per_fragment.min()) >= 4, f'a fragment with {int(per_fragment.min())} non-zero weights'

    for dtype in _FFN_DT:
        ref = R.ffn_direct_ref(case, d, dtype)
        outs = R.ffn_direct_outputs(case, ref)
        for key in ('x', 'A', 'R', 'X', 'X0'):
            if key in d:
                assert torch.equal(R.rnd(d[key].double(), dtype), d[key].double()), f'{key} is not representable'
        for key in mats:
            w = _ffn_weight(case, d, key, dtype)
            src = d[key].double() * (1 if kind in ('ffn', 'attn_out_ffn') else d[{'W3': 's3', 'Wds': 'sds', 'W1': 's1'}[key]].double().view(-1, 1))
            assert torch.equal(w, src), f'{key}: the scaled weight is not representable'
        hidden = ref['h'] if 'h' in ref else ref['Y']
        for name, v in list(outs.items()) + [('hidden', hidden)]:
            assert torch.equal(R.rnd(v, dtype), v), f'{name} is not representable in {dtype}'
            assert torch.equal(v * 16, (v * 16).round())
        if kind == 'attn_out_ffn':
            S = d['S'].double()
            assert torch.equal(ref['pre1'], S) and (S.sum(1) == 0).all() and d['eps1'] == 3.0
            want = S * 0.5 * d['g1'].double() + d['be1'].double()
            assert torch.equal(ref['x'], want) and (ref['x'] != 0).all()
            for f in (1 - 2.0 ** -20, 1 + 2.0 ** -20):        # an rsqrtf(4) that is not exactly 1/2 moves nothing
                assert torch.equal(R.rnd(S * 0.5 * f * d['g1'].double() + d['be1'].double(), dtype), want)
        # sums of magnitudes: every partial sum of multiples of 1/16 below 2^20 is exact in f32
        assert float(ref['absA'].max()) < 2 ** 20 and float(ref['majA'].max()) < 2 ** 20 and float(ref['majB'].max()) < 2 ** 20
        if kind == 'attn_out_ffn':
            assert float(ref['majO'].max()) < 2 ** 20
        # live hidden chunks: (16-row tile, 32-unit chunk)
        tiles = (hidden != 0)[:M - M % 16].view(-1, 16, hidden.shape[1] // 32, 32).any(3).any(1)
        assert tiles.all() and (hidden != 0)[M - M % 16:].view(-1, hidden.shape[1] // 32, 32).any(2).any(0).all()

        base = {k: R.rnd(v, dtype) for k, v in outs.items()}
        for gi, (name, (left, fed)) in enumerate(_FFN_GEMMS[kind].items()):
            L = (d[left] if left in d else ref[left]).double()
            W = _ffn_weight(case, d, name, dtype)
            g = torch.Generator().manual_seed(1000 * gi + D + F_ + M)
            n_draw = 600000
            m = torch.randint(0, M, (n_draw,), generator=g)
            n = torch.randint(0, W.shape[0], (n_draw,), generator=g)
            k = torch.randint(0, W.shape[1], (n_draw,), generator=g)
            ok = (L[m, k] != 0) & (W[n, k] != 0)
            if fed is not None:
                ok &= ref[fed][m, n] > 0
            idx = ok.nonzero().flatten()
            # one probe per row of the batch: the perturbed reference runs on the probes' rows, a product out of each
            _, first = np.unique(m[idx].numpy(), return_index=True)
            idx = idx[torch.from_numpy(np.sort(first))][:FFN_PROBES]
            assert idx.numel() == FFN_PROBES, f'{name}: only {idx.numel()} probes'
            m, n, k = m[idx], n[idx], k[idx]
            pert = R.ffn_direct_ref(case, d, dtype, rows=m, drop=(name, torch.arange(m.numel()), n, k))
            changed = torch.zeros(m.numel(), dtype=torch.bool)
            for key, v in R.ffn_direct_outputs(case, pert).items():
                changed |= (R.rnd(v, dtype) != base[key][m]).any(1)
            assert changed.all(), f'{name} {dtype}: {int((~changed).sum())} of {m.numel()} dropped products do not show'


def _ffn_f32_composition(case, d, dtype, ln, rows):
    """The entry point as a composition of torch's own f32 operators, the 16-bit roundings where the kernel has them."""
    kind = case[0]
    f = lambda k: d[k][rows] if d[k].shape[0] == case[4] and k not in ('W1', 'W2', 'Wo', 'W3', 'Wds') else d[k]
    if kind in ('ffn', 'attn_out_ffn'):
        if kind == 'ffn':
            x = f('x')
        else:
            x = F.layer_norm(f('R') + F.linear(f('A'), d['Wo'], d['bo']), (case[1],), d['g1'], d['be1'], d['eps1']).to(dtype).float()
        h = F.relu(F.linear(x, d['W1'], d['b1'])).to(dtype).float()
        y = x + F.linear(h, d['W2'], d['b2'])
        return {'y': F.layer_norm(y, (case[1],), d['ln'][0], d['ln'][1], d['ln'][2]) if ln else y}
    w3, w1 = (d['W3'] * d['s3'].view(-1, 1)).to(dtype).float(), (d['W1'] * d['s1'].view(-1, 1)).to(dtype).float()
    if kind == 'pair':
        Y = F.relu(F.linear(f('X'), w3, d['b3']) + f('R'))
    else:
        Y = F.relu(F.linear(f('X'), w3) + F.linear(f('X0'), (d['Wds'] * d['sds'].view(-1, 1)).to(dtype).float()) + d['b3'])
    return {'Y': Y, 'T': F.relu(F.linear(Y.to(dtype).float(), w1, d['b1']))}


_FFN_YARD = [c for c in R.FFN_DIRECT_CASES if c[4] != R.FFN_BIG_ROWS and c[2] in (160, 2048, 256, 512) and c[5] in (0, 128)]


@pytest.mark.parametrize('dtype', _FFN_DT, ids=str)
@pytest.mark.parametrize('case', _FFN_YARD, ids=R.ffn_case_id)
def test_ffn_refs_against_an_f32_torch_composition(case, dtype):
    """The four references against torch's own f32 operators on the generic class (its first 96 rows): within the
    generic bound, LayerNorm off and (kinet_ffn_fused) on -- and in the exact class, equal."""
    rows = slice(0, 96)
    d = R.ffn_direct_inputs(case, 'generic', dtype)
    # (the attention entry's worst-case bound, three 16-bit roundings deep, is too wide to carry through a LayerNorm)
    for ln in ((False, True) if case[0] == 'ffn' else (False,)):
        ref = R.ffn_direct_ref(case, d, dtype, ln=ln, rows=rows)
        tol = R.ffn_direct_generic_tol(case, d, ref, dtype, ln)
        got = _ffn_f32_composition(case, d, dtype, ln, rows)
        for name, want in R.ffn_direct_outputs(case, ref).items():
            ratio = float(((got[name].to(dtype).double() - want).abs() / tol[name]).max())
            assert ratio <= 1.0, (name, ln, ratio)
    d = R.ffn_direct_inputs(case, 'exact')
    ref = R.ffn_direct_ref(case, d, dtype, rows=rows)
    got = _ffn_f32_composition(case, d, dtype, False, rows)
    for name, want in R.ffn_direct_outputs(case, ref).items():
        assert torch.equal(got[name].double(), want), name


# ------------------------------------------------------- attention forward, kernel by kernel
_ATTN_DT = [torch.bfloat16, torch.float16, torch.float32]
_KT = R.ATTN_KT


def _attn_exact_model(case, dtype):
    """The f64 block model of the kernels on an exact-class case, as the output type's bits."""
    return R.attn_bits(R.attn_blockwise(case).to(dtype))


def _attn_scores(case):
    """(scores of the case's actual q and k in f64, the same in f32 arithmetic) -- scale 1."""
    H = case['heads']
    q, k = R._attn_split(case['q'], H), R._attn_split(case['k'], H)
    return q.double() @ k.double().transpose(-1, -2), q.float() @ k.float().transpose(-1, -2)


@pytest.mark.parametrize('dtype', _ATTN_DT, ids=str)
@pytest.mark.parametrize('D', [16, 32, 36, 64])
def test_attn_select_cases_gap_and_expected(D, dtype):
    """Every selection case the GPU test runs: q and k hold exactly 64 code and code, every score is an f32-exact
    integer, the selected key leads every other live key by >= 128, the expected row is v[sel], and the block
    model of the kernels reproduces it bit for bit."""
    shapes = R.attn_shapes('fma', D)
    if D in R.ATTN_RESIDENT_MAXK and dtype != torch.float32:
        shapes = list(dict.fromkeys(shapes + R.attn_shapes('resident', D) + R.attn_shapes('stream', D)))
    for Lq, Lk in shapes:
        modes = ('pairs', 'edges', 'last') if (Lq, Lk) == R.ATTN_MAIN else ('pairs',)
        for mode in modes:
            c = R.attn_select_case(D, Lq, Lk, dtype, mode)
            S64, S32 = _attn_scores(c)
            assert torch.equal(S64, c['scores'].double()) and torch.equal(S32.double(), S64)
            assert S64.abs().max() <= 64 * D and torch.equal(S64, S64.round())
            live = ~c['mask'][:, None, None, :]
            sel_s = torch.gather(S64, 3, c['sel'][..., None])
            others = S64.masked_fill(~live.expand_as(S64), float('-inf')).scatter(3, c['sel'][..., None], float('-inf'))
            alive = ~c['mask'].all(1)
            if Lk > 1:
                assert (sel_s - others.amax(-1, keepdim=True))[alive].min() >= 128
            assert not torch.gather(c['mask'][:, None, :].expand(-1, c['heads'], -1), 2, c['sel'])[alive].any()
            v = R._attn_split(c['v'], c['heads'])
            want = torch.gather(v, 2, c['sel'][..., None].expand(-1, -1, -1, D))
            want[~alive] = 0
            assert torch.equal(R.attn_bits(R._attn_merge(want)), R.attn_bits(c['expected']))
            assert torch.isfinite(c['v'].double()).all()
            assert torch.equal(_attn_exact_model(c, dtype), R.attn_bits(c['expected'])), (Lq, Lk, mode)
            # a masked key holds the largest finite values: a leak shows
            vm = v.double().abs()[c['mask'][:, None, :, None].expand_as(v)]
            assert (vm == torch.finfo(dtype).max).all()
            # the case differs per batch, head and query
            assert not torch.equal(c['q'][0], c['q'][1]) or Lk == 1
            if Lq > 1 and Lk > 2 and mode == 'pairs':
                e = R._attn_split(c['expected'], c['heads'])
                assert not torch.equal(e[0, 0], e[0, 1]) and not torch.equal(e[0, 0, 0], e[0, 0, 1])


@pytest.mark.parametrize('Lk', [2 * _KT + 5, 3 * _KT])
@pytest.mark.parametrize('D', [32, 36])
def test_attn_select_cases_cover_slots_dims_and_order(D, Lk):
    """The builder's guarantees on the three-tile cases: every slot of the first block, of the last block of the
    second tile and of the last (ragged) block is selected -- one block in each tile of the streaming kernel; for
    every head dim a live pair differing in that dim only, each member selected by some query (so the selected key
    sits blocks before its runner-up for one query and blocks after it for another); masked-best-match queries."""
    c = R.attn_select_case(D, 129, Lk, torch.bfloat16, 'pairs')
    lo, hi, mid = R.attn_pair_keys(D, Lk)
    nblk = (Lk + 31) // 32
    assert mid == 2 * _KT // 32 - 1 and len(lo) == D and nblk - 1 >= 2 * _KT // 32
    chosen = set(c['sel'].flatten().tolist())
    for blk in (0, mid, nblk - 1):
        assert set(range(blk * 32, min(blk * 32 + 32, Lk))) <= chosen, blk
    assert 0 // _KT == 0 and (mid * 32) // _KT == 1 and ((nblk - 1) * 32) // _KT == 2
    codes, mask, sel = c['codes'], c['mask'], c['sel']
    before = after = best_match = 0
    for d in range(D):
        diff = (codes[:, :, lo[d]] != codes[:, :, hi[d]])
        assert diff[..., d].all() and diff.sum(-1).eq(1).all()
        assert hi[d] // 32 > lo[d] // 32 + 1
        ok = False
        for b in range(R.ATTN_B):
            if not mask[b, lo[d]] and not mask[b, hi[d]]:
                s = set(sel[b].flatten().tolist())
                ok |= lo[d] in s and hi[d] in s
                before += lo[d] in s          # selected before the runner-up's block: the max stays
                after += hi[d] in s           # selected after it: the max rises, O is rescaled to 0
        assert ok, d
    for b in range(R.ATTN_B):
        t_masked = torch.gather(mask[b][None, :].expand(c['heads'], -1), 1, c['target'][b])
        partner = {**dict(zip(lo, hi)), **dict(zip(hi, lo))}
        for h, i in t_masked.nonzero().tolist():
            assert int(sel[b, h, i]) == partner[int(c['target'][b, h, i])]
            best_match += 1
    assert before >= D // 2 and after >= D // 2 and best_match >= 8
    assert mask[0].any() and mask[1].any() and not torch.equal(mask[0], mask[1])


@pytest.mark.parametrize('dtype', _ATTN_DT, ids=str)
@pytest.mark.parametrize('D', [16, 32, 36, 64])
def test_attn_tie_case_means_are_exact(D, dtype):
    c = R.attn_tie_case(D, 129, dtype)
    groups = R.attn_tie_groups()
    assert {len(ks) for ks in groups.values()} == {2, 4, 8, 16, 32, 64}
    lane = lambda j: (j % 32 % 16) // 4                                   # noqa: E731
    assert len({lane(j) for j in groups['lane8']}) == 1 and len({j // 32 for j in groups['lane8']}) == 1
    assert {lane(j) for j in groups['groups4']} == {0, 1, 2, 3} == {lane(j) for j in groups['groups16']}
    for n in ('consec64', 'consec2'):
        blocks = sorted({j // 32 for j in groups[n]})
        assert blocks == [blocks[0], blocks[0] + 1] and blocks[0] // (_KT // 32) == blocks[1] // (_KT // 32)
    assert {j // _KT for j in groups['edge4']} == {0, 1}
    assert {j // _KT for j in groups['tiles02_2']} == {0, 2} == {j // _KT for j in groups['tiles02_8']}
    assert groups['groups4'][0] // 32 == _KT // 32 - 1 and groups['groups16'][0] // 32 == 2 * _KT // 32 - 1
    assert set(c['group'].flatten().tolist()) == set(range(len(groups)))
    S64, S32 = _attn_scores(c)
    assert torch.equal(S64, c['scores'].double()) and torch.equal(S32.double(), S64)
    # the f32 sum of a group's values is exact and the mean is a value of the output type
    v = R._attn_split(c['v'], c['heads'])
    s32 = c['tied'].float() @ v.float().masked_fill(c['mask'][:, None, :, None], 0)
    assert torch.equal(s32.double(), c['tied'].double() @ v.double().masked_fill(c['mask'][:, None, :, None], 0))
    assert torch.equal(c['expected'].double(), c['mean64'])
    assert c['mask'][:, R.ATTN_TIE_DECOY[0]].all() and not c['tied'][..., R.ATTN_TIE_DECOY[0]].any()
    assert torch.equal(_attn_exact_model(c, dtype), R.attn_bits(c['expected']))


@pytest.mark.parametrize('variant', R.ATTN_VARIANTS)
@pytest.mark.parametrize('D', [32, 36])
def test_attn_blockwise_is_the_reference(D, variant):
    for maskmode in ('random', 'first_tile', 'dead_batch'):
        c = R.attn_generic_case(D, 65, 2 * _KT + 5, torch.bfloat16, variant, maskmode)
        assert (R.attn_blockwise(c) - c['o']).abs().max() <= 1e-12 * max(1.0, c['o'].abs().max().item())


def _attn_generic_cases(dtype, D):
    yield 'plain', R.attn_generic_case(D, 65, 2 * _KT + 5, dtype, 'plain', 'random')
    yield 'wide', R.attn_generic_case(D, 65, 2 * _KT + 5, dtype, 'wide', 'random')
    yield 'offset', R.attn_generic_case(D, 65, 2 * _KT + 5, dtype, 'offset', 'random')


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize('D', [32, 36])
def test_attn_bound_admits_the_kernel_model_and_f32_sdpa(D, dtype):
    """The f64 block model with p rounded to the 16-bit type (the MFMA kernels' one deliberate deviation) and torch's
    f32 SDPA, both rounded to the output type, are inside the bound; the scores of 'wide' reach +-60 and those of
    'offset' sit near 200."""
    for name, c in _attn_generic_cases(dtype, D):
        bound = R.attn_fwd_bound(c, 'resident', dtype)
        for got in (R.attn_blockwise(c, pround=dtype), c['sdpa']):
            worst, share, zeros = R.attn_ratio(got.to(dtype).double(), c, bound)
            assert worst < 1.0 and zeros and share > 0.99, (name, worst, share)
        S = (R._attn_split(c['q'].double(), 3) @ R._attn_split(c['k'].double(), 3).transpose(-1, -2)) * c['scale']
        if name == 'wide':
            assert S.max() > 60 and S.min() < -60
        if name == 'offset':
            assert S.min() > 150
    sub = R.attn_subnormal_case(D, dtype)
    bound = R.attn_fwd_bound(sub, 'resident', dtype)
    kept = R.attn_blockwise(sub, pround=dtype).to(dtype).double()
    assert R.attn_ratio(kept, sub, bound)[0] < 1.0
    if dtype == torch.float16:
        flushed = torch.full_like(kept, 1.0 / (1.0 + 256 * 2.0 ** -16)).to(dtype).double()
        assert R.attn_ratio(flushed, sub, bound)[0] > 1.0          # the case tells the two models apart


@pytest.mark.parametrize('mut', R.ATTN_MUTATIONS)
@pytest.mark.parametrize('D', [32, 36])
def test_attn_mutations_are_caught(D, mut):
    """Each way the block step could be broken, applied to the model: class 1 and class 2 must see a wrong bit,
    class 3 an element over the bound.  'l_rounded' is the exception.  It changes l by at most u16 relative, and only
    where p is neither 0 nor 1: the exact classes have p in {0, 1} and cannot see it, and on N(0, 1) operands it moves
    the output by at most u16 |o|, inside terms (a) + (b) -- the bound is too wide for it there.  The class-3 case
    built for it, R.attn_bias_case, catches it (the model of the kernels as they are stays inside)."""
    dt = torch.bfloat16
    c1 = R.attn_select_case(D, *R.ATTN_MAIN, dt, 'pairs')
    c2 = R.attn_tie_case(D, 129, dt)
    caught = {}
    for name, c in (('select', c1), ('tie', c2)):
        arg = R.attn_mutation_arg(mut, c)
        if arg is not None:
            got = R.attn_blockwise(c, mut, arg, pround=dt).to(dt)
            caught[name] = not torch.equal(R.attn_bits(got), R.attn_bits(c['expected']))
    worst = 0.0
    for dtype in (torch.bfloat16, torch.float16):
        for name, c in _attn_generic_cases(dtype, D):
            arg = R.attn_mutation_arg(mut, c)
            if arg is not None:
                got = R.attn_blockwise(c, mut, arg, pround=dtype).to(dtype).double()
                worst = max(worst, R.attn_ratio(got, c, _attn_bound(D, dtype, name))[0])
                caught['generic'] = worst > 1.0
    if mut == 'l_rounded':
        assert caught == {'select': False, 'tie': False, 'generic': False}, (caught, worst)
        for dtype in (torch.bfloat16, torch.float16):
            c = R.attn_bias_case(D, dtype)
            bound = R.attn_fwd_bound(c, 'resident', dtype)
            as_is, broken, sdpa = (R.attn_ratio(o.to(dtype).double(), c, bound)[0] for o in
                                   (R.attn_blockwise(c, pround=dtype), R.attn_blockwise(c, mut, True, pround=dtype), c['sdpa']))
            assert as_is < 1.0 < broken and sdpa < 1.0, (as_is, broken, sdpa)
    elif mut == 'drop_dim35' and D == 32:
        assert caught == {}
    else:
        # a lost head dim ties no two keys of the tie case, which has no pair by design: class 1's pairs catch it
        assert caught == {'select': True, 'tie': not mut.startswith('drop_dim'), 'generic': True}, (caught, worst)


@functools.lru_cache(maxsize=None)
def _attn_bound(D, dtype, name):
    return R.attn_fwd_bound(dict(_attn_generic_cases(dtype, D))[name], 'resident', dtype)


# ------------------------------------- the stem and direct 3x3 kernels (test_stem_conv3x3_direct_gpu.py)
_FRONT_DT = [torch.bfloat16, torch.float16]


def _front_nhwc(kind, x):
    return x if kind == 'c3' else x.permute(0, 2, 3, 1)


def _front_f32(kind, c, scale_bias=True, relu=True, x=None):
    """torch's own f32 convolution and f32 epilogue of a case's operands -> (B*Ho*Wo, 64) f32."""
    k, stride, pad, Cin, K = R.FRONT_GEO[kind]
    x = c['x'] if x is None else x
    y = F.conv2d(x.permute(0, 3, 1, 2) if kind == 'c3' else x, c['w'], stride=stride, padding=pad)
    y = y.permute(0, 2, 3, 1).reshape(-1, 64)
    if scale_bias:
        y = y * c['scale'] + c['bias']
    return torch.relu(y) if relu else y


def test_front_tables_reach_the_paths_they_name():
    """The geometry behind the tables' comments: tiles, strips, persistent walks."""
    def tiles(shape, th, tw, stem):
        B, H, W = shape
        Ho, Wo = R.stem_out(H, W) if stem else (H, W)
        return B, -(-Ho // th), -(-Wo // tw)
    assert [tiles(s, 8, 32, False) for s in R.C3_SHAPES] == [(1, 1, 1), (1, 1, 1), (1, 1, 1), (1, 2, 2), (1, 1, 1), (3, 3, 3)]
    for cus in (256, 304, 64):
        B, ty, tx = tiles(R.c3_persistent_shape(cus), 8, 32, False)
        assert (ty, tx) == (3, 3) and 2 * cus < B * 9 <= 2 * cus + 9
    assert [tiles(s, 4, 64, True) for s in R.STEM_SHAPES] == [(1, 1, 1), (1, 2, 1), (1, 1, 1), (1, 2, 2), (2, 1, 2), (1, 2, 1),
                                                              (1, 2, 1)]
    assert R.stem_out(8, 128) == (4, 64) and R.stem_out(16, 126) == R.stem_out(15, 125) == (8, 63)
    B, ty, tx = tiles(R.STEM_PERSISTENT, 4, 64, True)
    assert B * ty * tx > 2 * 512
    Ho, Wo = R.stem_out(*R.STEM_PERSISTENT[1:])
    assert B * -(-((Wo - 1) // 2 + 1) // 31) * -(-Ho // 4) > 2 * 512              # pooled, at seg_tiles = 1
    geo = {(R.stem_out(H, W)[0], (R.stem_out(H, W)[1] - 1) // 2 + 1) for _, H, W in R.POOL_SHAPES}
    assert {h for h, _ in geo} == {4, 5, 8, 9} and {w for _, w in geo} == {31, 32, 63, 75}
    assert {R.stem_out(H, W)[1] for _, H, W in R.POOL_SHAPES} == {61, 62, 63, 64, 125, 150}
    assert {b for b, _, _ in R.POOL_SHAPES} == {1, 2}


@pytest.mark.parametrize('kind,shape,variant', R.front_exact_cases(), ids=str)
def test_front_exact_cases_are_exact_with_headroom(kind, shape, variant):
    """Every exact-class case of the GPU module: operands on the class's grids and representable in both
    16-bit types; the tap-sum reference equals F.conv2d in f64; torch's f32 convolution and f32 epilogue
    equal the f64 result (the class is order-free); a 16-bit output resolves one dropped product on
    every element, under every epilogue the module runs."""
    c = R.front_case(kind, shape, 'exact', None, variant)
    k, stride, pad, Cin, K = R.FRONT_GEO[kind]
    x, w = c['x'], c['w']
    assert ((x * 2) == (x * 2).round()).all() and x.abs().max() <= 1
    assert ((w * 8) == (w * 8).round()).all() and w.abs().max() <= 0.25 and w.shape == (64, Cin, k, k)
    assert (w != 0).float().mean() > 0.15 or variant == 'zero'
    for dt in _FRONT_DT:
        assert (x.to(dt).float() == x).all() and (w.to(dt).float() == w).all()
    assert torch.equal(c['acc'], R.conv64(_front_nhwc(kind, x), w.permute(0, 2, 3, 1), stride, pad))
    assert c['acc'].shape == (c['B'] * c['Ho'] * c['Wo'], 64)
    for sb, relu in (R.C3_EPILOGUES.values() if kind == 'c3' else [(True, True)]):
        pre, _, s = R.front_expected(c, sb, relu)
        assert torch.equal(_front_f32(kind, c, sb, relu).double(), pre)
        if not relu:
            assert (pre < 0).any()
        for dt in _FRONT_DT:
            assert R.exact_headroom(pre, s, dt).all(), (sb, relu, dt, pre.abs().max().item())


@pytest.mark.parametrize('fault', R.FRONT_FAULTS)
@pytest.mark.parametrize('kind', ['c3', 'stem'])
def test_front_exact_inputs_discriminate(kind, fault):
    """The smallest multi-tile exact case (with a batch for the row leaking from image b - 1) recomputed with
    one fault differs from the true reference -- in the accumulator, in the rounded 16-bit output and, for
    the stem, in the pooled map."""
    multi, batch = {'c3': (R.C3_MULTI_TILE, R.C3_SHAPES[-1]), 'stem': (R.STEM_MULTI_TILE, (2, 7, 130))}[kind]
    c = R.front_case(kind, batch if fault == 'prev_image_row' else multi, 'exact')
    k, stride, pad, Cin, K = R.FRONT_GEO[kind]
    xn, wn = _front_nhwc(kind, c['x']), c['w'].permute(0, 2, 3, 1)
    assert torch.equal(R.conv_taps64(xn, wn, stride, pad), c['acc'])
    bad = R.conv_taps64(xn, wn, stride, pad, fault)
    assert (bad != c['acc']).any()
    pre = R.front_expected(c)[0]
    pre_bad = R.epilogue64(bad, c['scale'], c['bias'], None, True)[0]
    for dt in _FRONT_DT:
        assert (pre_bad.to(dt) != pre.to(dt)).any()
        if kind == 'stem':
            geo = (c['B'], c['Ho'], c['Wo'])
            assert (R.pool_rows(pre_bad.to(dt), *geo) != R.pool_rows(pre.to(dt), *geo)).any()


def _truncate(x, dtype):
    """f32 -> dtype rounded towards zero (what a kernel that drops the low bits would feed the MFMAs)."""
    if dtype == torch.bfloat16:
        return (x.view(torch.int32) & -65536).view(torch.float32)
    h = x.half()
    over = h.float().abs() > x.abs()
    return torch.where(over, (h.view(torch.int16) - 1).view(torch.float16), h).float()


@pytest.mark.parametrize('dtype', _FRONT_DT, ids=str)
@pytest.mark.parametrize('kind,shape', [('c3', R.C3_MULTI_TILE), ('stem', R.STEM_MULTI_TILE), ('stem', R.POOL_BIAS1_SHAPE)], ids=str)
def test_front_generic_bound_holds_for_torch_f32_and_rejects_defects(kind, shape, dtype):
    """torch's f32 convolution of the rounded operands + f32 epilogue + one output rounding stays inside the
    generic bound, and its pooled map inside the pooled bound; one dropped tap leaves it, and so does (stem)
    an image truncated to the 16-bit type instead of rounded to nearest."""
    c = R.front_case(kind, shape, 'generic', dtype)
    k, stride, pad, Cin, K = R.FRONT_GEO[kind]
    xr = c['x'].to(dtype).float()
    assert (c['w'].to(dtype).float() == c['w']).all()
    assert (xr != c['x']).any() == (kind == 'stem')
    pre, maj, s = R.front_expected(c)
    bound = R.gemm_generic_bound(c['absprod'], K, maj, pre, dtype, s)
    geo = (c['B'], c['Ho'], c['Wo'])
    good = _front_f32(kind, c, x=xr).to(dtype).double()
    err = (good - pre).abs()
    print(f'{kind} {shape} {dtype}: torch f32 worst err / bound {(err / bound).max().item():.3f}')
    assert (err <= bound).all()
    dropped = R.epilogue64(R.conv_taps64(_front_nhwc(kind, xr), c['w'].permute(0, 2, 3, 1), stride, pad, 'drop_tap'),
                           c['scale'], c['bias'], None, True)[0].to(dtype).double()
    # (ReLU clears half of the map, and at the bottom rows the dropped tap lies in the padding)
    assert ((dropped - pre).abs() > bound).float().mean() > 0.1
    if kind == 'stem':
        pooled, pbound = R.pool_rows(pre, *geo), R.pool_rows(bound, *geo)
        assert ((R.pool_rows(good, *geo) - pooled).abs() <= pbound).all()
        assert ((R.pool_rows(dropped, *geo) - pooled).abs() > pbound).float().mean() > 0.1
        xt = _truncate(c['x'], dtype)
        assert (xt.abs() <= c['x'].abs()).all() and (xt.to(dtype).float() == xt).all() and (xt != xr).any()
        trunc = _front_f32(kind, c, x=xt).to(dtype).double()
        share = ((trunc - pre).abs() > bound).float().mean().item()
        pshare = ((R.pool_rows(trunc, *geo) - pooled).abs() > pbound).float().mean().item()
        print(f'truncated image: {share:.3f} of the conv map and {pshare:.3f} of the pooled map outside the bound')
        assert share > 0.01 and pshare > 0.01


@pytest.mark.parametrize('dtype', _FRONT_DT, ids=str)
def test_pool_border_case_tells_parked_padding_from_computed_padding(dtype):
    """The bias = 1 case: the signed 16-bit maximum over post-ReLU patterns, with the taps outside the conv map
    parked as -0.0 (0x8000, the smallest int16), is torch's max_pool2d; were those taps computed from the
    zero-padded image instead (relu(bias) = 1), the last pooled row and column would change."""
    c = R.front_case('stem', R.POOL_BIAS1_SHAPE, 'exact', None, 'bias1')
    B, Ho, Wo = c['B'], c['Ho'], c['Wo']
    conv = R.front_expected(c)[0].to(dtype)
    want = R.pool_rows(conv, B, Ho, Wo).view(B, (Ho - 1) // 2 + 1, (Wo - 1) // 2 + 1, 64)
    bits = conv.view(torch.int16).double().view(B, Ho, Wo, 64).permute(0, 3, 1, 2)
    assert (bits >= 0).all()                                       # post-ReLU: the sign bit is clear
    parked = F.max_pool2d(F.pad(bits, (1, 1, 1, 1), value=-32768.0), 3, 2, 0).permute(0, 2, 3, 1)
    assert torch.equal(parked.to(torch.int16).view(dtype), want)
    ones = F.max_pool2d(F.pad(conv.double().view(B, Ho, Wo, 64).permute(0, 3, 1, 2), (1, 1, 1, 1), value=1.0), 3, 2, 0)
    differ = ones.permute(0, 2, 3, 1) != want.double()
    assert Ho % 2 == 1 and Wo % 2 == 1                             # the last pooled row and column reach past the map
    assert differ[:, -1].any() and differ[:, :, -1].any()


def test_pool_zero_case_is_all_positive_zero():
    c = R.front_case('stem', R.POOL_ZERO_SHAPE, 'exact', None, 'zero')
    assert (c['w'] == 0).all() and (c['bias'] == 0).all() and (c['x'] != 0).any()
    assert (R.front_expected(c)[0] == 0).all()
