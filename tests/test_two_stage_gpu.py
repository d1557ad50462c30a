"""Two-stage Deformable DETR on the GPU: the kernels of csrc/two_stage.hip against references
written here, and the model against the reference model's outputs
(tests/golden/make_golden_two_stage.py; same name-seeded weights, frames regenerated from CPU
generator seeds: 3x256x448 and 3x224x320 in one NestedTensor, level shapes 32x56, 16x28, 8x14,
4x7, S = 2380, 100 proposals).

  A  with_box_refine: true      B  with_box_refine: false

Selection is discontinuous, so the model checks are split: the selected SET equals the
reference's (the fixture's weight seed keeps >= 4e-3 between the k-th and (k+1)-th reference
score, 4x the fp32 gate), the selected ORDER is exactly the stable descending sort of the
model's own scores, and per-query outputs are compared after matching queries by proposal
index (inside the set the reference's adjacent gaps go down to 1e-6, so its order is not
reproducible within the gate).
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-3
FRAMES = ((2101, 256, 448), (2102, 224, 320))
SHAPES = [(32, 56), (16, 28), (8, 14), (4, 7)]
K_PROP = 100
# 16-bit compute vs the fp32 HIP run: the deformable path's existing per-tensor bounds
# (tests/test_fullsize_gpu.py BF16_TOL / F16_TOL)
TOL16 = {torch.bfloat16: {'pred_logits': 0.3, 'pred_boxes': 0.03, 'hs_embed': 0.45},
         torch.float16: {'pred_logits': 0.08, 'pred_boxes': 0.01, 'hs_embed': 0.13}}
# Share of the fp32 run's 100 proposals that the 16-bit run also selects, per frame.  Measured on
# MI355X (profiles/two_stage_tolerances.log): bf16 0.99 / 0.99, f16 1.00 / 1.00.  The floor
# leaves a margin of 5 proposals of 100 below the smallest measured share of each dtype: a
# 16-bit score error moves proposals across the cut one at a time, and a handful more than
# measured is rounding, while a drop of tens means the scores no longer rank alike.
COMMON_FLOOR = {torch.bfloat16: 0.94, torch.float16: 0.95}


# --------------------------------------------------------------------------------------
# proposals kernel
# --------------------------------------------------------------------------------------
def _ref_proposals(shapes, mask):
    """deformable_transformer.py:92-116 restated (CPU, f32 as the reference; the logit also in
    f64 from the same f32 proposals).  mask (B, S) bool."""
    N = mask.shape[0]
    proposals, cur = [], 0
    for lvl, (H, W) in enumerate(shapes):
        m = mask[:, cur:cur + H * W].view(N, H, W, 1)
        valid_H = torch.sum(~m[:, :, 0, 0], 1)
        valid_W = torch.sum(~m[:, 0, :, 0], 1)
        gy, gx = torch.meshgrid(torch.linspace(0, H - 1, H, dtype=torch.float32),
                                torch.linspace(0, W - 1, W, dtype=torch.float32), indexing='ij')
        grid = torch.cat([gx.unsqueeze(-1), gy.unsqueeze(-1)], -1)
        scale = torch.cat([valid_W.unsqueeze(-1), valid_H.unsqueeze(-1)], 1).view(N, 1, 1, 2)
        grid = (grid.unsqueeze(0).expand(N, -1, -1, -1) + 0.5) / scale
        wh = torch.ones_like(grid) * 0.05 * (2.0 ** lvl)
        proposals.append(torch.cat((grid, wh), -1).view(N, -1, 4))
        cur += H * W
    p = torch.cat(proposals, 1)
    assert p.dtype == torch.float32
    valid = ((p > 0.01) & (p < 0.99)).all(-1, keepdim=True)
    keep = valid & ~mask.unsqueeze(-1)
    inf = float('inf')
    out32 = torch.log(p / (1 - p)).masked_fill(~keep, inf)
    out64 = torch.log(p.double() / (1 - p.double())).masked_fill(~keep, inf)
    return out32, out64, keep.squeeze(-1)


def _fixture_mask():
    from kinet_amd.models.backbone import interp_mask
    m = torch.ones(2, 256, 448, dtype=torch.bool)
    for b, (_, h, w) in enumerate(FRAMES):
        m[b, :h, :w] = False
    return torch.cat([interp_mask(m.cuda(), s).flatten(1) for s in SHAPES], 1).cpu()


def _check_proposals(shapes, mask, pass_mask=True):
    from kinet_amd import kernels as K
    S = sum(h * w for h, w in shapes)
    B = mask.shape[0]
    prop, keep = K.two_stage_proposals(shapes, mask.cuda() if pass_mask else None, B, torch.device('cuda'))
    torch.cuda.synchronize()
    prop, keep = prop.cpu(), keep.cpu()
    r32, r64, rkeep = _ref_proposals(shapes, mask)
    assert prop.shape == (B, S, 4) and keep.shape == (B, S)
    assert not torch.isnan(prop).any()
    assert torch.equal(keep.bool(), rkeep)
    assert torch.equal(torch.isinf(prop), torch.isinf(r32))
    assert (prop[torch.isinf(prop)] > 0).all()
    fin = torch.isfinite(prop)
    e64 = (prop[fin].double() - r64[fin]).abs().max().item()
    e32 = (prop[fin] - r32[fin]).abs().max().item()
    print(f'[two_stage] proposals {shapes}: kept {int(keep.sum())}/{keep.numel()} max err vs f64 {e64:.3g} vs f32 {e32:.3g}')
    assert e64 <= 1e-6 and e32 <= 1e-6
    return keep


def test_proposals_fixture_geometry_padded():
    keep = _check_proposals(SHAPES, _fixture_mask())
    assert (keep == 0).sum(1).tolist() == [64, 890]     # the reference run's invalid tokens


def test_proposals_fixture_geometry_unpadded():
    mask = torch.zeros(2, 2380, dtype=torch.bool)
    _check_proposals(SHAPES, mask)
    _check_proposals(SHAPES, mask, pass_mask=False)


def test_proposals_threshold_widths():
    """(j + 0.5) / 50 hits 0.01f and 0.99f exactly (both invalid: the compares are strict);
    width 100 puts 0.005 / 0.015 and 0.985 / 0.995 around them; also 50 valid of 64 padded
    columns, and levels whose w / h proposal leaves (0.01, 0.99) (0.05 * 2^5 = 1.6)."""
    shapes = [(4, 100), (3, 50)]
    keep = _check_proposals(shapes, torch.zeros(3, 550, dtype=torch.bool), pass_mask=False)
    k0, k1 = keep[0, :400].view(4, 100), keep[0, 400:].view(3, 50)
    assert k0[:, 1:99].all() and not k0[:, 0].any() and not k0[:, 99].any()
    assert k1[:, 1:49].all() and not k1[:, 0].any() and not k1[:, 49].any()
    m = torch.zeros(2, 5, 64, dtype=torch.bool)
    m[:, :, 50:] = True
    m[1, 3:] = True
    keep = _check_proposals([(5, 64)], m.flatten(1))
    assert keep[0].view(5, 64)[:, 1:49].all() and not keep[0].view(5, 64)[:, 49:].any()
    shapes = [(3, 5), (3, 5), (3, 5), (3, 5), (3, 5), (3, 5)]
    keep = _check_proposals(shapes, torch.zeros(1, 90, dtype=torch.bool))
    assert keep[0, :60].any() and not keep[0, 75:].any()


# --------------------------------------------------------------------------------------
# top-k kernel
# --------------------------------------------------------------------------------------
def _check_topk(x, k):
    from kinet_amd import kernels as K
    got = K.topk_rows(x, k)
    torch.cuda.synchronize()
    want = torch.sort(x.cpu(), dim=1, descending=True, stable=True)[1][:, :k]
    assert got.dtype == torch.int64 and got.shape == (x.shape[0], k)
    assert torch.equal(got.cpu(), want)


def _randn(rows, S, seed):
    return torch.randn(rows, S, generator=torch.Generator().manual_seed(seed)).cuda()


# 36 000 is the longest row whose keys the kernel keeps in LDS (csrc/two_stage.hip TK_CACHE): longer
# rows re-read global memory
@pytest.mark.parametrize('S,k', [(2380, 100), (22223, 300), (22223, 1024), (257, 257), (1, 1), (1025, 1024),
                                 (36000, 300), (36001, 300), ((1 << 17) + 3, 64), ((1 << 17) + 3, 1024)])
def test_topk_random(S, k):
    _check_topk(_randn(3, S, S + k), k)


def test_topk_strided_channel_zero():
    x = torch.randn(2, 2380, 20, generator=torch.Generator().manual_seed(5)).cuda()
    _check_topk(x[..., 0], 100)
    _check_topk(x[..., 7], 300)


def test_topk_ties():
    g = torch.Generator().manual_seed(6)
    # 900 equal values straddling the cut: 50 above, 900 equal, the rest below, shuffled
    x = torch.cat([torch.rand(50, generator=g) + 5, torch.full((900,), 1.0), torch.rand(1430, generator=g) - 3])
    x = torch.stack([x[torch.randperm(2380, generator=g)] for _ in range(3)]).cuda()
    _check_topk(x, 100)
    _check_topk(x, 949)
    _check_topk(x, 950)
    _check_topk(x, 951)
    # all-equal rows
    _check_topk(torch.zeros(2, 2380).cuda(), 100)
    _check_topk(torch.full((2, 22223), -7.5).cuda(), 1024)
    # many ties everywhere: two-decimal values (the second row length re-reads global memory)
    _check_topk((_randn(2, 22223, 7) * 100).round() / 100, 300)
    _check_topk((_randn(2, 43000, 8) * 100).round() / 100, 1024)


def test_topk_special_values():
    g = torch.Generator().manual_seed(8)
    inf = float('inf')
    x = torch.randn(3, 257, generator=g)
    x[0, [5, 100, 256]] = inf
    x[0, [0, 7, 200]] = -inf
    x[1, 3] = -inf
    x[2, :] = -inf
    x[2, 17] = inf
    _check_topk(x.cuda(), 257)
    _check_topk(x.cuda(), 4)
    # -0.0 and +0.0 are equal: ties by index across both
    z = torch.where(torch.rand(2, 2380, generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
    z[:, ::97] = 1.0
    z[:, 5::89] = -1.0
    _check_topk(z.cuda(), 100)
    _check_topk(z.cuda(), 1024)
    # one NaN: first, as in torch
    y = torch.randn(2, 2380, generator=g)
    y[0, 1234] = float('nan')
    y[1, 0] = float('nan')
    y[1, 2379] = inf
    _check_topk(y.cuda(), 100)
    _check_topk(y.cuda(), 1)


# --------------------------------------------------------------------------------------
# gather + proposal position embedding
# --------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def query_case():
    g = torch.Generator().manual_seed(9)
    B, S, k = 2, 300, 100
    coord = torch.randn(B, S, 4, generator=g) * 2.5
    coord[0, 10] = float('inf')
    coord[1, 20, 2:] = float('inf')
    coord[1, 21, 0] = -float('inf')
    idx = torch.stack([torch.randperm(S, generator=g)[:k] for _ in range(B)])
    idx[0, 3], idx[1, 0], idx[1, 99] = 10, 20, 21
    sg = 1 / (1 + torch.exp(-coord.double()))
    ref = torch.gather(sg, 1, idx.unsqueeze(-1).expand(-1, -1, 4))
    f = torch.arange(128, dtype=torch.float64)
    dim_t = 10000.0 ** (2 * torch.div(f, 2, rounding_mode='floor') / 128)
    arg = ref[..., None] * (2 * math.pi) / dim_t                      # (B, k, 4, 128)
    pos = torch.stack((arg[..., 0::2].sin(), arg[..., 1::2].cos()), dim=4).flatten(2)
    return coord, idx, ref, pos


def test_queries_fp32(query_case):
    from kinet_amd import kernels as K
    coord, idx, ref, pos = query_case
    r, p = K.two_stage_queries(coord.cuda(), idx.cuda(), torch.float32)
    torch.cuda.synchronize()
    assert r.shape == (2, 100, 4) and p.shape == (2, 100, 512) and p.dtype == torch.float32
    er = (r.cpu().double() - ref).abs().max().item()
    ep = (p.cpu().double() - pos).abs().max().item()
    print(f'[two_stage] queries fp32: max err reference_points {er:.3g} embedding {ep:.3g}')
    assert er <= 1e-5 and ep <= 1e-5
    assert (r[0, 3] == 1).all() and (r[1, 0, 2:] == 1).all() and r[1, 99, 0] == 0


@pytest.mark.parametrize('dtype,mant', [(torch.bfloat16, 7), (torch.float16, 10)])
def test_queries_16bit(query_case, dtype, mant):
    from kinet_amd import kernels as K
    coord, idx, _, _ = query_case
    r32, p32 = K.two_stage_queries(coord.cuda(), idx.cuda(), torch.float32)
    r, p = K.two_stage_queries(coord.cuda(), idx.cuda(), dtype)
    torch.cuda.synchronize()
    assert p.dtype == dtype and torch.equal(r, r32)
    # one rounding step of the 16-bit format at the f32 value (f16: its subnormal spacing below 2^-14)
    step = torch.clamp(p32.abs() * 2.0 ** -mant, min=2.0 ** -24 if dtype == torch.float16 else 0.0)
    assert ((p.float() - p32).abs() <= step).all()


def test_fill_rows_and_boxes():
    from kinet_amd import kernels as K
    g = torch.Generator().manual_seed(10)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        y = torch.randn(3, 515, 256, generator=g).to(dt).cuda()
        keep = (torch.rand(3, 515, generator=g) < 0.7).to(torch.uint8).cuda()
        row = torch.randn(256, generator=g).to(dt).cuda()
        want = torch.where(keep.bool().unsqueeze(-1), y, row)
        K.two_stage_fill_rows(y, keep, row)
        assert torch.equal(y, want)
    tmp = torch.randn(2, 515, 4, generator=g).cuda()
    prop = torch.randn(2, 515, 4, generator=g)
    prop[0, 7] = float('inf')
    prop[1, ::5] = float('inf')
    prop = prop.cuda()
    unact, boxes = K.two_stage_boxes(tmp, prop)
    torch.cuda.synchronize()
    assert torch.equal(unact, tmp + prop)
    assert (boxes.double() - torch.sigmoid((tmp + prop).double())).abs().max().item() <= 1e-6
    assert (boxes[0, 7] == 1).all() and (boxes[1, ::5] == 1).all() and not torch.isnan(boxes).any()


# --------------------------------------------------------------------------------------
# model
# --------------------------------------------------------------------------------------
def _build(golden_dir, tag, refine):
    from weights import make_state_dict
    from kinet_amd.models import build_model
    from kinet_amd.models.config import load_args
    d = dict(np.load(os.path.join(golden_dir, f'two_stage_{tag}.npz')))
    shapes = {}
    for ln in open(os.path.join(golden_dir, f'two_stage_{tag}.keys.txt')):
        k, *s = ln.split()
        shapes[k] = [int(x) for x in s]
    model, _, _ = build_model(load_args('train_deformable', two_stage=True, num_queries=K_PROP, with_box_refine=refine))
    model.load_state_dict(make_state_dict(shapes, seed=int(d['seed'])))
    return model.cuda().eval(), d


@pytest.fixture(scope='module')
def frames():
    return [torch.randn(3, h, w, generator=torch.Generator().manual_seed(s)).cuda() for s, h, w in FRAMES]


@pytest.fixture(scope='module')
def case_a(golden_dir):
    return _build(golden_dir, 'a', True)


@pytest.fixture(scope='module')
def case_b(golden_dir):
    return _build(golden_dir, 'b', False)


def _fwd(model, frames, dtype):
    model.set_compute_dtype(dtype)
    try:
        with torch.no_grad():
            out = model(frames)[0]
        topk = model.transformer.topk_proposals.clone()
        torch.cuda.synchronize()
        return out, topk
    finally:
        model.set_compute_dtype(torch.float32)


def _assert_self_order(out, topk):
    """The selection is exactly the stable descending sort of the model's own scores."""
    scores = out['enc_outputs']['pred_logits'][..., 0]
    assert torch.equal(topk, torch.sort(scores, dim=1, descending=True, stable=True)[1][:, :topk.shape[1]])


def _check_fp32(model, d, frames):
    out, topk = _fwd(model, frames, torch.float32)
    enc = out['enc_outputs']
    assert tuple(enc['pred_logits'].shape) == tuple(d['shape_enc_logits']) == (2, 2380, 91)
    assert tuple(enc['pred_boxes'].shape) == (2, 2380, 4)
    assert tuple(out['pred_logits'].shape) == (2, K_PROP, 91) and tuple(out['hs_embed'].shape) == (2, K_PROP, 256)
    assert topk.dtype == torch.int64 and tuple(topk.shape) == (2, K_PROP)
    _assert_self_order(out, topk)
    ref_topk = d['topk']
    for b in range(2):
        assert set(topk[b].tolist()) == set(ref_topk[b].tolist()), f'frame {b}: selected set differs'
    e = np.abs(enc['pred_logits'][..., 0].cpu().numpy() - d['enc_logits0']).max()
    print(f'[two_stage] fp32 enc logits max err {e:.3g}')
    assert e <= TOL
    boxes, ref_boxes = enc['pred_boxes'].cpu().numpy(), d['enc_boxes']
    invalid = (ref_boxes == 1).all(-1)
    assert invalid.sum(1).tolist() == [64, 890]
    assert (boxes[invalid] == 1).all()
    assert np.abs(boxes[~invalid] - ref_boxes[~invalid]).max() <= TOL
    # queries matched to the reference's by proposal index
    errs = {}
    names = [('pred_logits', 'pred_logits'), ('pred_boxes', 'pred_boxes'), ('hs_embed', 'hs_embed')]
    got = {k: out[k].float().cpu().numpy() for k, _ in names}
    assert len(out['aux_outputs']) == 5
    for i, aux in enumerate(out['aux_outputs']):
        got[f'aux{i}_logits'] = aux['pred_logits'].cpu().numpy()
        got[f'aux{i}_boxes'] = aux['pred_boxes'].cpu().numpy()
    for b in range(2):
        where = {int(p): r for r, p in enumerate(ref_topk[b])}
        perm = np.array([where[int(p)] for p in topk[b].tolist()])
        for k, v in got.items():
            errs[k] = max(errs.get(k, 0.0), float(np.abs(v[b] - d[k][b][perm]).max()))
    print('[two_stage] fp32 matched-query max err: ' + ' '.join(f'{k}={v:.3g}' for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= TOL, (k, v)


def test_case_a_fp32_parity(case_a, frames):
    _check_fp32(*case_a, frames)


def test_case_b_fp32_parity(case_b, frames):
    _check_fp32(*case_b, frames)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_case_a_16bit_vs_fp32(case_a, frames, dtype):
    model, _ = case_a
    ref, ref_topk = _fwd(model, frames, torch.float32)
    out, topk = _fwd(model, frames, dtype)
    _assert_self_order(out, topk)
    tol = TOL16[dtype]
    el = (out['enc_outputs']['pred_logits'] - ref['enc_outputs']['pred_logits']).abs().max().item()
    eb = (out['enc_outputs']['pred_boxes'] - ref['enc_outputs']['pred_boxes']).abs().max().item()
    invalid = (ref['enc_outputs']['pred_boxes'] == 1).all(-1)
    assert (out['enc_outputs']['pred_boxes'][invalid] == 1).all()
    errs, shares = {}, []
    for b in range(2):
        pos = {int(p): q for q, p in enumerate(ref_topk[b].tolist())}
        mine = [q for q, p in enumerate(topk[b].tolist()) if p in pos]
        theirs = [pos[int(topk[b, q])] for q in mine]
        shares.append(len(mine) / K_PROP)
        for k in ('pred_logits', 'pred_boxes', 'hs_embed'):
            e = (out[k][b, mine].float() - ref[k][b, theirs].float()).abs().max().item()
            errs[k] = max(errs.get(k, 0.0), e)
    print(f'[two_stage] {dtype} vs fp32: enc logits {el:.4g} enc boxes {eb:.4g} common share per frame {shares} '
          + ' '.join(f'{k}={v:.4g}' for k, v in errs.items()))
    assert el < tol['pred_logits'] and eb < tol['pred_boxes']
    assert min(shares) >= COMMON_FLOOR[dtype]
    for k, v in errs.items():
        assert v < tol[k], (k, v, tol[k])
    assert torch.isfinite(out['pred_boxes']).all() and torch.isfinite(out['pred_logits']).all()


def test_graph_replay_is_bit_identical(case_a, frames):
    from kinet_amd.graph import GraphedCall
    model, _ = case_a

    def fn(a, b):
        out = model([a, b])[0]
        return (out['pred_logits'], out['pred_boxes'], out['hs_embed'], out['enc_outputs']['pred_logits'],
                out['enc_outputs']['pred_boxes'], model.transformer.topk_proposals)

    def eager(fs):
        with torch.no_grad():
            r = [t.clone() for t in fn(*fs)]
        torch.cuda.synchronize()
        return r
    g = torch.Generator().manual_seed(77)
    other = [torch.randn(f.shape, generator=g).cuda() for f in frames]
    want0, want1 = eager(frames), eager(other)
    assert not torch.equal(want0[5], want1[5])
    gc = GraphedCall(fn, frames, params=list(model.parameters()) + list(model.buffers()))
    for fs, want in ((frames, want0), (other, want1), (frames, want0)):
        got = gc(*fs)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)


def test_train_mode_forward_raises(case_a, frames):
    model, _ = case_a
    model.train()
    try:
        with pytest.raises(NotImplementedError, match='inference'), torch.no_grad():
            model(frames)
    finally:
        model.eval()
