"""Ragged track queries in the Deformable detector (targets[i]['track_queries_placeholder_mask']): on the
small tracking model, B = 2 with K = (3, 1) track queries (Kmax = 3), the placeholder rows' contents reach no
other row (bit for bit), each sample agrees with its own batch-1 forward, and a forward without the key is
untouched."""
import os

import numpy as np
import pytest
import torch

import multi_track_refs as R

pytestmark = pytest.mark.gpu

K_I = (3, 1)
KMAX = 3
OUT = ('pred_logits', 'pred_boxes', 'hs_embed')


@pytest.fixture(scope='module')
def setup(golden_dir):
    d = dict(np.load(os.path.join(golden_dir, 'detr_tracking_mf_small.npz')))
    model = R.small_tracking_model(golden_dir)
    model.set_compute_dtype(torch.float32)
    f0, f1 = torch.from_numpy(d['frame0']).cuda(), torch.from_numpy(d['frame1']).cuda()
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        out0, _, feats, _, _ = model([f0, f1])
    top = torch.from_numpy(d['top_idx']).cuda()[:KMAX]
    embeds = out0['hs_embed'][:, top].clone()                      # (2, Kmax, d) plausible track queries
    boxes = out0['pred_boxes'][:, top].clone()
    noise = (torch.randn(2, KMAX, embeds.shape[-1], generator=g).cuda(),
             (torch.rand(2, KMAX, 4, generator=g) * 0.8 + 0.1).cuda())
    return model, [f1, f0], feats, embeds, boxes, noise


def _targets(embeds, boxes, Q, fill=None, mask=True):
    out = []
    for i, k in enumerate(K_I):
        e, b = embeds[i].clone(), boxes[i].clone()
        e[k:], b[k:] = 0.0, 0.5
        if fill is not None:
            e[k:], b[k:] = fill[0][i, k:], fill[1][i, k:]
        t = {'track_query_hs_embeds': e, 'track_query_boxes': b}
        if mask:
            m = torch.zeros(KMAX + Q, dtype=torch.bool, device='cuda')
            m[k:KMAX] = True
            t['track_queries_placeholder_mask'] = m
        out.append(t)
    return out


def _real_rows(Q):
    rows = torch.ones(2, KMAX + Q, dtype=torch.bool)
    for i, k in enumerate(K_I):
        rows[i, k:KMAX] = False
    return rows


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_placeholder_contents_reach_no_other_row(setup, dtype):
    model, frames, feats, embeds, boxes, noise = setup
    Q = model.num_queries
    model.set_compute_dtype(dtype)
    try:
        with torch.no_grad():
            a = model(frames, _targets(embeds, boxes, Q), feats)[0]
            b = model(frames, _targets(embeds, boxes, Q, fill=noise), feats)[0]
        rows = _real_rows(Q)
        for name in OUT:
            x, y = a[name].cpu(), b[name].cpu()
            assert tuple(x.shape[:2]) == (2, KMAX + Q)
            assert torch.isfinite(x[rows]).all()
            assert torch.equal(x[rows], y[rows]), name
    finally:
        model.set_compute_dtype(torch.float32)


def test_each_sample_matches_its_batch_one_forward(setup, capsys):
    """f32: the same arithmetic reordered, under the project's f32 parity gate of 1e-3 absolute."""
    from kinet_amd.models.misc import NestedTensor
    model, frames, feats, embeds, boxes, noise = setup
    Q = model.num_queries
    with torch.no_grad():
        ragged = model(frames, _targets(embeds, boxes, Q), feats)[0]
        worst = 0.0
        for i, k in enumerate(K_I):
            prev = [NestedTensor(f.tensors[i:i + 1], f.mask[i:i + 1], None if f.sizes is None else f.sizes[i:i + 1])
                    for f in feats]
            t = [{'track_query_hs_embeds': embeds[i, :k].clone(), 'track_query_boxes': boxes[i, :k].clone()}]
            one = model([frames[i]], t, prev)[0]
            for name in OUT:
                got = torch.cat([ragged[name][i, :k], ragged[name][i, KMAX:]])
                err = (got - one[name][0]).abs().max().item()
                worst = max(worst, err)
                assert err <= 1e-3, (name, i, err)
    with capsys.disabled():
        print(f'\nragged vs batch-1 forward, f32: max abs difference {worst:.3e}')


def test_without_the_key_nothing_changes(setup):
    """Equal K and no key: the parent's code path.  With an all-False mask the same rows come out bit for
    bit, so the expected tensors are the mask-free call's own."""
    model, frames, feats, embeds, boxes, noise = setup
    Q = model.num_queries
    plain = [{'track_query_hs_embeds': embeds[i].clone(), 'track_query_boxes': boxes[i].clone()} for i in range(2)]
    masked = [dict(t, track_queries_placeholder_mask=torch.zeros(KMAX + Q, dtype=torch.bool, device='cuda')) for t in plain]
    with torch.no_grad():
        a = model(frames, plain, feats)[0]
        b = model(frames, masked, feats)[0]
        c = model(frames, plain, feats)[0]
    for name in OUT:
        assert torch.equal(a[name], c[name]), name
        assert torch.equal(a[name], b[name]), name


def test_mask_shape_is_checked(setup):
    model, frames, feats, embeds, boxes, noise = setup
    t = _targets(embeds, boxes, model.num_queries)
    for x in t:
        x['track_queries_placeholder_mask'] = x['track_queries_placeholder_mask'][:-1]
    with pytest.raises(ValueError), torch.no_grad():
        model(frames, t, feats)
