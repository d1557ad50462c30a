"""Vanilla DETR (config 1) on the GPU against the reference model's outputs
(tests/golden/make_golden_detr.py; same name-seeded weights, frames regenerated from CPU
generator seeds).  Every case runs frames of 3x672x992 and 3x608x800 in one NestedTensor: a
21x31 feature map = 651 keys, above the resident attention kernels' caps, so the 16-bit modes
run the key-streaming MFMA kernel at head_dim 32 (case A) and 36 (cases B, C); 176 keys of the
second frame are padding.

  A  load_args():                     d 256, 100 queries
  B  load_args('train_detr'):         d 288, 500 queries
  C  B with tracking=True, tracking mode, 5 track queries per frame

fp32 vs the reference within 1e-3 abs (the project's gate, test_fullsize_gpu.TOL); bf16 / f16 vs
the reference within the per-tensor bounds below; the same 16-bit forward with the attention
core forced onto the FMA kernel within the same bounds of the default run.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-3
FRAMES = ((1101, 672, 992), (1102, 608, 800))
N_TRACK = 5
KEYS = ('pred_logits', 'pred_boxes', 'hs_embed')
# 16-bit compute vs the REFERENCE's fp32 outputs (max |diff| per tensor over the stored queries),
# and vs the same forward with the attention core on the FMA kernel.  Measured on MI355X
# (profiles/detr_vanilla_tolerances.log), pred_logits / pred_boxes / hs_embed:
#   A bf16  vs reference 0.06227 / 0.004553 / 0.1161     vs FMA core 0.02766 / 0.003647 / 0.03882
#   B bf16  vs reference 0.03913 / 0.003554 / 0.05632    vs FMA core 0.03242 / 0.003822 / 0.0625
#   B f16   vs reference 0.004262 / 0.0004611 / 0.00828  vs FMA core 0.003534 / 0.0004782 / 0.007812
# The bounds are ~1.6x the largest measured value per tensor and dtype, the convention of
# test_fullsize_gpu.BF16_TOL / F16_TOL (whose deformable-path bf16 logit bound is 0.3).
BF16_TOL = {'pred_logits': 0.1, 'pred_boxes': 0.0075, 'hs_embed': 0.19}
F16_TOL = {'pred_logits': 0.007, 'pred_boxes': 0.0008, 'hs_embed': 0.0135}

_SD = {}


def _state_dict(golden_dir, keyfile, seed):
    from weights import make_state_dict
    if (keyfile, seed) not in _SD:
        shapes = {}
        for ln in open(os.path.join(golden_dir, keyfile)):
            k, *s = ln.split()
            shapes[k] = [int(x) for x in s]
        _SD[(keyfile, seed)] = make_state_dict(shapes, seed=seed)
    return _SD[(keyfile, seed)]


def _build(golden_dir, keyfile, seed, *cfgs, **over):
    from kinet_amd.models import build_model
    from kinet_amd.models.config import load_args
    model, _, _ = build_model(load_args(*cfgs, **over))
    model.load_state_dict(_state_dict(golden_dir, keyfile, seed))
    return model.cuda().eval()


@pytest.fixture(scope='module')
def frames():
    return [torch.randn(3, h, w, generator=torch.Generator().manual_seed(s)).cuda() for s, h, w in FRAMES]


@pytest.fixture(scope='module')
def case_a(golden_dir):
    return _build(golden_dir, 'detr_vanilla_a.keys.txt', 101), dict(np.load(os.path.join(golden_dir, 'detr_vanilla_a.npz')))


@pytest.fixture(scope='module')
def case_b(golden_dir):
    return (_build(golden_dir, 'detr_vanilla_b.keys.txt', 102, 'train_detr'),
            dict(np.load(os.path.join(golden_dir, 'detr_vanilla_b.npz'))))


@pytest.fixture(scope='module')
def case_c(golden_dir):
    model = _build(golden_dir, 'detr_vanilla_b.keys.txt', 102, 'train_detr', tracking=True)
    model.tracking()
    return model, dict(np.load(os.path.join(golden_dir, 'detr_vanilla_c.npz')))


def _track_targets(d):
    g = torch.Generator().manual_seed(113)
    return [{'track_query_hs_embeds': torch.randn(N_TRACK, d, generator=g).cuda()} for _ in FRAMES]


def _fwd(model, frames, dtype, targets=None, knob=None):
    from kinet_amd import _native
    model.set_compute_dtype(dtype)
    old = _native.lib().kinet_mha_set_mfma(knob) if knob is not None else None
    try:
        with torch.no_grad():
            r = model(frames, targets)
        torch.cuda.synchronize()
        return r
    finally:
        if knob is not None:
            _native.lib().kinet_mha_set_mfma(old)
        model.set_compute_dtype(torch.float32)


def _diffs(out, d):
    """max |out - fixture| per tensor at the stored query indices."""
    q = torch.from_numpy(d['qsel']).cuda()
    return {k: float(np.abs(out[k][:, q].float().cpu().numpy() - d[k]).max()) for k in KEYS}


def _report(tag, diffs):
    print(f'[detr_vanilla] {tag}: ' + ' '.join(f'{k}={v:.4g}' for k, v in diffs.items()))


def _check_fp32(ret, d, n_queries, dim):
    out, _, features, memory, hs = ret
    q = torch.from_numpy(d['qsel']).cuda()

    def close(t, ref):
        np.testing.assert_allclose(t.float().cpu().numpy(), ref, atol=TOL, rtol=0)
    for k in KEYS:
        close(out[k][:, q], d[k])
    assert len(out['aux_outputs']) == 5
    for i, aux in enumerate(out['aux_outputs']):
        close(aux['pred_logits'][:, q], d[f'aux{i}_logits'])
        close(aux['pred_boxes'][:, q], d[f'aux{i}_boxes'])
    close(memory[:, :, ::3, ::3], d['memory_sub'])
    # shapes: the reference's own
    assert tuple(out['pred_logits'].shape) == tuple(d['shape_logits']) == (2, n_queries, 92)
    assert tuple(out['pred_boxes'].shape) == (2, n_queries, 4)
    assert tuple(out['hs_embed'].shape) == tuple(d['shape_hs_embed']) == (2, n_queries, dim)
    assert tuple(memory.shape) == tuple(d['shape_memory']) == (2, dim, 21, 31)
    assert tuple(hs.shape) == tuple(d['shape_hs']) == (6, 2, n_queries, dim)
    assert len(features) == 1 and tuple(features[-1].tensors.shape) == (2, 2048, 21, 31)
    assert int(features[-1].mask[1].sum()) == 176 and not features[-1].mask[0].any()


def test_case_a_fp32_parity(case_a, frames):
    model, d = case_a
    _check_fp32(_fwd(model, frames, torch.float32), d, 100, 256)


def test_case_b_fp32_parity(case_b, frames):
    model, d = case_b
    _check_fp32(_fwd(model, frames, torch.float32), d, 500, 288)


def test_case_c_tracking_fp32_parity(case_c, frames):
    """Tracking mode with track queries: prepended as tgt with zero query positions, and each
    target's entry rewritten to its (K + Q, d) tgt (detr.py:99-117)."""
    model, d = case_c
    targets = _track_targets(288)
    given = [t['track_query_hs_embeds'].clone() for t in targets]
    ret = _fwd(model, frames, torch.float32, targets)
    _check_fp32(ret, d, N_TRACK + 500, 288)
    assert ret[1] is targets
    for t, g in zip(targets, given):
        e = t['track_query_hs_embeds']
        assert tuple(e.shape) == (N_TRACK + 500, 288)
        assert torch.equal(e[:N_TRACK], g) and not e[N_TRACK:].any()


def _check_16bit(model, d, frames, dtype, bounds, tag):
    out = _fwd(model, frames, dtype)[0]
    diffs = _diffs(out, d)
    _report(f'{tag} vs reference', diffs)
    out_fma = _fwd(model, frames, dtype, knob=0)[0]
    vs_fma = {k: (out[k].float() - out_fma[k].float()).abs().max().item() for k in KEYS}
    _report(f'{tag} default vs FMA attention core', vs_fma)
    for k, tol in bounds.items():
        assert diffs[k] < tol, (k, diffs[k], tol)
        assert vs_fma[k] < tol, (k, vs_fma[k], tol)
    boxes = out['pred_boxes']
    assert torch.isfinite(boxes).all() and (boxes >= 0).all() and (boxes <= 1).all()
    for aux in out['aux_outputs']:
        assert torch.isfinite(aux['pred_boxes']).all() and torch.isfinite(aux['pred_logits']).all()


def test_case_a_bf16_vs_reference(case_a, frames):
    _check_16bit(*case_a, frames, torch.bfloat16, BF16_TOL, 'A bf16')


def test_case_b_bf16_vs_reference(case_b, frames):
    _check_16bit(*case_b, frames, torch.bfloat16, BF16_TOL, 'B bf16')


def test_case_b_f16_vs_reference(case_b, frames):
    _check_16bit(*case_b, frames, torch.float16, F16_TOL, 'B f16')


def test_sixteen_bit_forward_runs_the_streaming_kernel(case_a, frames):
    """The 651-key attention calls of the 16-bit forward leave the FMA kernel: forcing it back
    changes the bits (within the bounds, see above)."""
    model, _ = case_a
    a = _fwd(model, frames, torch.bfloat16)[0]['hs_embed']
    assert torch.equal(a, _fwd(model, frames, torch.bfloat16)[0]['hs_embed'])
    assert not torch.equal(a, _fwd(model, frames, torch.bfloat16, knob=0)[0]['hs_embed'])


def test_train_mode_forward_raises(case_a, frames):
    model, _ = case_a
    model.train()
    try:
        with pytest.raises(NotImplementedError), torch.no_grad():
            model(frames)
    finally:
        model.eval()
