"""Mask training without a GPU: the opt-in wiring (build_mask_training, build_criterion(mask_losses=True))
against the reference's construction, what stays as it was (build_model, a default model's refusal),
loss_masks skipped for the aux outputs, synthetic_mask_batch, the constants the direct tests' bounds
use (tests/segm_train_refs.py) against autograd in double, and the new entry points' argument checks."""
import math

import pytest
import torch

import segm_refs as R
import segm_train_refs as T
from kinet_amd import _native as N
from kinet_amd import train as TR
from kinet_amd.models import build_model
from kinet_amd.models.criterion import build_criterion


@pytest.fixture(scope='module')
def trained():
    torch.manual_seed(0)
    return TR.build_mask_training(R.case_args('a', freeze_detr=True))


def reference_weights_and_losses(args):
    """models/__init__.py:127-146 of the reference, written out."""
    weight_dict = {'loss_ce': args.cls_loss_coef, 'loss_bbox': args.bbox_loss_coef, 'loss_giou': args.giou_loss_coef}
    if args.masks:
        weight_dict['loss_mask'] = args.mask_loss_coef
        weight_dict['loss_dice'] = args.dice_loss_coef
    if args.aux_loss:
        aux = {}
        for i in range(args.dec_layers - 1):
            aux.update({k + f'_{i}': v for k, v in weight_dict.items()})
        weight_dict.update(aux)
    losses = ['labels', 'boxes', 'cardinality']
    if args.masks:
        losses.append('masks')
    return weight_dict, losses


@pytest.mark.parametrize('over', [dict(), dict(aux_loss=False), dict(mask_loss_coef=3.0, dice_loss_coef=0.5, dec_layers=3)])
def test_mask_losses_wiring_equals_the_references(over):
    args = R.case_args('a', **over)
    model, criterion, post = TR.build_mask_training(args)
    want_w, want_l = reference_weights_and_losses(args)
    assert criterion.weight_dict == want_w and list(criterion.weight_dict) == list(want_w)
    assert criterion.losses == want_l
    if args.aux_loss:
        assert f'loss_mask_{args.dec_layers - 2}' in criterion.weight_dict
    assert model.mask_training is True and 'segm' in post and criterion.matcher is not None


def test_build_model_is_unchanged():
    args = R.case_args('a')
    model, criterion, _ = build_model(args)
    assert model.mask_training is False and model.mask_train_all_rows is False
    assert 'masks' not in criterion.losses and not any('mask' in k or 'dice' in k for k in criterion.weight_dict)
    plain = build_criterion(args, 20, criterion.matcher)
    assert plain.weight_dict == criterion.weight_dict and plain.losses == criterion.losses
    with pytest.raises(NotImplementedError, match='outside'):
        criterion.get_loss('masks', {}, [], [], 1.0)                 # the default criterion does not know the loss
    model.train()
    with pytest.raises(NotImplementedError, match='inference'):
        model([torch.zeros(3, 64, 64)])


def test_build_mask_training_needs_a_masks_config():
    from kinet_amd.models.config import load_args
    with pytest.raises(ValueError, match='masks'):
        TR.build_mask_training(load_args('train_deformable'))
    for over, match in ((dict(two_stage=True), 'two_stage'), (dict(dataset='coco_panoptic'), 'Panoptic')):
        with pytest.raises(NotImplementedError, match=match):
            TR.build_mask_training(load_args('train_deformable', masks=True, **over))


def test_frozen_parameters_stay_out_of_the_optimizer(trained):
    model, _, _ = trained
    opt = TR.build_optimizer(model, R.case_args('a', freeze_detr=True))
    in_opt = {id(p) for g in opt.param_groups for p in g['params']}
    for n, p in model.named_parameters():
        assert (id(p) in in_opt) == n.startswith(('bbox_attention.', 'mask_head.')), n


def test_loss_masks_is_skipped_for_aux_outputs(trained, monkeypatch):
    _, criterion, _ = trained
    calls = []

    def fake(outputs, targets, indices, num_boxes):
        calls.append(outputs)
        return {'loss_mask': torch.zeros(()), 'loss_dice': torch.zeros(())}
    monkeypatch.setattr(criterion, 'loss_masks', fake)
    g = R.gen(5)
    Q, C = 6, criterion.num_classes

    def out():
        return {'pred_logits': torch.randn(2, Q, C, generator=g), 'pred_boxes': torch.rand(2, Q, 4, generator=g) * 0.5 + 0.25}
    outputs = dict(out(), pred_masks=torch.zeros(2, Q, 4, 4), aux_outputs=[out(), out()])
    targets = [{'boxes': torch.rand(k, 4, generator=g) * 0.4 + 0.3, 'labels': torch.zeros(k, dtype=torch.long),
                'masks': torch.zeros(k, 16, 16, dtype=torch.uint8)} for k in (2, 1)]
    losses = criterion(outputs, targets)
    assert len(calls) == 1 and calls[0]['pred_masks'] is outputs['pred_masks']
    assert {'loss_mask', 'loss_dice'} <= set(losses) and not any(k.startswith(('loss_mask_', 'loss_dice_')) for k in losses)
    assert 'loss_ce_0' in losses and 'loss_ce_1' in losses


def test_loss_masks_raises_on_cpu_tensors(trained):
    _, criterion, _ = trained
    outputs = {'pred_masks': torch.zeros(1, 3, 4, 4)}
    targets = [{'masks': torch.ones(2, 16, 16, dtype=torch.uint8)}]
    indices = [(torch.tensor([0, 2]), torch.tensor([1, 0]))]
    with pytest.raises(RuntimeError, match='GPU'):
        criterion.loss_masks(outputs, targets, indices, 2.0)


def test_synthetic_mask_batch_shapes():
    g = torch.Generator().manual_seed(3)
    samples, targets = TR.synthetic_mask_batch(2, 96, 128, torch.device('cpu'), g, num_boxes=(3, 6))
    assert tuple(samples.tensors.shape) == (2, 3, 96, 128) and len(targets) == 2
    for t in targets:
        n = len(t['labels'])
        m = t['masks']
        assert 3 <= n <= 6 and m.dtype == torch.uint8 and tuple(m.shape) == (n, 96, 128) and int(m.max()) <= 1
        assert 'prev_target' in t and 'prev_image' in t and 'track_ids' in t
        scale = t['boxes'].new_tensor([128, 96, 128, 96])
        cx, cy, bw, bh = (t['boxes'] * scale).unbind(-1)
        ys, xs = torch.arange(96.0).view(1, -1, 1) + 0.5, torch.arange(128.0).view(1, 1, -1) + 0.5
        inside = ((xs - cx.view(-1, 1, 1)).abs() <= bw.view(-1, 1, 1) / 2) & ((ys - cy.view(-1, 1, 1)).abs() <= bh.view(-1, 1, 1) / 2)
        assert not (m.bool() & ~inside).any()                         # the ellipse lies inside its box
        big = (bw >= 8) & (bh >= 8) & (inside.flatten(1).sum(1) > 0.99 * bw * bh)
        share = m.flatten(1).sum(1).float() / inside.flatten(1).sum(1).clamp(min=1)
        assert ((share[big] - math.pi / 4).abs() < 0.12).all()        # pi/4 of a box that lies inside the image


def test_focal_derivative_constants_hold():
    """FOCAL_D1 / FOCAL_D2 of segm_train_refs.py (hand-derived caps of |focal'| and |focal''|) against
    autograd in double on a grid of logits, both targets."""
    v = torch.linspace(-30, 30, 24001, dtype=torch.float64, requires_grad=True)
    for t in (0.0, 1.0):
        f = T.focal_terms(v, torch.full_like(v, t))
        d1, = torch.autograd.grad(f.sum(), v, create_graph=True)
        d2, = torch.autograd.grad(d1.sum(), v)
        assert d1.abs().max() <= T.FOCAL_D1 * max(T.ALPHA, 1 - T.ALPHA) and d2.abs().max() <= T.FOCAL_D2 * max(T.ALPHA, 1 - T.ALPHA)
    p = v.sigmoid()
    d, = torch.autograd.grad((p * (1 - p)).sum(), v)
    assert d.abs().max() <= 0.1 and (p * (1 - p)).max() <= 0.25


def test_loss_reference_equals_the_criterions_composition():
    """segm_train_refs.loss_composition is detr.py:779-790: the same numbers as the criterion's own
    sigmoid_focal_loss and the reference's dice_loss formula written out."""
    from kinet_amd.models.criterion import sigmoid_focal_loss
    logits, target = T.loss_case(3, 7, 13, 29, 53, seed=7)
    lm, ld, sums, v = T.loss_composition(logits.double(), target, 2.5)
    t = target.flatten(1).double()
    assert torch.allclose(lm, sigmoid_focal_loss(v, t, 2.5), rtol=1e-12, atol=0)
    p = v.sigmoid()
    dice = (1 - (2 * (p * t).sum(1) + 1) / (p.sum(-1) + t.sum(-1) + 1)).sum() / 2.5      # util/misc.py:616-631
    assert torch.allclose(ld, dice, rtol=1e-12, atol=0)
    assert torch.equal(sums[:, 3], t.sum(1))


# --------------------------------------------------------------------------- the C ABI's argument checks
def _err(name, *args):
    with pytest.raises(RuntimeError) as e:
        N.call(name, *args)
    return str(e.value)


def test_abi_rejects_bad_arguments_before_any_launch():
    z = None
    assert 'at least' in _err('kinet_segm_mask_loss', z, z, z, 8, 1, 8, 8, 4, 8, 0.25, 2.0, 1.0, z, z)
    assert 'gamma' in _err('kinet_segm_mask_loss', z, z, z, 8, 1, 4, 4, 8, 8, 0.25, 1.0, 1.0, z, z)
    assert 'num_boxes' in _err('kinet_segm_mask_loss', z, z, z, 8, 1, 4, 4, 8, 8, 0.25, 2.0, 0.0, z, z)
    assert 'null' in _err('kinet_segm_mask_loss', z, z, z, z, 1, 4, 4, 8, 8, 0.25, 2.0, 1.0, z, z)
    assert 'workspace' in _err('kinet_segm_mask_loss', 8, 8, 8, 8, 1, 4, 4, 8, 8, 0.25, 2.0, 1.0, z, z)
    assert 'at least' in _err('kinet_segm_mask_loss_backward', z, z, z, z, z, 1, 8, 8, 8, 4, 0.25, 2.0, 1.0, z)
    assert 'null' in _err('kinet_segm_mask_loss_backward', z, z, z, z, z, 1, 4, 4, 8, 8, 0.25, 2.0, 1.0, z)
    assert 'heads' in _err('kinet_segm_attention_backward', z, z, z, z, z, z, 1, 1, 4, 6, 252, 0.1, z, z)
    assert 'null' in _err('kinet_segm_attention_backward', z, z, z, z, z, z, 1, 1, 4, 8, 256, 0.1, z, z)
    assert 'workspace' in _err('kinet_segm_attention_backward', 8, 8, 8, 8, z, z, 1, 1, 4, 8, 256, 0.1, z, z)
    assert 'multiple of 4' in _err('kinet_segm_relu_up_add', z, z, z, 1, 0, 1, 1, 4, 4, 8, 8, 18, z)
    assert 'output has the input' in _err('kinet_segm_relu_up_add', z, z, z, 1, 0, 1, 1, 4, 4, 8, 8, 16, z)
    assert 'at least' in _err('kinet_segm_relu_up_add', z, z, z, 1, 0, 1, 1, 8, 8, 4, 4, 16, z)
    assert 'outside' in _err('kinet_segm_relu_up_add', z, z, z, 4, 3, 3, 2, 4, 4, 4, 4, 16, z)
    assert 'aligned' in _err('kinet_segm_relu_up_add', 16, z, 24, 1, 0, 1, 1, 4, 4, 4, 4, 16, z)
    assert 'null' in _err('kinet_segm_relu_up_add_backward', z, z, z, z, 1, 0, 1, 1, 4, 4, 4, 4, 16, z)
    assert 'C must' in _err('kinet_segm_out_conv_backward', z, z, z, z, z, z, 1, 4, 4, 128, z, z)
    assert 'go together' in _err('kinet_segm_out_conv_backward', z, z, z, z, 8, z, 1, 4, 4, 16, z, z)
    assert 'null' in _err('kinet_segm_out_conv_backward', z, z, z, z, z, z, 1, 4, 4, 16, z, z)
    assert 'workspace' in _err('kinet_segm_out_conv_backward', 8, 8, 8, z, 8, 8, 1, 4, 4, 16, z, z)


def test_abi_empty_calls_and_workspaces():
    z = None
    L = N.lib()
    assert N.call('kinet_segm_mask_loss_backward', z, z, z, z, z, 0, 4, 4, 8, 8, 0.25, 2.0, 1.0, z) == 0
    assert N.call('kinet_segm_attention_backward', z, z, z, z, z, z, 2, 0, 4, 8, 256, 0.1, z, z) == 0
    assert N.call('kinet_segm_relu_up_add', z, z, z, 0, 0, 1, 1, 4, 4, 4, 4, 16, z) == 0
    assert L.kinet_segm_mask_loss_workspace(3, 28, 52) == 3 * 1 * 4
    assert L.kinet_segm_mask_loss_workspace(3, 106, 202) == 3 * T.loss_blocks(106, 202) * 4 == 3 * 6 * 4
    assert L.kinet_segm_mask_loss_workspace(0, 28, 52) == 0
    assert L.kinet_segm_attention_backward_workspace(2, 5) == 10
    assert L.kinet_segm_out_conv_backward_workspace(5, 26, 50, 16) == 7 * (9 * 16 + 1)      # 6500 pixels in blocks of 1024


# --------------------------------------------------------------------------- the fixture's recorded conditions
def test_fixture_conditions(golden_dir):
    """What make_golden_segm_train.py asserted when it wrote segm_train.npz, re-checked on the stored data."""
    import os

    import numpy as np
    path = os.path.join(golden_dir, 'segm_train.npz')
    d = np.load(path)
    assert os.path.getsize(path) < min(1 << 20, os.path.getsize(os.path.join(golden_dir, 'train_step_small.npz')))
    for (_, H, W), boxes in zip(T.TRAIN_FRAMES, T.TRAIN_BOXES):
        assert (H + 3) // 4 != H / 4                                                  # the stride-4 map is not H / 4
        share = T.ellipse_masks(boxes, H, W).flatten(1).sum(1).double() / torch.tensor([b[2] * W * b[3] * H for b in boxes])
        assert ((share > 0.1) & (share < 0.9)).all()
    assert [len(t['boxes']) for t in T.train_targets()] == [3, 2]
    keys = R.key_shapes(golden_dir, 'train')
    for run in ('frozen', 'full'):
        rows = [d[f'{run}_rows{b}'] for b in range(2)]
        assert sum(len(r) for r in rows) >= 5 and all(len(set(r.tolist())) == len(r) for r in rows)
        names = [k.split(':', 1)[1] for k in d.files if k.startswith(f'{run}_grad:')]
        head = [n for n in names if n.startswith(('bbox_attention.', 'mask_head.'))]
        assert len(head) == 32 and set(names) - set(head) == (set() if run == 'frozen' else set(T.TRAIN_DETECTOR_GRADS))
        for n in names:
            g = d[f'{run}_grad:{n}']
            numel = int(np.prod(keys[n]))
            assert g.dtype == np.float32 and g.size == T.lattice(torch.empty(numel)).numel() <= T.LATTICE_MAX
            peak = float(np.abs(g).max())
            assert peak > 0 and float(d[f'{run}_norm:{n}']) >= peak * (1 - 1e-6)
            assert 10 * float(d[f'{run}_err64:{n}']) < T.grad_gate(n, peak), n
        for k in ('loss_ce', 'loss_bbox', 'loss_giou', 'loss_mask', 'loss_dice', 'loss_total'):
            assert np.isfinite(d[f'{run}_{k}']) and float(d[f'{run}_{k}']) > 0
        assert abs(float(d[f'{run}_loss_total']) - float(d[f'{run}_loss_total64'])) < 1e-4 * float(d[f'{run}_loss_total64'])
    assert not any('loss_mask_' in k or 'loss_dice_' in k for k in d.files)           # no mask losses on aux outputs
