"""Mask training on the GPU (kinet_amd.train.build_mask_training): one training step against the
reference's (tests/golden/segm_train.npz, made by make_golden_segm_train.py: losses and gradients of
DeformableDETRSegm with the mask / dice losses, detector frozen and unfrozen), the matched-rows
backward against differentiating every row, a few optimisation steps of the tracking class on a
synthetic batch, and the inference path after training.  fp32, dropout 0.

Measured on MI355X (exact f32 matmuls, 'highest'): see DESIGN.md section 4, "Mask training"."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import segm_refs as R
import segm_train_refs as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'segm_train.npz'))


@pytest.fixture
def highest():
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision('highest')
    yield
    torch.set_float32_matmul_precision(prev)


def build(golden_dir, seed, freeze, mask_training=True):
    sys.path.insert(0, golden_dir)
    from segm_weights import condition
    from weights import make_state_dict
    from kinet_amd.models import build_model
    from kinet_amd.train import build_mask_training
    args = R.case_args('a', freeze_detr=freeze, device='cuda', **T.TRAIN_OVER)
    model, criterion, _ = (build_mask_training if mask_training else build_model)(args)
    model.load_state_dict(make_state_dict(R.key_shapes(golden_dir, 'train'), seed=seed))
    return args, condition(model).cuda().train(), criterion.cuda()


def batch():
    from kinet_amd.models import nested_tensor_from_tensor_list
    samples = nested_tensor_from_tensor_list([f.cuda() for f in T.train_frames()])
    targets = [{k: v.cuda() for k, v in t.items()} for t in T.train_targets()]
    return samples, targets


def step(model, criterion):
    from kinet_amd.train import weighted_loss
    samples, targets = batch()
    model.zero_grad(set_to_none=True)
    out, targets, *_ = model(samples, targets)
    out['pred_masks'].retain_grad()
    losses = criterion(out, targets)
    total = weighted_loss(losses, criterion.weight_dict)
    total.backward()
    return out, losses, total


def head_names(model):
    return [n for n, _ in model.named_parameters() if n.startswith(('bbox_attention.', 'mask_head.'))]


@pytest.mark.parametrize('run', ['frozen', 'full'])
def test_training_step_matches_reference(golden_dir, fixture, highest, run):
    """Losses to rtol 1e-3 / atol 1e-4 and gradients to 2e-3 max|ref| + 1e-5 (5e-3 for the backbone weight):
    the gates of tests/test_train_gpu.py.  The loss values come from the inference kernels' logits, the
    gradients from the head recomputed on the matched rows."""
    d = fixture
    args, model, criterion = build(golden_dir, int(d['seed']), freeze=run == 'frozen')
    out, losses, total = step(model, criterion)
    assert out['pred_masks'].shape == (2, R.N_QUERIES, 27, 51)
    assert model.last_mask_rows == [sorted(d[f'{run}_rows{b}'].tolist()) for b in range(2)]      # the matcher's rows
    for k, v in losses.items():
        want = float(d[f'{run}_{k}'])
        print(f'[loss] {run} {k}: {v.item():.7g} ref {want:.7g} diff {abs(v.item() - want):.2e}')
        np.testing.assert_allclose(v.item(), want, rtol=1e-3, atol=1e-4, err_msg=k)
    assert {'loss_mask', 'loss_dice'} <= set(losses)
    np.testing.assert_allclose(total.item(), float(d[f'{run}_loss_total']), rtol=1e-3)
    params = dict(model.named_parameters())
    names = [k.split(':', 1)[1] for k in d.files if k.startswith(f'{run}_grad:')]
    assert set(head_names(model)) <= set(names) and len(names) == 32 + (0 if run == 'frozen' else len(T.TRAIN_DETECTOR_GRADS))
    bad = []
    for n in names:
        g = params[n].grad
        assert g is not None, n
        ref = torch.from_numpy(d[f'{run}_grad:{n}'])
        got = T.lattice(g).cpu()
        peak = ref.abs().max().item()
        err = (got - ref).abs().max().item()
        gate = T.grad_gate(n, peak)
        # the whole tensor through its L2 norm: | ||g|| - ||ref|| | <= ||g - ref|| <= sqrt(numel) * the element gate
        norm_err = abs(g.double().norm().item() - float(d[f'{run}_norm:{n}']))
        print(f'[grad] {run} {n}: max err {err:.3e} rel {err / peak:.3e} (reference f32-vs-f64 '
              f'{float(d[f"{run}_err64:{n}"]):.2e}), norm err {norm_err:.3e} of {float(d[f"{run}_norm:{n}"]):.3e}')
        if err > gate or norm_err > math.sqrt(g.numel()) * gate:
            bad.append((n, err, gate, norm_err))
    assert not bad, bad
    detector = [n for n in params if n not in head_names(model)]
    if run == 'frozen':
        assert all(params[n].grad is None and not params[n].requires_grad for n in detector)
    else:
        assert sum(params[n].grad is not None and bool(params[n].grad.abs().max() > 0) for n in detector) > 100
        assert params['backbone.0.body.layer1.0.conv1.weight'].grad is None        # layer1 stays frozen


def test_high_precision_mode_runs(golden_dir, fixture):
    """'high' (three bf16 MFMA passes per f32 product, the training benchmark's setting): printed, not gated."""
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision('high')
    try:
        d = fixture
        args, model, criterion = build(golden_dir, int(d['seed']), freeze=True)
        out, losses, total = step(model, criterion)
        params = dict(model.named_parameters())
        for n in head_names(model):
            ref = torch.from_numpy(d[f'frozen_grad:{n}'])
            err = (T.lattice(params[n].grad).cpu() - ref).abs().max().item()
            print(f'[grad high] {n}: rel {err / ref.abs().max().item():.3e}')
        assert torch.isfinite(total) and all(torch.isfinite(p.grad).all() for n, p in params.items() if p.grad is not None)
    finally:
        torch.set_float32_matmul_precision(prev)


def test_matched_rows_backward_equals_all_rows(golden_dir, fixture, highest):
    """The head gradients from the rows that carry a gradient against those from differentiating the
    recomputed head over all B*Q rows.  The unmatched rows' incoming gradient is exactly zero, so both
    are f32 evaluations of the SAME sums (an unmatched row adds exact zeros) in different orders: the
    GEMMs' tiles and split-K chunks fall differently over 24 rows than over 5.  Each evaluation is off
    the exact sum by its own rounding error, and the two differ by at most the sum of those.  The scale
    of one such error is known for this very gradient: the reference's f32 run is a third f32 evaluation
    of the same sums and its distance from f64 is stored (err64, a maximum over the stored lattice only,
    taken with other chain splits than ours: allowed 4x per evaluation), next to the roundings of the
    final additions (4 u max|g| per evaluation).  Bound: 8 err64 + 8 u max|g|."""
    d = fixture
    args, model, criterion = build(golden_dir, int(d['seed']), freeze=True)
    out, _, _ = step(model, criterion)
    dseg = out['pred_masks'].grad
    live = model.last_mask_rows
    assert sum(len(r) for r in live) == 5
    for b in range(2):
        dead = [q for q in range(R.N_QUERIES) if q not in live[b]]
        assert (dseg[b, dead] == 0).all() and all((dseg[b, q] != 0).any() for q in live[b])
    params = dict(model.named_parameters())
    matched = {n: params[n].grad.clone() for n in head_names(model)}
    model.mask_train_all_rows = True
    step(model, criterion)
    assert model.last_mask_rows == [list(range(R.N_QUERIES))] * 2
    bad = []
    for n, g in matched.items():
        diff = (params[n].grad - g).abs().max().item()
        peak = g.abs().max().item()
        bound = 8 * float(d[f'frozen_err64:{n}']) + 8 * R.U32 * peak
        print(f'[rows] {n}: matched vs all rows {diff:.3e} (bound {bound:.3e}, max |g| {peak:.3e})')
        if diff > bound:
            bad.append((n, diff, bound))
    assert not bad, bad


@pytest.mark.parametrize('freeze', [False, True], ids=['unfrozen', 'frozen'])
def test_tracking_class_trains(freeze):
    """DeformableDETRSegmTracking (train_tracking): 4 train_steps on one synthetic batch."""
    from kinet_amd.models import DeformableDETRSegmTracking
    from kinet_amd.models.config import load_args
    from kinet_amd.train import build_mask_training, build_optimizer, synthetic_mask_batch, train_step
    args = load_args('train_deformable', 'train_tracking', masks=True, freeze_detr=freeze, num_queries=R.N_QUERIES,
                     device='cuda', **T.TRAIN_OVER)
    torch.manual_seed(0)
    model, criterion, _ = build_mask_training(args)
    assert type(model) is DeformableDETRSegmTracking
    model = model.cuda().train()
    samples, targets = synthetic_mask_batch(2, 96, 128, torch.device('cuda'), torch.Generator().manual_seed(3),
                                            num_boxes=(3, 6))
    opt = build_optimizer(model, args)
    n_opt = sum(len(g['params']) for g in opt.param_groups)
    assert n_opt == (32 if freeze else sum(p.requires_grad for p in model.parameters()))
    mask_losses = []
    for i in range(4):
        torch.manual_seed(5)
        tg = [dict(t, prev_target=dict(t['prev_target'])) for t in targets]
        loss, loss_dict = train_step(model, criterion, opt, samples, tg, args.clip_max_norm)
        assert torch.isfinite(loss) and all(torch.isfinite(v).all() for v in loss_dict.values())
        mask_losses.append((loss_dict['loss_mask'] + loss_dict['loss_dice']).item())
        if i == 0:
            params = dict(model.named_parameters())
            head = [params[n].grad for n in params if n.startswith(('bbox_attention.', 'mask_head.'))]
            assert len(head) == 32 and all(g is not None and bool(g.abs().max() > 0) for g in head)
            det = [p.grad for n, p in params.items() if not n.startswith(('bbox_attention.', 'mask_head.'))]
            if freeze:
                assert all(g is None for g in det)
            else:
                assert sum(g is not None and bool(g.abs().max() > 0) for g in det) > 100
    print(f'[track] freeze={freeze} loss_mask + loss_dice per step: {mask_losses}')
    assert mask_losses[3] < mask_losses[0], mask_losses


def test_inference_after_training_is_the_fast_path(golden_dir, fixture):
    """After an optimisation step, pred_masks of the trained model's eval / no_grad forward equals, bit for
    bit, the fast path's of a plain build_model model holding the same weights: training changes nothing
    the inference path reads (and no cached packed weight survives the in-place update)."""
    from kinet_amd.train import build_optimizer
    d = fixture
    args, model, criterion = build(golden_dir, int(d['seed']), freeze=False)
    samples, _ = batch()
    model.eval()
    with torch.no_grad():
        before = model(samples)[0]['pred_masks'].clone()
    model.train()
    opt = build_optimizer(model, args)
    step(model, criterion)
    opt.step()
    model.eval()
    with torch.no_grad():
        after = model(samples)[0]['pred_masks']
    assert not torch.equal(before, after)
    _, plain, _ = build(golden_dir, int(d['seed']), freeze=False, mask_training=False)
    plain.load_state_dict(model.state_dict())
    plain.eval()
    assert plain.mask_training is False
    with torch.no_grad():
        want = plain(samples)[0]['pred_masks']
    assert torch.equal(after, want)
    with pytest.raises(NotImplementedError, match='inference'):
        plain.train()(samples)
