"""Two-stage training without a GPU: the f64 references of tests/two_stage_train_refs.py against the
compositions the kernels replace (HungarianMatcher.cost_matrix block by block, loss_labels_focal), the
builder kinet_amd.train.build_two_stage_training, the criterion's enc_outputs branch on the torch
composition (CPU tensors take no kernel), and the C ABI of csrc/criterion.hip rejecting bad arguments
before any device work."""
import os

import numpy as np
import pytest
import torch

import two_stage_train_refs as T


def _args(**over):
    from kinet_amd.models.config import load_args
    return load_args('train_deformable', **dict(T.TRAIN_OVER, **over))


def _targets(labels, tboxes, sizes):
    out, o = [], 0
    for n in sizes:
        out.append({'labels': labels[o:o + n], 'boxes': tboxes[o:o + n]})
        o += n
    return out


# ------------------------------------------------------------------------- references vs compositions
@pytest.mark.parametrize('B,Q,C,sizes', [(1, 1, 1, [1]), (3, 63, 20, [3, 0, 2]), (2, 257, 91, [5, 7])])
def test_cost_reference_is_the_matchers_diagonal_blocks(B, Q, C, sizes):
    from kinet_amd.models.matcher import HungarianMatcher
    logits, boxes, labels, tboxes = T.cost_case(B, Q, C, sizes, seed=11 + Q)
    m = HungarianMatcher(cost_class=2.0, cost_bbox=5.0, cost_giou=2.0, focal_loss=True)
    ref, tol = T.match_cost_ref(logits, boxes, labels, tboxes, sizes, 2.0, 5.0, 2.0)
    assert ref.shape == (Q, sum(sizes)) and (tol > 0).all() and tol.max() < 1e-4
    # HungarianMatcher.cost_matrix itself (f32).  Its class cost forms 1 - p by subtraction, so the argument
    # of log(1 - p + 1e-8) carries up to 2^-23 absolute: log1p(2^-23 / (q + 1e-8)) on the log, which reaches
    # 2.5 at a logit of +20 -- the error the kernel avoids by forming q = 1 - p directly.
    full = m.cost_matrix({'pred_logits': logits, 'pred_boxes': boxes}, _targets(labels, tboxes, sizes))
    p64, q64, _, _ = T.logit_terms(logits.double())
    o = 0
    for b, n in enumerate(sizes):
        if n:
            lab = labels[o:o + n]
            coarse = 2.0 * (0.75 * torch.log1p(2.0 ** -23 / (q64[b][:, lab] + 1e-8))
                            + 0.25 * torch.log1p(2.0 ** -23 / (p64[b][:, lab] + 1e-8))) + 1e-4
            assert ((full[b][:, o:o + n].double() - ref[:, o:o + n]).abs() <= coarse).all()
        o += n
    # the same blocks from f64 arithmetic spelled as the composition spells it (1 - p formed by subtraction)
    p = logits.double().sigmoid()
    o = 0
    for b, n in enumerate(sizes):
        if n:
            lab = labels[o:o + n]
            neg = 0.75 * p[b][:, lab] ** 2 * -(1 - p[b][:, lab] + 1e-8).log()
            pos = 0.25 * (1 - p[b][:, lab]) ** 2 * -(p[b][:, lab] + 1e-8).log()
            from kinet_amd.models.misc import box_cxcywh_to_xyxy, generalized_box_iou
            giou = generalized_box_iou(box_cxcywh_to_xyxy(boxes[b].double()), box_cxcywh_to_xyxy(tboxes[o:o + n].double()))
            want = 5.0 * torch.cdist(boxes[b].double(), tboxes[o:o + n].double(), p=1) + 2.0 * (pos - neg) - 2.0 * giou
            # (the subtraction costs f64 the same way, 2^-52 on the logs' arguments)
            fine = 2.0 * (0.75 * torch.log1p(2.0 ** -52 / (q64[b][:, lab] + 1e-8))
                          + 0.25 * torch.log1p(2.0 ** -52 / (p64[b][:, lab] + 1e-8))) + 1e-11
            assert ((want - ref[:, o:o + n]).abs() <= fine).all()
        o += n


def test_cost_reference_extremes():
    """Logits of +-100 and (1, 1, 1, 1) boxes: finite, and the class term is the composition's limit."""
    logits, boxes, labels, tboxes = T.cost_case(2, 5, 3, [2, 1], seed=3)
    logits[0] = 100.0
    logits[1] = -100.0
    boxes[0, 2] = 1.0
    ref, tol = T.match_cost_ref(logits, boxes, labels, tboxes, [2, 1], 2.0, 5.0, 2.0)
    assert torch.isfinite(ref).all() and torch.isfinite(tol).all()
    assert T.boxes_ok_ref(boxes, tboxes)
    boxes[1, 4, 2] = -0.1
    assert not T.boxes_ok_ref(boxes, tboxes)


@pytest.mark.parametrize('R,C,n', [(1, 1, 0), (1, 1, 1), (255, 20, 5), (4760, 1, 5), (300, 91, 1)])
def test_focal_reference_is_loss_labels_focal(R, C, n):
    """focal_set_ref == SetCriterion.loss_labels_focal (one-hot, sigmoid_focal_loss, mean(1).sum() / num_boxes * Q)
    in f64, value and gradient."""
    from kinet_amd.models.criterion import SetCriterion
    g = T.gen(R + C + n)
    logits = torch.randn(R, C, generator=g) * 3
    rows = torch.randperm(R, generator=g)[:n]
    cls = torch.randint(0, C, (n,), generator=g)
    num_boxes = 3.0
    loss, tol, grad, tol_g = T.focal_set_ref(logits, rows, cls, num_boxes)
    crit = SetCriterion(C, None, {}, 0.1, ['labels'], True, T.ALPHA, T.GAMMA, False, False)
    x = logits.double().view(1, R, C).requires_grad_(True)
    want = crit.loss_labels_focal({'pred_logits': x}, [{'labels': cls}],
                                  [(rows, torch.arange(n))], num_boxes, log=False)['loss_ce']
    want.backward()
    assert abs(float(want.detach()) - float(loss)) <= 1e-12 * max(1.0, abs(float(want.detach())))
    assert (x.grad[0] - grad).abs().max() <= 1e-12
    assert float(tol) > 0 and float(tol) < 1e-3 * max(float(loss), 1e-3)
    assert (tol_g > 0).all()


def test_focal_reference_extremes_are_finite():
    logits = torch.tensor([[100.0, -100.0], [-100.0, 100.0]])
    loss, tol, grad, _ = T.focal_set_ref(logits, torch.tensor([0, 1]), torch.tensor([1, 1]), 1.0)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    # (0, 1): a positive at -100 -> alpha * 100; (0, 0): a negative at +100 -> (1 - alpha) * 100
    assert abs(float(loss) - (0.25 * 100 + 0.75 * 100)) < 1e-9


# ------------------------------------------------------------------------- builder
def test_build_two_stage_training():
    from kinet_amd.models import build_model
    from kinet_amd.train import build_two_stage_training
    model, criterion, post = build_two_stage_training(_args())
    assert model.two_stage_training is True and model.transformer.two_stage_training is True
    assert criterion.enc_losses is True
    base = {'loss_ce', 'loss_bbox', 'loss_giou'}
    assert set(criterion.weight_dict) == {k + s for k in base for s in T.TRAIN_SETS}
    for k in base:
        assert criterion.weight_dict[k + '_enc'] == criterion.weight_dict[k]
    plain, plain_crit, _ = build_model(_args())
    assert plain.two_stage_training is False and plain_crit.enc_losses is False
    assert set(plain_crit.weight_dict) == {k + s for k in base for s in ('', '_0')}
    assert [k for k, _ in plain.state_dict().items()] == [k for k, _ in model.state_dict().items()]
    with pytest.raises(NotImplementedError, match='inference'):
        plain(torch.zeros(1, 3, 64, 64))                                   # autograd enabled, no flag


def test_builder_refusals():
    from kinet_amd.models import build_model
    from kinet_amd.models.config import load_args
    from kinet_amd.train import build_two_stage_training
    with pytest.raises(NotImplementedError, match='with_box_refine'):
        build_two_stage_training(_args(with_box_refine=False))
    with pytest.raises(ValueError, match='two_stage'):
        build_two_stage_training(load_args('train_deformable'))
    model, _, _ = build_model(_args(with_box_refine=False))
    with pytest.raises(NotImplementedError, match='with_box_refine'):
        model.two_stage_training = True


def test_fixture_keys_are_the_models(golden_dir):
    from kinet_amd.train import build_two_stage_training
    model, _, _ = build_two_stage_training(_args())
    want = [(k, tuple(int(x) for x in s)) for k, *s in
            (ln.split() for ln in open(os.path.join(golden_dir, 'two_stage_train.keys.txt')))]
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == want
    params = dict(model.named_parameters(remove_duplicate=False))
    assert set(T.TRAIN_GRADS) <= set(params)
    d = np.load(os.path.join(golden_dir, 'two_stage_train.npz'))
    assert {k.split(':', 1)[1] for k in d.files if k.startswith('grad:')} == set(T.TRAIN_GRADS)
    assert set(T.loss_keys()) <= set(d.files)
    enc_rows = [set(d[f'rows_enc:{b}'].tolist()) for b in range(2)]
    assert any(r - set(d['topk'][b].tolist()) for b, r in enumerate(enc_rows))          # a row outside the top-k


# ------------------------------------------------------------------------- criterion branch (torch composition)
def _fake_outputs(seed=5, S=97, Q=7, C=4):
    g = T.gen(seed)

    def one(n):
        return {'pred_logits': torch.randn(2, n, C, generator=g),
                'pred_boxes': torch.cat([torch.rand(2, n, 2, generator=g) * 0.6 + 0.2,
                                         torch.rand(2, n, 2, generator=g) * 0.3 + 0.05], -1)}
    out = one(Q)
    out['aux_outputs'] = [one(Q)]
    out['enc_outputs'] = one(S)
    targets = [{'labels': torch.tensor([2, 1, 3]), 'boxes': torch.rand(3, 4, generator=g) * 0.3 + 0.2},
               {'labels': torch.tensor([1, 2]), 'boxes': torch.rand(2, 4, generator=g) * 0.3 + 0.2}]
    return out, targets


def test_enc_branch_on_cpu_equals_the_reference_recipe():
    """detr.py:870-886 spelled out with the criterion's own methods: class-0 copies, the matcher on the
    enc set alone, labels (log=False) / boxes / cardinality, `_enc` keys; the other sets are untouched."""
    from kinet_amd.models.criterion import build_criterion
    from kinet_amd.models.matcher import build_matcher
    args = _args()
    with_enc = build_criterion(args, 4, build_matcher(args), enc_losses=True)
    without = build_criterion(args, 4, build_matcher(args))
    out, targets = _fake_outputs()
    got = with_enc(out, targets)
    base = without(out, targets)
    assert set(got) == set(base) | {'loss_ce_enc', 'loss_bbox_enc', 'loss_giou_enc', 'cardinality_error_enc'}
    for k, v in base.items():
        assert torch.equal(got[k], v), k
    bin_targets = [dict(t, labels=torch.zeros_like(t['labels'])) for t in targets]
    idx = without.matcher(out['enc_outputs'], bin_targets)
    nb = without.num_boxes(out, targets)
    want = {}
    for loss in ('labels', 'boxes', 'cardinality'):
        kw = {'log': False} if loss == 'labels' else {}
        want.update({k + '_enc': v for k, v in without.get_loss(loss, out['enc_outputs'], bin_targets, idx, nb, **kw).items()})
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    assert targets[0]['labels'].tolist() == [2, 1, 3]                       # the caller's targets keep their labels


def test_match_many_extra_set_shares_the_host_copy():
    from kinet_amd.models import training as TR
    from kinet_amd.models.matcher import HungarianMatcher
    out, targets = _fake_outputs()
    m = HungarianMatcher(2.0, 5.0, 2.0, focal_loss=True)
    main = {k: out[k] for k in ('pred_logits', 'pred_boxes')}
    bin_targets = [dict(t, labels=torch.zeros_like(t['labels'])) for t in targets]
    res = m.match_many([main, out['aux_outputs'][0]], targets, extra=(out['enc_outputs'], bin_targets, False))
    assert len(res) == 3
    alone = m(out['enc_outputs'], bin_targets)
    for (a, b), (c, d) in zip(res[2], alone):
        assert torch.equal(a, c) and torch.equal(b, d)
    for got, want in zip(res[:2], m.match_many([main, out['aux_outputs'][0]], targets)):
        for (a, b), (c, d) in zip(got, want):
            assert torch.equal(a, c) and torch.equal(b, d)
    assert TR.GLUE['on'] is False


# ------------------------------------------------------------------------- C ABI
def test_criterion_entry_points_validate_arguments():
    """include/kinet_criterion.h: KINET_ERR_ARG and a message before touching the device."""
    from kinet_amd import _native
    L = _native.lib()
    fake = 4096   # never dereferenced: every call below fails validation first (or launches nothing)

    def err(rc):
        assert rc != 0
        return L.kinet_last_error().decode()

    def cost(logits=fake, boxes=fake, labels=fake, tboxes=fake, start=fake, out=fake, ok=None, B=2, Q=10, C=3, T_=4,
             gamma=2.0):
        return L.kinet_match_cost_focal(logits, boxes, labels, tboxes, start, out, ok, B, Q, C, T_, 2.0, 5.0, 2.0, 0.25,
                                        gamma, None)
    assert cost(T_=0) == 0                                                 # no targets: no launch, status 0
    assert 'bad sizes' in err(cost(B=0))
    assert 'bad sizes' in err(cost(C=0))
    assert 'bad sizes' in err(cost(T_=-1))
    assert 'gamma' in err(cost(gamma=-1.0))
    assert 'null pointer' in err(cost(logits=None))
    assert 'null pointer' in err(cost(start=None))
    assert '16-byte aligned' in err(cost(boxes=fake + 4))
    assert '16-byte aligned' in err(cost(tboxes=fake + 8))

    assert L.kinet_focal_set_loss_workspace(4760, 91) == T.focal_blocks(4760 * 91)[0]
    assert L.kinet_focal_set_loss_workspace(1, 1) == 1
    assert L.kinet_focal_set_loss_workspace(10 ** 7, 91) == T.focal_blocks(10 ** 7 * 91)[0] <= 1024

    def fwd(logits=fake, rows=fake, cls=fake, loss=fake, R=10, C=3, n=2, gamma=2.0, inv=0.5, ws=fake):
        return L.kinet_focal_set_loss(logits, rows, cls, loss, R, C, n, 0.25, gamma, inv, ws, None)
    assert 'bad sizes' in err(fwd(C=0))
    assert 'bad sizes' in err(fwd(n=-1))
    assert 'gamma' in err(fwd(gamma=-0.5))
    assert 'num_boxes' in err(fwd(inv=0.0))
    assert 'positives' in err(fwd(rows=None))
    assert '16-byte aligned' in err(fwd(logits=fake + 4))
    assert 'null pointer' in err(fwd(loss=None))
    assert 'null pointer' in err(fwd(ws=None))

    def bwd(logits=fake, rows=fake, cls=fake, dloss=fake, dlogits=fake, R=10, C=3, n=2):
        return L.kinet_focal_set_loss_backward(logits, rows, cls, dloss, dlogits, R, C, n, 0.25, 2.0, 0.5, None)
    assert bwd(R=0) == 0
    assert 'positives' in err(bwd(cls=None))
    assert 'dlogits' in err(bwd(dlogits=None))
    assert 'dlogits' in err(bwd(dlogits=fake + 4))

    assert L.kinet_two_stage_mask_rows(fake, fake, fake, 0, 256, None) == 0
    assert 'multiple of 4' in err(L.kinet_two_stage_mask_rows(fake, fake, fake, 10, 258, None))
    assert 'null pointer' in err(L.kinet_two_stage_mask_rows(fake, None, fake, 10, 256, None))
    assert '16-byte aligned' in err(L.kinet_two_stage_mask_rows(fake + 4, fake, fake, 10, 256, None))
    assert 'both input gradients' in err(L.kinet_two_stage_boxes_backward(None, None, fake, fake, 10, None))
    assert 'null pointer' in err(L.kinet_two_stage_boxes_backward(fake, None, None, fake, 10, None))
    assert 'null pointer' in err(L.kinet_two_stage_boxes_backward(fake, fake, fake, None, 10, None))
    assert '16-byte aligned' in err(L.kinet_two_stage_boxes_backward(fake, fake + 8, fake, fake, 10, None))


def test_wrappers_refuse_cpu_tensors():
    from kinet_amd import autograd as A
    from kinet_amd import kernels as K
    z = torch.zeros(2, 8, 4)
    i64 = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='GPU only'):
        K.match_cost_focal(z, z, i64, torch.zeros(1, 4), torch.zeros(3, dtype=torch.int32), 2, 5, 2)
    with pytest.raises(RuntimeError, match='GPU only'):
        K.focal_set_loss(torch.zeros(8, 4), i64, i64, 1.0)
    with pytest.raises(RuntimeError, match='GPU only'):
        K.focal_set_loss_backward(torch.zeros(8, 4), i64, i64, torch.ones(1), 1.0)
    with pytest.raises(RuntimeError, match='GPU only'):
        K.two_stage_mask_rows(z, torch.ones(2, 8, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='GPU only'):
        K.two_stage_boxes_backward(z, None, z)
    with pytest.raises(RuntimeError, match='GPU only'):
        A.focal_set_loss(torch.zeros(8, 4, requires_grad=True), i64, i64, 1.0)
