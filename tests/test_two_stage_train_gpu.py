"""Two-stage Deformable DETR training on the GPU (kinet_amd.train.build_two_stage_training): one training
step against the reference's (tests/golden/two_stage_train.npz, made by make_golden_two_stage_train.py:
losses, selections, matched pairs and gradients of the reference model with its enc_outputs losses), the
fused enc_outputs kernels against the torch composition they replace, the criterion's host synchronisations,
a few optimisation steps, and the inference path after training.  fp32, dropout 0, exact f32 matmuls
('highest') where a gate applies, as tests/test_segm_train_gpu.py.

The queries of a two-stage model are its selected proposals in score order, and inside the selected set the
reference's adjacent scores come as close as 1e-6 (tests/test_two_stage_gpu.py), so the selected SET is
compared with the fixture's and the matched rows of the final and auxiliary sets are compared as the
PROPOSALS they select (topk[row]), not as positions in the order."""
import math
import os

import numpy as np
import pytest
import torch

import two_stage_train_refs as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'two_stage_train.npz'))


@pytest.fixture
def highest():
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision('highest')
    yield
    torch.set_float32_matmul_precision(prev)


def _args():
    from kinet_amd.models.config import load_args
    return load_args('train_deformable', device='cuda', **T.TRAIN_OVER)


def build(golden_dir, seed, training=True):
    from weights import make_state_dict
    from kinet_amd.models import build_model
    from kinet_amd.train import build_two_stage_training
    args = _args()
    model, criterion, _ = (build_two_stage_training if training else build_model)(args)
    shapes = {k: [int(x) for x in s] for k, *s in
              (ln.split() for ln in open(os.path.join(golden_dir, 'two_stage_train.keys.txt')))}
    model.load_state_dict(make_state_dict(shapes, seed=seed))
    return args, model.cuda().train(), criterion.cuda()


def batch():
    from kinet_amd.models import nested_tensor_from_tensor_list
    samples = nested_tensor_from_tensor_list([f.cuda() for f in T.train_frames()])
    targets = [{k: v.cuda() for k, v in t.items()} for t in T.train_targets()]
    return samples, targets


def forward(model):
    samples, targets = batch()
    model.zero_grad(set_to_none=True)
    out, targets, *_ = model(samples, targets)
    return out, targets


@pytest.fixture(scope='module')
def stepped(golden_dir, fixture):
    """One forward -> criterion -> backward of the fixture's model in exact f32, shared by the tests that
    only read it: (args, model, criterion, out, targets, losses, total, matched indices, topk)."""
    from kinet_amd.train import weighted_loss
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision('highest')
    try:
        args, model, criterion = build(golden_dir, int(fixture['seed']))
        out, targets = forward(model)
        out['enc_outputs']['pred_logits'].retain_grad()
        seen = {}
        match = criterion.match

        def spy(*a, **kw):
            seen['indices'] = match(*a, **kw)
            return seen['indices']
        criterion.match = spy
        try:
            losses = criterion(out, targets)
        finally:
            del criterion.match
        total = weighted_loss(losses, criterion.weight_dict)
        total.backward(retain_graph=True)
        torch.cuda.synchronize()
        return dict(args=args, model=model, criterion=criterion, out=out, targets=targets, losses=losses, total=total,
                    indices=seen['indices'], topk=model.transformer.topk_proposals.clone())
    finally:
        torch.set_float32_matmul_precision(prev)


def test_training_step_matches_reference(fixture, stepped):
    """Losses and the total to rtol 1e-3 (atol 1e-4), gradients to 2e-3 max|ref| + 1e-5 (5e-3 for the backbone
    weight): the gates of tests/test_train_gpu.py, through tests/segm_train_refs.py."""
    d, s = fixture, stepped
    out, losses, topk = s['out'], s['losses'], s['topk'].cpu()
    assert tuple(out['enc_outputs']['pred_logits'].shape) == (2, T.TRAIN_S, 91)
    assert tuple(out['pred_logits'].shape) == (2, T.TRAIN_K, 91) and len(out['aux_outputs']) == 1
    scores = out['enc_outputs']['pred_logits'].detach()[..., 0]
    assert torch.equal(s['topk'], torch.sort(scores, dim=1, descending=True, stable=True)[1][:, :T.TRAIN_K])
    ref_topk = torch.from_numpy(d['topk'])
    for b in range(2):
        assert set(topk[b].tolist()) == set(ref_topk[b].tolist()), f'frame {b}: selected set differs'
    print(f'[two_stage_train] selection order equals the reference\'s: {torch.equal(topk, ref_topk)}')
    assert set(losses) == set(T.loss_keys())
    for k, v in losses.items():
        want = float(d[k])
        print(f'[loss] {k}: {v.item():.7g} ref {want:.7g} diff {abs(v.item() - want):.2e}')
        np.testing.assert_allclose(v.item(), want, rtol=1e-3, atol=1e-4, err_msg=k)
    np.testing.assert_allclose(s['total'].item(), float(d['loss_total']), rtol=1e-3)
    # matched pairs: final, auxiliary (as proposals), enc_outputs (as rows)
    for n_set, name in enumerate(T.TRAIN_SETS):
        for b in range(2):
            rows, cols = (t.cpu() for t in s['indices'][n_set][b])
            ref_rows, ref_cols = torch.from_numpy(d[f'rows{name}:{b}']), torch.from_numpy(d[f'cols{name}:{b}'])
            if name != '_enc':
                rows, ref_rows = topk[b][rows], ref_topk[b][ref_rows]
            got = sorted(zip(rows.tolist(), cols.tolist()))
            want = sorted(zip(ref_rows.tolist(), ref_cols.tolist()))
            assert got == want, (name, b, got, want)
    params = dict(s['model'].named_parameters(remove_duplicate=False))
    bad = []
    for n in T.TRAIN_GRADS:
        g = params[n].grad
        assert g is not None, n
        ref = torch.from_numpy(d[f'grad:{n}'])
        peak = ref.abs().max().item()
        err = (T.lattice(g).cpu() - ref).abs().max().item()
        gate = T.grad_gate(n, peak)
        # the whole tensor through its L2 norm: | ||g|| - ||ref|| | <= ||g - ref|| <= sqrt(numel) * the element gate
        norm_err = abs(g.double().norm().item() - float(d[f'norm:{n}']))
        print(f'[grad] {n}: max err {err:.3e} rel {err / peak:.3e} (reference f32-vs-f64 {float(d[f"err64:{n}"]):.2e}), '
              f'norm err {norm_err:.3e} of {float(d[f"norm:{n}"]):.3e}')
        if err > gate or norm_err > math.sqrt(g.numel()) * gate:
            bad.append((n, err, gate, norm_err))
    assert not bad, bad


def test_fused_enc_set_against_the_torch_composition(stepped, highest):
    """The same criterion on the same outputs with the kernels switched off (criterion.FUSED_ENC_COST /
    FUSED_ENC_LOSS): equal indices for every set; every loss but loss_ce_enc bit-equal (same methods, same
    indices).  loss_ce_enc and its gradient w.r.t. the enc logits lie within the direct tests' bounds of the
    f64 value of the same logits (tests/two_stage_train_refs.focal_set_ref), and the two paths differ by at most
    that bound plus the composition's own: for the loss as much again (it rounds every element as often and
    torch's tree sum is no deeper than the counted chain); for the gradient autograd's chain through sigmoid,
    BCE and the power has about 40 roundings (40 u |g|), and the composition forms 1 - p_t by subtraction, an
    absolute u on a factor in [0, 1]: through alpha_t ce (1 - p_t)^2 that is at most
    u (2 |ce'| (1 - p_t) + 2 ce p q) <= u (2 + ce / 2) per unit of upstream gradient, ce <= |x| + 1 -- an
    absolute term that dominates where the gradient itself is tiny (p ~ 1e-6), which the kernel, forming q
    directly, does not have."""
    from kinet_amd.models import criterion as CR
    s = stepped
    crit, out, targets = s['criterion'], s['out'], s['targets']
    enc_logits = out['enc_outputs']['pred_logits']
    fused_ce = s['losses']['loss_ce_enc']
    fused_grad, = torch.autograd.grad(fused_ce, enc_logits, retain_graph=True)
    seen = {}
    match = crit.match

    def spy(*a, **kw):
        seen['indices'] = match(*a, **kw)
        return seen['indices']
    CR.FUSED_ENC_COST = CR.FUSED_ENC_LOSS = False
    crit.match = spy
    try:
        losses = crit(out, targets)
    finally:
        CR.FUSED_ENC_COST = CR.FUSED_ENC_LOSS = True
        del crit.match
    comp_grad, = torch.autograd.grad(losses['loss_ce_enc'], enc_logits, retain_graph=True)
    torch.cuda.synchronize()
    for a, b in zip(seen['indices'], s['indices']):
        for (r0, c0), (r1, c1) in zip(a, b):
            assert torch.equal(r0, r1) and torch.equal(c0, c1)
    rows = torch.cat([r + b * T.TRAIN_S for b, (r, _) in enumerate(s['indices'][-1])]).cpu()
    cls = torch.zeros(rows.numel(), dtype=torch.long)
    nb = crit.num_boxes(out, targets)
    ref, tol, gref, gtol = T.focal_set_ref(enc_logits.detach().cpu().view(-1, 91), rows, cls, nb)
    e_f, e_c = abs(fused_ce.item() - ref.item()), abs(losses['loss_ce_enc'].item() - ref.item())
    print(f'[enc] loss_ce_enc {ref.item():.6g}: fused err {e_f:.3e}, composition err {e_c:.3e}, bound {tol.item():.3e}; '
          f'gradient: fused vs composition {(fused_grad - comp_grad).abs().max().item():.3e}')
    assert e_f <= tol.item()
    assert abs(fused_ce.item() - losses['loss_ce_enc'].item()) <= 2 * tol.item()
    assert ((fused_grad.cpu().double().view(-1, 91) - gref).abs() <= gtol).all()
    x = enc_logits.detach().cpu().double().view(-1, 91)
    comp_tol = T.SLACK * T.U32 * (40 * gref.abs() + (2 + 0.5 * (x.abs() + 1)) / nb)
    worst = ((fused_grad - comp_grad).cpu().double().view(-1, 91).abs() / (gtol + comp_tol)).max().item()
    print(f'[enc] gradient: fused vs composition, worst difference / bound {worst:.3f}')
    assert worst <= 1
    for k, v in losses.items():
        if k != 'loss_ce_enc':
            assert torch.equal(v, s['losses'][k]), k


def test_criterion_syncs_and_other_sets_unchanged(stepped):
    """One device -> host synchronisation per criterion call, as the one-stage criterion on the same outputs
    (training.GLUE['syncs']); its final and auxiliary losses are bit-equal to that criterion's."""
    from kinet_amd.models import training as TR
    from kinet_amd.models.criterion import build_criterion
    s = stepped
    plain = build_criterion(s['args'], 91, s['criterion'].matcher).cuda()
    assert plain.enc_losses is False and not any(k.endswith('_enc') for k in plain.weight_dict)
    counts = {}
    for name, crit in (('two_stage', s['criterion']), ('plain', plain)):
        TR.GLUE.update(on=True, glue_s=0.0, sync_wait_s=0.0, syncs=0)
        try:
            with torch.no_grad():
                losses = crit(s['out'], s['targets'])
        finally:
            TR.GLUE['on'] = False
        counts[name] = (TR.GLUE['syncs'], losses)
    assert counts['two_stage'][0] == counts['plain'][0] == 1
    assert set(counts['two_stage'][1]) - set(counts['plain'][1]) == {k + '_enc' for k in T.TRAIN_LOSSES[:4]}
    for k, v in counts['plain'][1].items():
        assert torch.equal(v, counts['two_stage'][1][k]) and torch.equal(v, s['losses'][k].detach()), k


def test_train_steps_and_inference_after_training(golden_dir, fixture):
    """Two train_steps ('high', the training benchmark's setting) with finite losses and gradients on the
    proposal stage; then the eval / no_grad forward is the fast path and equals, bit for bit, that of a plain
    build_model model holding the same weights: training leaves no state behind.  A model without the flag
    still raises in train mode."""
    from kinet_amd.train import build_optimizer, train_step
    args, model, criterion = build(golden_dir, int(fixture['seed']))
    samples, targets = batch()
    model.eval()
    with torch.no_grad():
        before = model(samples)[0]['pred_logits'].clone()
    model.train()
    opt = build_optimizer(model, args)
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision('high')
    try:
        for i in range(2):
            loss, loss_dict = train_step(model, criterion, opt, samples, [dict(t) for t in targets], args.clip_max_norm)
            assert torch.isfinite(loss) and all(torch.isfinite(v).all() for v in loss_dict.values())
            assert set(loss_dict) == set(T.loss_keys())
    finally:
        torch.set_float32_matmul_precision(prev)
    t = model.transformer
    for p in (t.enc_output.weight, t.enc_output.bias, t.enc_output_norm.weight, t.pos_trans.weight, t.pos_trans_norm.bias,
              model.class_embed[2].weight, model.bbox_embed[2].layers[0].weight):
        assert p.grad is not None and torch.isfinite(p.grad).all() and bool(p.grad.abs().max() > 0)
    assert not t.enc_outputs_coord.requires_grad
    model.eval()
    with torch.no_grad():
        after = model(samples)[0]
    assert not torch.equal(before, after['pred_logits'])
    _, plain, _ = build(golden_dir, int(fixture['seed']), training=False)
    plain.load_state_dict(model.state_dict())
    plain.eval()
    assert plain.two_stage_training is False
    with torch.no_grad():
        want = plain(samples)[0]
    for k in ('pred_logits', 'pred_boxes', 'hs_embed'):
        assert torch.equal(after[k], want[k]), k
    for k in ('pred_logits', 'pred_boxes'):
        assert torch.equal(after['enc_outputs'][k], want['enc_outputs'][k]), k
    assert torch.equal(model.transformer.topk_proposals, plain.transformer.topk_proposals)
    with pytest.raises(NotImplementedError, match='inference'):
        plain.train()(samples)
