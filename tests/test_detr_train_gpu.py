"""Vanilla DETR (config 1) training on the GPU: one training step against the reference's
(tests/golden/detr_vanilla_train.npz, made by make_golden_detr_train.py: losses, matched pairs and gradients
of the reference model with its SetCriterion, and a criterion-free step with track queries), which attention
kernels the step runs, a step with the shipped dropout, the tracking model's two-pass step, and the
inference path after training.  fp32, exact f32 matmuls ('highest') where a gate applies.

Gates: tests/detr_train_refs.py -- gradients 2e-3 max|ref| + 1e-5 (5e-3 for a backbone weight), losses 1e-3
relative + 1e-4, each at least 10 x the reference's own f32-vs-f64 difference stored in the fixture (asserted
again here); the reached error is printed beside the gate."""
import math
import os

import numpy as np
import pytest
import torch

import detr_train_refs as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, 'detr_vanilla_train.npz'))


@pytest.fixture
def highest():
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision('highest')
    yield
    torch.set_float32_matmul_precision(prev)


def build(seed, **over):
    from weights import make_state_dict
    from kinet_amd.models import build_model
    from kinet_amd.models.config import load_args
    args = load_args(device='cuda', **dict(T.OVER, **over))
    model, criterion, _ = build_model(args)
    model.load_state_dict(make_state_dict({k: list(v.shape) for k, v in model.state_dict().items()}, seed=seed))
    return args, model.cuda().train(), criterion.cuda()


def batch():
    from kinet_amd.models import nested_tensor_from_tensor_list
    samples = nested_tensor_from_tensor_list([f.cuda() for f in T.frames()])
    targets = [{k: v.cuda() for k, v in t.items()} for t in T.targets()]
    return samples, targets


def spy_match(criterion, seen):
    match = criterion.match

    def spy(*a, **kw):
        seen['indices'] = match(*a, **kw)
        return seen['indices']
    criterion.match = spy


@pytest.fixture(scope='module')
def stepped(fixture):
    """One forward -> criterion -> backward of the fixture's model in exact f32, shared by the tests that only
    read it, with the kinet_mha_train_forward launches the step made."""
    from kinet_amd import kernels as K
    from kinet_amd.train import weighted_loss
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision('highest')
    try:
        args, model, criterion = build(int(fixture['seed']))
        samples, targets = batch()
        model.zero_grad(set_to_none=True)
        calls = K.mha_train_calls()
        out, targets, features, memory, hs = model(samples, targets)
        calls = K.mha_train_calls() - calls
        seen = {}
        spy_match(criterion, seen)
        try:
            losses = criterion(out, targets)
        finally:
            del criterion.match
        total = weighted_loss(losses, criterion.weight_dict)
        total.backward()
        torch.cuda.synchronize()
        return dict(args=args, model=model, criterion=criterion, out=out, losses=losses, total=total, memory=memory,
                    hs=hs, features=features, indices=seen['indices'], calls=calls)
    finally:
        torch.set_float32_matmul_precision(prev)


def _check_grad(bad, tag, name, g, d, key=''):
    ref = torch.from_numpy(d[f'{key}grad:{name}'])
    peak, err64 = ref.abs().max().item(), float(d[f'{key}err64:{name}'])
    gate = T.grad_gate(name, peak)
    assert 10 * err64 < gate, (name, err64, gate)            # the gate is a margin over the reference's own f32
    err = (T.lattice(g).cpu() - ref).abs().max().item()
    # the whole tensor through its L2 norm: | ||g|| - ||ref|| | <= ||g - ref|| <= sqrt(numel) * the element gate
    norm_err = abs(g.double().norm().item() - float(d[f'{key}norm:{name}']))
    print(f'[{tag}] {name}: max err {err:.3e} gate {gate:.3e} (reference f32-vs-f64 {err64:.2e}), norm err '
          f'{norm_err:.3e} of {float(d[f"{key}norm:{name}"]):.3e}')
    if err > gate or norm_err > math.sqrt(g.numel()) * gate:
        bad.append((name, err, gate, norm_err))


def test_training_step_matches_reference(fixture, stepped):
    d, s = fixture, stepped
    out, losses = s['out'], s['losses']
    assert tuple(out['pred_logits'].shape) == (2, 100, 92) and tuple(out['pred_boxes'].shape) == (2, 100, 4)
    assert tuple(out['hs_embed'].shape) == (2, 100, 256) and len(out['aux_outputs']) == 1
    assert tuple(s['memory'].shape) == (2, 256) + T.MAP_HW and tuple(s['hs'].shape) == (2, 2, 100, 256)
    assert int(s['features'][-1].mask[1].sum()) == T.PADDED_KEYS
    assert set(losses) == set(T.loss_keys())
    for k, v in losses.items():
        want, err64 = float(d[k]), float(d[f'err64:{k}'])
        gate = T.LOSS_RTOL * abs(want) + T.LOSS_ATOL
        assert 10 * err64 < gate, (k, err64, gate)
        print(f'[loss] {k}: {v.item():.7g} ref {want:.7g} diff {abs(v.item() - want):.2e} gate {gate:.2e} '
              f'(reference f32-vs-f64 {err64:.2e})')
        assert abs(v.item() - want) <= gate, k
    np.testing.assert_allclose(s['total'].item(), float(d['loss_total']), rtol=T.LOSS_RTOL)
    for n_set, name in enumerate(T.SETS):
        for b in range(2):
            rows, cols = (t.cpu() for t in s['indices'][n_set][b])
            got = sorted(zip(rows.tolist(), cols.tolist()))
            want = sorted(zip(d[f'rows{name}:{b}'].tolist(), d[f'cols{name}:{b}'].tolist()))
            assert got == want, (name, b, got, want)
    params = dict(s['model'].named_parameters())
    bad = []
    for n in T.GRADS:
        assert params[n].grad is not None, n
        _check_grad(bad, 'grad', n, params[n].grad, d)
    assert not bad, bad


def test_track_queries_stay_differentiable(fixture, stepped, highest):
    """The plain DETR with N_TRACK track_query_hs_embeds per frame as leaves: outputs and the gradients
    w.r.t. the embeddings and query_embed against the fixture's criterion-free step."""
    d, model = fixture, stepped['model']
    samples, _ = batch()
    model.zero_grad(set_to_none=True)
    emb = T.track_embeds(256).cuda().requires_grad_(True)
    targets = [{'track_query_hs_embeds': emb[i]} for i in range(emb.shape[0])]
    out, targets, *_ = model(samples, targets)
    assert tuple(out['pred_logits'].shape) == (2, T.N_TRACK + 100, 92)
    assert tuple(targets[0]['track_query_hs_embeds'].shape) == (T.N_TRACK + 100, 256)
    w1, w2 = (w.cuda() for w in T.track_weights(92))
    loss = (out['pred_logits'] * w1).sum() + (out['pred_boxes'] * w2).sum()
    loss.backward()
    qsel = torch.from_numpy(d['track:qsel'])
    for k, key in (('logits', 'pred_logits'), ('boxes', 'pred_boxes')):
        ref, err64 = torch.from_numpy(d[f'track:{k}']), float(d[f'track:err64:{k}'])
        gate = T.LOSS_RTOL * ref.abs().max().item() + T.LOSS_ATOL
        assert 10 * err64 < gate, (k, err64, gate)
        err = (out[key].detach().cpu()[:, qsel] - ref).abs().max().item()
        print(f'[track] {key}: max err {err:.3e} gate {gate:.3e} (reference f32-vs-f64 {err64:.2e})')
        assert err <= gate, key
    bad = []
    _check_grad(bad, 'track', 'track_query_hs_embeds', emb.grad, d, 'track:')
    _check_grad(bad, 'track', 'query_embed.weight', model.query_embed.weight.grad, d, 'track:')
    assert not bad, bad
    model.zero_grad(set_to_none=True)


def test_dense_attention_runs_the_streaming_pair(stepped, monkeypatch):
    """Every attention of the step -- 2 encoder self-, 2 decoder self- and 2 decoder cross-attentions -- went
    through kinet_mha_train_forward; a Deformable DETR decoder self-attention training call still goes through
    kinet_mha_core_dropout / kinet_mha_backward."""
    from kinet_amd import autograd as A
    from kinet_amd import kernels as K
    from kinet_amd.models import build_model
    from kinet_amd.models.config import load_args
    assert stepped['calls'] == 6
    assert all(layer.dense_attn for layer in stepped['model'].transformer.encoder.layers)
    assert all(layer.dense_attn for layer in stepped['model'].transformer.decoder.layers)
    deformable = build_model(load_args('train_deformable', device='cuda', enc_layers=1, dec_layers=1))[0].cuda().train()
    sa = deformable.transformer.decoder.layers[0].self_attn
    assert isinstance(sa, torch.nn.MultiheadAttention) and sa.dropout > 0
    names = []
    call = K.N.call
    monkeypatch.setattr(K.N, 'call', lambda name, *a, **kw: (names.append(name), call(name, *a, **kw))[1])
    x = torch.randn(2, 300, sa.embed_dim, device='cuda', requires_grad=True)
    before = K.mha_train_calls()
    A.multihead_attention(sa, x, x, x).sum().backward()
    torch.cuda.synchronize()
    assert K.mha_train_calls() == before
    assert 'kinet_mha_core_dropout' in names and 'kinet_mha_backward' in names
    assert not any(n.startswith('kinet_mha_train') for n in names)


def test_step_with_the_shipped_dropout_is_finite_complete_and_repeatable(fixture):
    """dropout 0.1 in train mode: finite losses and gradients, a gradient for every parameter that requires
    one, and two steps from the same torch.cuda.manual_seed bit-identical."""
    from kinet_amd.train import weighted_loss
    args, model, criterion = build(int(fixture['seed']), dropout=0.1)
    samples, targets = batch()

    def step():
        torch.cuda.manual_seed(1234)
        model.zero_grad(set_to_none=True)
        out, tg, *_ = model(samples, [dict(t) for t in targets])
        losses = criterion(out, tg)
        weighted_loss(losses, criterion.weight_dict).backward()
        torch.cuda.synchronize()
        return losses, {n: p.grad.clone() for n, p in model.named_parameters() if p.requires_grad}
    losses, grads = step()
    assert all(torch.isfinite(v).all() for v in losses.values())
    missing = [n for n, p in model.named_parameters() if p.requires_grad and p.grad is None]
    assert not missing, missing
    assert all(torch.isfinite(g).all() for g in grads.values())
    losses2, grads2 = step()
    assert all(torch.equal(losses[k], losses2[k]) for k in losses)
    assert all(torch.equal(g, grads2[n]) for n, g in grads.items())


def test_tracking_model_train_step():
    """DETRTracking (tracking: true) in train mode, shipped dropout: one train_step on a synthetic MOT batch;
    the previous-frame pass runs under no_grad in train mode.  The reference's random track-query sampling is
    not reproduced: a smoke test."""
    from kinet_amd.models.detr_tracking import DETRTracking
    from kinet_amd.train import build_optimizer, synthetic_mot_batch, train_step
    torch.manual_seed(0)
    args, model, criterion = build(77, tracking=True, dropout=0.1)
    assert isinstance(model, DETRTracking)
    samples, targets = synthetic_mot_batch(2, 256, 320, torch.device('cuda'), torch.Generator().manual_seed(5), num_boxes=(3, 6))
    opt = build_optimizer(model, args)
    loss, loss_dict = train_step(model, criterion, opt, samples, targets, args.clip_max_norm)
    assert torch.isfinite(loss) and all(torch.isfinite(v).all() for v in loss_dict.values())
    assert 'track_query_hs_embeds' in targets[0]


def test_inference_is_unchanged_by_training(stepped):
    """Eval mode under no_grad is the inference kernel path, bit-identical before and after training calls and
    equal to a fresh build_model model holding the same weights: training leaves no state behind."""
    s = stepped
    model = s['model']
    samples, _ = batch()
    fresh = build(0)[1]
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    model.eval()
    try:
        with torch.no_grad():
            got, want = model(samples)[0], fresh(samples)[0]
        for k in ('pred_logits', 'pred_boxes', 'hs_embed'):
            assert not got[k].requires_grad and torch.equal(got[k], want[k]), k
    finally:
        model.train()
