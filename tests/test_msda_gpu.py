"""GPU parity of the HIP MSDeformAttn operator (through the C-ABI drop-in module) against
the reference's own outputs (tests/golden, generated from ms_deform_attn_core_pytorch)
and the C oracle (oracle/msda_oracle.c, pinned in test_oracle_golden.py).

Tolerances follow the reference op tests: fp32 forward/backward allclose(rtol=1e-2,
atol=1e-3) (ops/test.py:31, :55); the gate requested by BASELINE is 1e-3 abs fp32.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CASES = ['msda_kat_f32.npz', 'msda_kat_f64.npz', 'msda_mid_d32.npz', 'msda_mid_d36.npz']


def _load(golden_dir, name):
    d = dict(np.load(os.path.join(golden_dir, name)))
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    return d, t


def _on_knot(d):
    from test_oracle_golden import _on_knot as k
    return k(d)


@pytest.fixture(scope='module')
def MSDA():
    import kinet_amd  # noqa: F401
    import MultiScaleDeformableAttention as M
    assert M.__file__.endswith('kinet_amd/MultiScaleDeformableAttention.py')
    return M


@pytest.mark.parametrize('name', CASES)
def test_forward_matches_reference(MSDA, golden_dir, name):
    d, t = _load(golden_dir, name)
    out = MSDA.ms_deform_attn_forward(t['value'], t['shapes'], t['loc'], t['attw'], 2)
    torch.cuda.synchronize()
    ref = d['out']
    atol = 1e-10 if ref.dtype == np.float64 else 1e-5
    np.testing.assert_allclose(out.cpu().numpy(), ref, atol=atol, rtol=1e-4)


@pytest.mark.parametrize('name', CASES)
def test_backward_matches_reference(MSDA, golden_dir, name):
    from oracle import msda_oracle
    d, t = _load(golden_dir, name)
    go = d.get('grad_out')
    if go is None:
        go = np.sign(d['out'])
    gv, gl, ga = MSDA.ms_deform_attn_backward(t['value'], t['shapes'], t['loc'], t['attw'],
                                              torch.from_numpy(go).cuda(), 2)
    torch.cuda.synchronize()
    f64 = d['value'].dtype == np.float64
    atol = 1e-10 if f64 else 1e-4
    np.testing.assert_allclose(gv.cpu().numpy(), d['grad_value'], atol=atol, rtol=1e-3)
    np.testing.assert_allclose(ga.cpu().numpy(), d['grad_attw'], atol=atol, rtol=1e-3)
    keep = ~_on_knot(d)
    np.testing.assert_allclose(gl.cpu().numpy()[keep], d['grad_loc'][keep], atol=atol * 10, rtol=1e-3)
    # on the derivative knots compare with the C restatement of the CUDA kernel instead
    ogv, ogl, oga = msda_oracle.bwd(d['value'], d['shapes'], d['loc'], d['attw'], go)
    np.testing.assert_allclose(gl.cpu().numpy(), ogl, atol=atol * 10, rtol=1e-3)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_half_value_forward_backward(MSDA, golden_dir, dtype):
    d, t = _load(golden_dir, 'msda_mid_d32.npz')
    v = t['value'].to(dtype)
    out = MSDA.ms_deform_attn_forward(v, t['shapes'], t['loc'], t['attw'], 64)
    assert out.dtype == dtype
    ref = torch.from_numpy(d['out'])
    err = (out.float().cpu() - ref).abs().max().item()
    assert err < 0.05 * ref.abs().max().item(), err
    gv, gl, ga = MSDA.ms_deform_attn_backward(v, t['shapes'], t['loc'], t['attw'], t['grad_out'].to(dtype), 64)
    assert gv.dtype == dtype and gl.dtype == torch.float32
    gref = torch.from_numpy(d['grad_value'])
    assert (gv.float().cpu() - gref).abs().max().item() < 0.05 * gref.abs().max().item()


def test_large_encoder_shape_vs_oracle(MSDA):
    """config-2 level geometry at 1/4 resolution, checked against the C oracle."""
    from oracle import msda_oracle
    g = torch.Generator().manual_seed(0)
    shapes = torch.tensor([[25, 42], [13, 21], [7, 11], [4, 6]], dtype=torch.int64)
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    N, M, D, L, P, Lq = 2, 8, 32, 4, 4, 300
    value = torch.randn(N, S, M, D, generator=g)
    loc = torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.2 - 0.1
    attw = torch.rand(N, Lq, M, L, P, generator=g)
    attw /= attw.sum((-1, -2), keepdim=True)
    out = MSDA.ms_deform_attn_forward(value.cuda(), shapes.cuda(), loc.cuda(), attw.cuda(), 64).cpu()
    ref = msda_oracle.fwd(value.numpy(), shapes.numpy(), loc.numpy(), attw.numpy())
    np.testing.assert_allclose(out.numpy(), ref, atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize('tune,extra', [((0, 0, 0, 0, 0), 0), ((1, 0, 0, 0, 0), 57), ((1, 6, 32, 256, 0), 57),
                                        ((1, 6, 64, 512, 16), 57), ((1, 10, 512, 512, 64), 0),
                                        ((2, 0, 0, 0, 0), 0), ((0, 0, 0, 0, 0), 57), ((-1, 0, 0, 0, 0), 0),
                                        ((3, 0, 0, 0, 0), 0)])
@pytest.mark.parametrize('D', [32, 36])
def test_backward_list_kernel_vs_oracle(MSDA, tune, extra, D):
    """Encoder-call backward: grad_value rows summed on chip per pass of queries
    (msda_bwd_list_kernel; automatic when Lq == S -- queries walked in 8-pixel-wide blocks of
    each level -- forced by tune mode 1, index order by mode 2, four samples' loads in flight by
    mode 3).  Encoder-like
    queries (raster-ordered pixel centres + grid offsets, heavy row reuse) plus `extra` random
    ones; hash sizes from automatic down to 64 rows (most corners overflow to the direct
    global add), passes of 16-64 queries, and the one-atomic-per-corner kernel (mode -1 and
    the automatic choice for Lq != S), all against the C oracle."""
    from oracle import msda_oracle
    from kinet_amd import _native
    g = torch.Generator().manual_seed(D)
    shapes = torch.tensor([[20, 33], [10, 17], [5, 9], [3, 5]], dtype=torch.int64)
    S = int((shapes[:, 0] * shapes[:, 1]).sum())
    N, M, L, P = 2, 8, 4, 4
    refs = []
    for h, w in shapes.tolist():
        y, x = torch.meshgrid(torch.arange(h) + 0.5, torch.arange(w) + 0.5, indexing='ij')
        refs.append(torch.stack([x.reshape(-1) / w, y.reshape(-1) / h], -1))
    ref = torch.cat([torch.cat(refs), torch.rand(extra, 2, generator=g)])
    Lq = ref.shape[0]
    th = torch.arange(M) * (2 * np.pi / M)
    grid = torch.stack([th.cos(), th.sin()], -1)[:, None, None, :] * (torch.arange(P) + 1.0)[None, None, :, None]
    wh = shapes.flip(1).float()[None, :, None, :]
    loc = ref[None, :, None, None, None, :] + (grid + 0.7 * torch.randn(N, Lq, M, L, P, 2, generator=g)) / wh
    loc = loc.float().contiguous()
    value = torch.randn(N, S, M, D, generator=g)
    attw = torch.rand(N, Lq, M, L, P, generator=g)
    go = torch.randn(N, Lq, M * D, generator=g)
    lib = _native.lib()
    from kinet_amd import kernels as K
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lib.kinet_msda_backward_tune(*tune)
    try:
        gv, gl, ga = MSDA.ms_deform_attn_backward(value.cuda(), shapes.cuda(), loc.cuda(), attw.cuda(), go.cuda(), 64)
        # the kernel the plan names is the kernel the call launched
        plan = K.msda_launch_plan('backward', N, S, M, D, L, Lq, P, torch.float32, tune=tune, cus=cus)
        assert plan['family'] == K.MSDA_BWD_LAST[lib.kinet_msda_backward_last_kernel()]
        gvh, _, _ = MSDA.ms_deform_attn_backward(value.cuda().bfloat16(), shapes.cuda(), loc.cuda(), attw.cuda(),
                                                 go.cuda().bfloat16(), 64)
        plan = K.msda_launch_plan('backward', N, S, M, D, L, Lq, P, torch.bfloat16, tune=tune, cus=cus)
        assert plan['family'] == K.MSDA_BWD_LAST[lib.kinet_msda_backward_last_kernel()]
        torch.cuda.synchronize()
    finally:
        lib.kinet_msda_backward_tune(0, 0, 0, 0, 0)
    ogv, ogl, oga = msda_oracle.bwd(value.numpy(), shapes.numpy(), loc.numpy(), attw.numpy(), go.numpy())
    np.testing.assert_allclose(gv.cpu().numpy(), ogv, atol=2e-4, rtol=1e-4)
    np.testing.assert_allclose(gl.cpu().numpy(), ogl, atol=2e-3, rtol=1e-3)
    np.testing.assert_allclose(ga.cpu().numpy(), oga, atol=2e-4, rtol=1e-4)
    # bf16 values: f32 sums of the bf16 grad_output, rounded once to bf16 (8 significant bits)
    ogvh, _, _ = msda_oracle.bwd(value.numpy(), shapes.numpy(), loc.numpy(), attw.numpy(),
                                 go.bfloat16().float().numpy())
    np.testing.assert_allclose(gvh.float().cpu().numpy(), ogvh, atol=1e-3, rtol=8e-3)


def test_errors_like_reference(MSDA, golden_dir):
    d, t = _load(golden_dir, 'msda_kat_f32.npz')
    with pytest.raises(RuntimeError, match='must divide im2col_step'):
        # N=2, step=3 -> min(2,3)=2 divides; use N=2 with step... reference: batch % min(batch, step)
        v = torch.cat([t['value'], t['value'][:1]], 0)
        MSDA.ms_deform_attn_forward(v, t['shapes'], torch.cat([t['loc'], t['loc'][:1]]),
                                    torch.cat([t['attw'], t['attw'][:1]]), 2)
    with pytest.raises(RuntimeError, match='contiguous'):
        nc = t['value'].transpose(0, 1).contiguous().transpose(0, 1)   # same shape, not contiguous
        MSDA.ms_deform_attn_forward(nc, t['shapes'], t['loc'], t['attw'], 2)
    with pytest.raises(RuntimeError):
        MSDA.ms_deform_attn_forward(t['value'].cpu(), t['shapes'], t['loc'], t['attw'], 2)


def test_function_gradcheck_f64(golden_dir):
    """ops/test_double_precision.py:111-119: gradcheck of the Function in fp64."""
    from torch.autograd import gradcheck
    from kinet_amd.msda import MSDeformAttnFunction
    d, t = _load(golden_dir, 'msda_kat_f64.npz')
    # keep locations away from the derivative knots, as gradcheck's finite differences need
    value = t['value'].clone().requires_grad_()
    loc = (t['loc'] * 0.9 + 0.05).clone().requires_grad_()
    attw = t['attw'].clone().requires_grad_()
    assert gradcheck(MSDeformAttnFunction.apply, (value, t['shapes'], loc, attw, 2), eps=1e-6, atol=1e-6)


def test_fused_module_path_matches_reference(golden_dir):
    """MSDeformAttn module (fused softmax/location/sampling kernel) vs the reference module."""
    from weights import randomize
    from kinet_amd.msda import MSDeformAttn
    d, t = _load(golden_dir, 'msda_module.npz')
    mod = randomize(MSDeformAttn(256, 4, 8, 4), seed=5).cuda().eval()
    with torch.no_grad():
        out2 = mod(t['query'], t['ref2'], t['input_flatten'], t['shapes'], t['padding_mask'])
        out4 = mod(t['query'], t['ref4'], t['input_flatten'], t['shapes'], None)
    np.testing.assert_allclose(out2.cpu().numpy(), d['out_ref2_masked'], atol=1e-3, rtol=0)
    np.testing.assert_allclose(out4.cpu().numpy(), d['out_ref4'], atol=1e-3, rtol=0)


# ---- specialised fused kernel (16-bit values, head_dim 32, L*P in {16, 32}) vs the generic one ----

def _fused_inputs(B, shapes, Lq, M, P, ref_dim, noise, seed, dtype=torch.bfloat16, D=32):
    g = torch.Generator().manual_seed(seed)
    L = len(shapes)
    S = sum(h * w for h, w in shapes)
    value = torch.randn(M, B, S, D, generator=g).to(dtype)
    ref = torch.rand(B, Lq, L, ref_dim, generator=g)
    if ref_dim == 4:
        ref[..., 2:] = ref[..., 2:] * 0.5 + 0.05
    off = noise * torch.randn(B, Lq, M * L * P * 2, generator=g)
    logits = torch.randn(B, Lq, M * L * P, generator=g)
    offlog = torch.cat([off, logits], -1)
    qmask = torch.rand(B, Lq, generator=g) < 0.1
    ss = torch.tensor(shapes, dtype=torch.int64)
    return [t.cuda() for t in (value, ss, offlog, ref, qmask)]


@pytest.mark.parametrize('shapes,Lq,ref_dim,noise', [
    (((40, 50), (20, 25), (10, 13), (5, 7)), 3000, 2, 3.0),    # encoder-like, samples leave the image
    (((40, 50), (20, 25), (10, 13), (5, 7)), 300, 4, 8.0),     # decoder-like, box references
    (((23, 31), (12, 16), (6, 8), (3, 4), (23, 31), (12, 16), (6, 8), (3, 4)), 517, 2, 2.0),  # 8 levels (2 frames)
])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_fast_fused_kernel_matches_generic(shapes, Lq, ref_dim, noise, dtype):
    """The specialised 16-bit kernel (msda_fused_fast_kernel) against the generic fused kernel
    run in f32 on the same values (exactly representable in f32): locations and attention
    weights to a few ulp, outputs within one 16-bit output rounding plus the f16 tap-weight
    quantisation (2^-11 relative per weight)."""
    from kinet_amd import kernels as K
    B, M, P = 2, 8, 4
    value, ss, offlog, ref, qmask = _fused_inputs(B, shapes, Lq, M, P, ref_dim, noise, Lq, dtype)
    L = len(shapes)
    out_f, loc_f, aw_f = K.msda_fused(value, ss, offlog, ref, M, L, P, qmask, want_loc_attw=True, head_major=True)
    out_g, loc_g, aw_g = K.msda_fused(value.float(), ss, offlog, ref, M, L, P, qmask, want_loc_attw=True,
                                      head_major=True)
    torch.cuda.synchronize()
    # reciprocal-multiply normalisation / approximate reciprocal in the softmax: a few ulp
    assert torch.allclose(loc_f, loc_g, rtol=1e-6, atol=1e-6)
    assert torch.allclose(aw_f, aw_g, rtol=1e-5, atol=1e-7)
    d = (out_f.float() - out_g.float()).abs()
    tol = out_g.float().abs() * 2.0 ** -7 + 1e-3
    assert (d <= tol).all(), d.max().item()
    assert (out_f.float()[qmask] == 0).all()


@pytest.mark.parametrize('D,dtype', [(32, torch.bfloat16), (36, torch.float16)])
def test_fast_fused_kernel_vs_oracle(D, dtype):
    """The fused kernel against the C oracle (through loc/attw it reports): head_dim 32 on the
    specialised kernel, head_dim 36 (d = 288 of configs 3-5, f16) on the generic one."""
    from kinet_amd import kernels as K
    from oracle import msda_oracle as O
    shapes = ((40, 50), (20, 25), (10, 13), (5, 7))
    B, M, P, Lq = 2, 8, 4, 700
    value, ss, offlog, ref, qmask = _fused_inputs(B, shapes, Lq, M, P, 2, 3.0, 5, dtype=dtype, D=D)
    out, loc, aw = K.msda_fused(value, ss, offlog, ref, M, 4, P, qmask, want_loc_attw=True, head_major=True)
    torch.cuda.synchronize()
    v = value.float().permute(1, 2, 0, 3).contiguous().cpu().numpy()          # (B, S, M, D)
    ref_out = O.fwd(v, ss.cpu().numpy(), loc.cpu().numpy(), aw.cpu().numpy())
    d = (out.float().cpu() - torch.from_numpy(ref_out).reshape(out.shape)).abs()
    assert (d <= 1e-2 * torch.from_numpy(ref_out).reshape(out.shape).abs() + 1e-2).all(), d.max().item()


def test_fast_fused_f16_values_bf16_out():
    """f16 values (v_fma_mix path) with bf16 output vs the same values sampled into f16 output:
    identical f32 accumulation, so they differ by the output rounding only."""
    from kinet_amd import kernels as K
    shapes = ((40, 50), (20, 25), (10, 13), (5, 7))
    B, M, P, Lq = 2, 8, 4, 1500
    value, ss, offlog, ref, qmask = _fused_inputs(B, shapes, Lq, M, P, 2, 3.0, 9, dtype=torch.float16)
    o_bf = K.msda_fused(value, ss, offlog, ref, M, 4, P, qmask, head_major=True, out_dtype=torch.bfloat16)
    o_h = K.msda_fused(value, ss, offlog, ref, M, 4, P, qmask, head_major=True)
    torch.cuda.synchronize()
    assert o_bf.dtype == torch.bfloat16 and o_h.dtype == torch.float16
    d = (o_bf.float() - o_h.float()).abs()
    assert (d <= o_h.float().abs() * 2.0 ** -8 + 1e-6).all(), d.max().item()
    with pytest.raises(RuntimeError):
        K.msda_fused(value.float(), ss, offlog, ref, M, 4, P, head_major=True, out_dtype=torch.bfloat16)


def test_fast_fused_f16_offsets_logits():
    """f16 offsets/logits (bf16 compute path) vs the same values in f32: sampling locations
    differ only by the f16 rounding of the offsets."""
    from kinet_amd import kernels as K
    shapes = ((40, 50), (20, 25), (10, 13), (5, 7))
    B, M, P, Lq = 2, 8, 4, 1500
    value, ss, offlog, ref, qmask = _fused_inputs(B, shapes, Lq, M, P, 2, 3.0, 13, dtype=torch.float16)
    oh = offlog.half()
    o32, loc32, aw32 = K.msda_fused(value, ss, oh.float(), ref, M, 4, P, qmask, want_loc_attw=True, head_major=True,
                                    out_dtype=torch.bfloat16)
    o16, loc16, aw16 = K.msda_fused(value, ss, oh, ref, M, 4, P, qmask, want_loc_attw=True, head_major=True,
                                    out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    # identical input values (the f32 tensor holds the f16 values exactly): the two
    # instantiations agree up to instruction selection (fma contraction)
    torch.testing.assert_close(loc16, loc32, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(aw16, aw32, rtol=1e-5, atol=1e-7)
    d = (o16.float() - o32.float()).abs()
    assert (d <= o32.float().abs() * 2.0 ** -7 + 1e-4).all(), d.max().item()


def test_fast_fused_query_tile_order_invariant():
    """The encoder's tile processing order (kinet_amd.kernels.encoder_tile_order) changes only
    WHEN each 16-query tile runs: every output / loc / attw is bit-identical to natural order."""
    from kinet_amd import kernels as K
    shapes = ((40, 50), (20, 25), (10, 13), (5, 7))
    B, M, P = 2, 8, 4
    Lq = sum(h * w for h, w in shapes)
    value, ss, offlog, ref, qmask = _fused_inputs(B, shapes, Lq, M, P, 2, 3.0, 21, dtype=torch.float16)
    order = K.encoder_tile_order(shapes, value.device)
    assert sorted(order.tolist()) == list(range((Lq + 15) // 16)) and order.tolist() != sorted(order.tolist())
    o0, l0, a0 = K.msda_fused(value, ss, offlog.half(), ref, M, 4, P, qmask, want_loc_attw=True, head_major=True,
                              out_dtype=torch.bfloat16)
    o1, l1, a1 = K.msda_fused(value, ss, offlog.half(), ref, M, 4, P, qmask, want_loc_attw=True, head_major=True,
                              out_dtype=torch.bfloat16, query_tile_order=order)
    torch.cuda.synchronize()
    assert torch.equal(o0, o1) and torch.equal(l0, l1) and torch.equal(a0, a1)


# ---- encoder kernel, head-major offsets / logits (msda_enc.hip, kinet_msda_encoder_forward) ----

def _hm(offlog, M, L=4, P=4):
    """(B, Lq, M*L*P*3) [offsets | logits] -> (M, B, Lq, L*P*3) per-head [offsets | logits], f16."""
    B, Lq, _ = offlog.shape
    off = offlog[..., :M * L * P * 2].reshape(B, Lq, M, L * P * 2)
    lg = offlog[..., M * L * P * 2:].reshape(B, Lq, M, L * P)
    return torch.cat([off, lg], -1).permute(2, 0, 1, 3).contiguous().half()


@pytest.mark.parametrize('shapes,ref_dim,noise', [
    (((64, 84), (32, 42), (16, 21), (8, 11)), 2, 3.0),       # levels 2-3 staged (as at 800x1333)
    (((64, 84), (32, 42), (16, 21), (8, 11)), 4, 6.0),       # box references, far-out samples
    (((60, 70), (40, 50), (45, 50), (10, 13)), 2, 2.0),      # level 3 only fits
    (((50, 60), (20, 30), (10, 13), (5, 7)), 2, 1.0),        # levels 1-3 staged
    (((25, 40), (15, 20), (8, 10), (4, 5)), 2, 4.0),         # every level staged (Lq > S)
    (((100, 167), (50, 84), (25, 42), (13, 21)), 2, 2.0),    # the config-2 geometry (800x1333)
])
@pytest.mark.parametrize('out_dtype,masked,ordered', [(torch.bfloat16, False, True), (torch.float16, True, False),
                                                      (torch.float16, True, True)])
def test_encoder_kernel_matches_fast_kernel(shapes, ref_dim, noise, out_dtype, masked, ordered):
    """kinet_msda_encoder_forward against msda_fused_fast_kernel on the same f16
    offsets / logits (row-major for the fast kernel, head-major for the encoder kernel).
    Bound as test_encoder_lds_kernel_matches_fast_kernel (acc16): the tap weights are
    quantised to f16 after f32 location arithmetic that the compiler may contract
    differently (2^-11 max|value|), each level's 16 taps are summed as f16 pairs
    (2^-7 max|value|), plus one rounding of either output."""
    from kinet_amd import kernels as K
    B, M, P = 2, 8, 4
    Lq = max(sum(h * w for h, w in shapes), 2304)
    value, ss, offlog, ref, qmask = _fused_inputs(B, shapes, Lq, M, P, ref_dim, noise, Lq + 7 * ref_dim,
                                                  dtype=torch.float16)
    offlog = offlog.half()
    qm = qmask if masked else None
    # ordered: the encoder's row-sorted tile order (queries = the pixels of the levels)
    S = sum(h * w for h, w in shapes)
    order = K.encoder_tile_order(shapes, value.device) if ordered and Lq == S else None
    o_enc = K.msda_encoder(value, shapes, _hm(offlog, M), ref, M, qm, out_dtype=out_dtype, query_tile_order=order)
    o_fast = K.msda_fused(value, ss, offlog, ref, M, 4, P, qm, head_major=True, out_dtype=out_dtype)
    torch.cuda.synchronize()
    ulp = 2.0 ** -7 if out_dtype == torch.bfloat16 else 2.0 ** -10
    d = (o_enc.float() - o_fast.float()).abs()
    vmax = value.float().abs().max().item()
    big = torch.maximum(o_fast.float().abs(), o_enc.float().abs())
    assert (d <= big * ulp + (2.0 ** -7 + 2.0 ** -11) * vmax).all(), d.max().item()
    assert d.mean().item() <= 2e-3, d.mean().item()
    if masked:
        assert (o_enc.float()[qmask] == 0).all()
    assert torch.isfinite(o_enc.float()).all()


def test_encoder_kernel_vs_oracle():
    """The encoder kernel against the C oracle (cuh:165-237 restated), fed the locations /
    attention weights the fast kernel reports for the same inputs."""
    from kinet_amd import kernels as K
    from oracle import msda_oracle as O
    shapes = ((64, 84), (32, 42), (16, 21), (8, 11))
    B, M, P = 2, 8, 4
    Lq = sum(h * w for h, w in shapes)
    value, ss, offlog, ref, qmask = _fused_inputs(B, shapes, Lq, M, P, 2, 3.0, 78, dtype=torch.float16)
    offlog = offlog.half()
    out = K.msda_encoder(value, shapes, _hm(offlog, M), ref, M, qmask, out_dtype=torch.float16)
    _, loc, aw = K.msda_fused(value, ss, offlog, ref, M, 4, P, qmask, want_loc_attw=True, head_major=True,
                              out_dtype=torch.float16)
    torch.cuda.synchronize()
    v = value.float().permute(1, 2, 0, 3).contiguous().cpu().numpy()
    ref_out = torch.from_numpy(O.fwd(v, ss.cpu().numpy(), loc.cpu().numpy(), aw.cpu().numpy())).reshape(out.shape)
    d = (out.float().cpu() - ref_out).abs()
    bound = 4e-3 * ref_out.abs() + 4e-3 + 2.0 ** -7 * value.float().abs().max().item()
    assert (d <= bound).all(), d.max().item()
    assert d.mean().item() <= 2e-3, d.mean().item()


def test_encoder_kernel_order_and_batch_invariant():
    """Each query's result depends only on its own inputs: tile order, batch size (query
    chunks per head map) and a rerun leave it bit-identical."""
    from kinet_amd import kernels as K
    shapes = ((64, 84), (32, 42), (16, 21), (8, 11))
    M, P = 8, 4
    Lq = sum(h * w for h, w in shapes)
    value, ss, offlog, ref, qmask = _fused_inputs(3, shapes, Lq, M, P, 2, 3.0, 6, dtype=torch.float16)
    hm = _hm(offlog, M)
    order = K.encoder_tile_order(shapes, value.device)
    o_nat = K.msda_encoder(value, shapes, hm, ref, M, out_dtype=torch.bfloat16)
    o_ord = K.msda_encoder(value, shapes, hm, ref, M, out_dtype=torch.bfloat16, query_tile_order=order)
    o_again = K.msda_encoder(value, shapes, hm, ref, M, out_dtype=torch.bfloat16, query_tile_order=order)
    o_one = K.msda_encoder(value[:, 1:2], shapes, hm[:, 1:2], ref[1:2], M, out_dtype=torch.bfloat16,
                           query_tile_order=order)
    torch.cuda.synchronize()
    assert torch.equal(o_nat, o_ord) and torch.equal(o_ord, o_again)
    assert torch.equal(o_one[0], o_ord[1])


def test_encoder_kernel_large_magnitudes():
    """f16 range on the bf16 path (values and offsets are stored f16): values up to 2^14 and
    offsets of thousands of pixels (samples far outside every level) stay finite, match the
    f32-accumulating fast kernel within the stated f16 bounds, and out-of-image samples add 0."""
    from kinet_amd import kernels as K
    shapes = ((64, 84), (32, 42), (16, 21), (8, 11))
    B, M, P = 1, 8, 4
    Lq = sum(h * w for h, w in shapes)
    value, ss, offlog, ref, _ = _fused_inputs(B, shapes, Lq, M, P, 2, 3.0, 99, dtype=torch.float16)
    value = (value.float() * 4096.0).clamp(-16384, 16384).half()
    offlog = offlog.clone()
    offlog[:, : Lq // 2, : M * 32] *= 1000.0          # half the queries sample far outside
    offlog = offlog.half()
    o_enc = K.msda_encoder(value, shapes, _hm(offlog, M), ref, M, out_dtype=torch.bfloat16)
    o_fast = K.msda_fused(value, ss, offlog, ref, M, 4, P, None, head_major=True, out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert torch.isfinite(o_enc.float()).all()
    vmax = value.float().abs().max().item()
    d = (o_enc.float() - o_fast.float()).abs()
    big = torch.maximum(o_fast.float().abs(), o_enc.float().abs())
    assert (d <= big * 2.0 ** -7 + (2.0 ** -7 + 2.0 ** -11) * vmax).all(), d.max().item()


def test_encoder_kernel_rejects_unstaged_geometry():
    """Shapes whose levels do not fit the LDS map even as strips (12 staged rows of a
    250-pixel-wide coarsest level) are refused: msda_encoder_supported is False and the module
    falls back to kinet_msda_fused_forward."""
    from kinet_amd import kernels as K
    shapes = ((20, 250), (20, 250), (20, 250), (20, 250))
    B, M, P = 1, 8, 4
    Lq = sum(h * w for h, w in shapes)
    value, ss, offlog, ref, _ = _fused_inputs(B, shapes, Lq, M, P, 2, 1.0, 3, dtype=torch.float16)
    assert K.msda_encoder_plan(shapes, B, M, Lq) is None
    assert not K.msda_encoder_supported(value, shapes, Lq, M, 4, 4, B)
    with pytest.raises(RuntimeError, match='no strip plan'):
        K.msda_encoder(value, shapes, _hm(offlog, M), ref, M, out_dtype=torch.bfloat16)


def _encoder_refs(shapes, B):
    """The encoder's reference points (deformable_transformer.py:get_reference_points with
    valid ratios 1): query q = pixel (i, j) of its level -> ((j + .5) / W, (i + .5) / H) at
    every level."""
    pts = []
    for h, w in shapes:
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32) + 0.5, torch.arange(w, dtype=torch.float32) + 0.5,
                                indexing='ij')
        pts.append(torch.stack([xx.reshape(-1) / w, yy.reshape(-1) / h], -1))
    r = torch.cat(pts, 0)
    return r[None, :, None, :].expand(B, -1, len(shapes), -1).contiguous().cuda()


@pytest.mark.parametrize('shapes', [
    ((100, 167), (50, 84), (25, 42), (13, 21)),    # config 2 (800x1333): level 0 gathered, 1-3 staged
    ((60, 70), (40, 50), (45, 50), (10, 13)),      # wide level 2: levels 2-3 staged
    ((25, 40), (15, 20), (8, 10), (4, 5)),         # every level staged whole
])
@pytest.mark.parametrize('noise', [0.5, 3.0, 25.0])
def test_encoder_kernel_strips_staged_and_far(shapes, noise):
    """Encoder geometry (queries = the pixels of the levels, references at their centres, tiles
    in row-sorted order): small offsets read the strip's staged rows, large ones (noise 25 px)
    leave them and are gathered from the head map -- both against the fast kernel, within the
    bound of test_encoder_kernel_matches_fast_kernel, and the plan is the expected one."""
    from kinet_amd import kernels as K
    B, M, P = 2, 8, 4
    S = sum(h * w for h, w in shapes)
    value, ss, offlog, _, qmask = _fused_inputs(B, shapes, S, M, P, 2, noise, 11 + int(noise), dtype=torch.float16)
    ref = _encoder_refs(shapes, B)
    # offsets in pixels of each level: the reference's normaliser divides x by H and y by W
    # (ms_deform_attn.py:77-79), so scale the noise back to pixels per level
    offlog = offlog.half()
    plan = K.msda_encoder_plan(shapes, B, M, S)
    assert plan is not None
    if shapes[0] == (100, 167):
        assert plan[0] == 1 and plan[1] >= 8, plan
    order = K.encoder_tile_order(shapes, value.device)
    o_enc = K.msda_encoder(value, shapes, _hm(offlog, M), ref, M, qmask, out_dtype=torch.bfloat16,
                           query_tile_order=order)
    o_nat = K.msda_encoder(value, shapes, _hm(offlog, M), ref, M, qmask, out_dtype=torch.bfloat16)
    o_fast = K.msda_fused(value, ss, offlog, ref, M, 4, P, qmask, head_major=True, out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    # natural order: other strips, other staged rows, same result bit for bit
    assert torch.equal(o_enc, o_nat)
    d = (o_enc.float() - o_fast.float()).abs()
    vmax = value.float().abs().max().item()
    big = torch.maximum(o_fast.float().abs(), o_enc.float().abs())
    assert (d <= big * 2.0 ** -7 + (2.0 ** -7 + 2.0 ** -11) * vmax).all(), d.max().item()
    assert d.mean().item() <= 2e-3, d.mean().item()
    assert (o_enc.float()[qmask] == 0).all()


# ---- head_dim 36: split value planes (kinet_gemm_headmajor_split -> kinet_msda_encoder_forward_split) ----

def _split(value):
    """(M, B, S, 36) -> K.SplitValue planes (M, B, S, 32) + (M, B, S, 4) in one buffer."""
    from kinet_amd import kernels as K
    M_, B, S, _ = value.shape
    buf = torch.empty(M_ * B * S * 36, dtype=value.dtype, device=value.device)
    main = buf[:M_ * B * S * 32].view(M_, B, S, 32)
    tail = buf[M_ * B * S * 32:].view(M_, B, S, 4)
    main.copy_(value[..., :32])
    tail.copy_(value[..., 32:])
    return K.SplitValue(main, tail)


@pytest.mark.parametrize('masked_rows', [False, True])
def test_value_proj_split_matches_headmajor(masked_rows):
    """kinet_gemm_headmajor_split (weight rows reordered [heads x 32 | heads x 4]) writes the same
    numbers as the (M, B, S, 36) head-major projection, bit for bit (same dot products, same
    tile), with padding rows zeroed in both planes."""
    from kinet_amd import kernels as K
    g = torch.Generator().manual_seed(5)
    B, S, d, M = 2, 3100, 288, 8
    x = torch.randn(B, S, d, generator=g).half().cuda()
    w = (torch.randn(d, d, generator=g) / 16).cuda()
    b = torch.randn(d, generator=g).cuda()
    mask = (torch.rand(B, S, generator=g) < 0.2).cuda() if masked_rows else None
    ref = K.value_proj_headmajor(x, w, b, 36, row_mask=mask, out_dtype=torch.float16)
    ws, bs = K.split_value_weights(w, b, M)
    sv = K.value_proj_headmajor_split(x, ws, bs, M, row_mask=mask, out_dtype=torch.float16)
    torch.cuda.synchronize()
    assert sv.shape == (M, B, S, 36)
    assert torch.equal(sv.main, ref[..., :32]) and torch.equal(sv.tail, ref[..., 32:])
    if masked_rows:
        assert (sv.tail.permute(1, 2, 0, 3)[mask] == 0).all()


@pytest.mark.parametrize('shapes,ref_dim,noise', [
    (((64, 84), (32, 42), (16, 21), (8, 11)), 2, 3.0),
    (((64, 84), (32, 42), (16, 21), (8, 11)), 4, 6.0),       # box references, far-out samples
    (((50, 60), (20, 30), (10, 13), (5, 7)), 2, 1.0),        # levels 1-3 staged
    (((25, 40), (15, 20), (8, 10), (4, 5)), 2, 4.0),         # every level staged (Lq > S)
    (((135, 240), (68, 120), (34, 60), (17, 30)), 2, 2.0),   # the config-5 geometry (1080x1920)
])
@pytest.mark.parametrize('out_dtype,masked', [(torch.float16, False), (torch.bfloat16, True)])
def test_encoder_split_kernel_matches_generic(shapes, ref_dim, noise, out_dtype, masked):
    """kinet_msda_encoder_forward_split (head_dim 36 as a 32- + 4-channel plane) against the
    generic fused kernel on the same (M, B, S, 36) f16 values and f16 offsets / logits: the bound of
    test_encoder_kernel_matches_fast_kernel (f16 tap weights, per-level f16 pair sums, one output
    rounding), on the 32 main channels and the 4 tail channels alike."""
    from kinet_amd import kernels as K
    B, M, P = 2, 8, 4
    S = sum(h * w for h, w in shapes)
    Lq = max(S, 2304)
    value, ss, offlog, ref, qmask = _fused_inputs(B, shapes, Lq, M, P, ref_dim, noise, Lq + 5 * ref_dim,
                                                  dtype=torch.float16, D=36)
    offlog = offlog.half()
    qm = qmask if masked else None
    plan = K.msda_encoder_plan(shapes, B, M, Lq, 36)
    assert plan is not None and K.msda_split_supported(torch.float16, 36, shapes, Lq, M, 4, P, B)
    order = K.encoder_tile_order(shapes, value.device) if Lq == S else None
    o_enc = K.msda_encoder_split(_split(value), shapes, _hm(offlog, M), ref, M, qm, out_dtype=out_dtype,
                                 query_tile_order=order)
    # the generic kernel in f32 on the same (f16-exact) values and offsets / logits
    o_gen = K.msda_fused(value.float(), ss, offlog.float(), ref, M, 4, P, qm, head_major=True)
    torch.cuda.synchronize()
    ulp = 2.0 ** -7 if out_dtype == torch.bfloat16 else 2.0 ** -10
    d = (o_enc.float() - o_gen.float()).abs()
    vmax = value.float().abs().max().item()
    big = torch.maximum(o_gen.float().abs(), o_enc.float().abs())
    bad = d > big * ulp + (2.0 ** -7 + 2.0 ** -11) * vmax
    assert not bad.any(), (d.max().item(), int(bad.sum()),
                           [(c, n) for c, n in enumerate(bad.view(B, Lq, M, 36).sum((0, 1, 2)).tolist()) if n])
    assert d.mean().item() <= 2e-3, d.mean().item()
    tail = d.view(B, Lq, M, 36)[..., 32:]
    assert tail.mean().item() <= 2e-3, tail.mean().item()
    if masked:
        assert (o_enc.float()[qmask] == 0).all()
    assert torch.isfinite(o_enc.float()).all()


def test_encoder_split_kernel_vs_oracle():
    """The split kernel against the C oracle (cuh:165-237 restated, any channel count) on the
    locations / attention weights the generic kernel reports for the same inputs."""
    from kinet_amd import kernels as K
    from oracle import msda_oracle as O
    shapes = ((64, 84), (32, 42), (16, 21), (8, 11))
    B, M, P = 2, 8, 4
    Lq = sum(h * w for h, w in shapes)
    value, ss, offlog, ref, qmask = _fused_inputs(B, shapes, Lq, M, P, 2, 3.0, 81, dtype=torch.float16, D=36)
    offlog = offlog.half()
    out = K.msda_encoder_split(_split(value), shapes, _hm(offlog, M), ref, M, qmask, out_dtype=torch.float16)
    _, loc, aw = K.msda_fused(value.float(), ss, offlog.float(), ref, M, 4, P, qmask, want_loc_attw=True,
                              head_major=True)
    torch.cuda.synchronize()
    v = value.float().permute(1, 2, 0, 3).contiguous().cpu().numpy()
    ref_out = torch.from_numpy(O.fwd(v, ss.cpu().numpy(), loc.cpu().numpy(), aw.cpu().numpy())).reshape(out.shape)
    d = (out.float().cpu() - ref_out).abs()
    bound = 4e-3 * ref_out.abs() + 4e-3 + 2.0 ** -7 * value.float().abs().max().item()
    assert (d <= bound).all(), d.max().item()
    assert d.mean().item() <= 2e-3, d.mean().item()


def test_encoder_split_kernel_order_and_batch_invariant():
    """Each query's result depends only on its own inputs (tile order, batch, rerun)."""
    from kinet_amd import kernels as K
    shapes = ((64, 84), (32, 42), (16, 21), (8, 11))
    M, P = 8, 4
    Lq = sum(h * w for h, w in shapes)
    value, ss, offlog, ref, qmask = _fused_inputs(3, shapes, Lq, M, P, 2, 25.0, 9, dtype=torch.float16, D=36)
    hm = _hm(offlog, M)
    sv = _split(value)
    order = K.encoder_tile_order(shapes, value.device)
    o_nat = K.msda_encoder_split(sv, shapes, hm, ref, M, out_dtype=torch.bfloat16)
    o_ord = K.msda_encoder_split(sv, shapes, hm, ref, M, out_dtype=torch.bfloat16, query_tile_order=order)
    o_one = K.msda_encoder_split(_split(value[:, 1:2].contiguous()), shapes, hm[:, 1:2], ref[1:2], M,
                                 out_dtype=torch.bfloat16, query_tile_order=order)
    torch.cuda.synchronize()
    assert torch.equal(o_nat, o_ord)
    assert torch.equal(o_one[0], o_ord[1])


# ---- sampling records (kinet_msda_sample_records -> kinet_msda_encoder_forward_records) ----

def _record_problem(shapes, B, noise, seed, ref_dim=2, masked=False, dtype=torch.bfloat16):
    """Encoder-geometry inputs of the records GEMM: x, pos (B, S, 256), the MSDA projection
    (rows grouped per (head, level) as MSDeformAttn.packed_records_weights), references."""
    g = torch.Generator().manual_seed(seed)
    M, L, P = 8, 4, 4
    S = sum(h * w for h, w in shapes)
    x = torch.randn(B, S, 256, generator=g).to(dtype)
    pos = (0.5 * torch.randn(B, S, 256, generator=g)).to(dtype)
    # offsets ~ noise pixels, logits ~ N(0, 1) (weights scaled so the projections have that spread)
    w_off = torch.randn(M * L * P * 2, 256, generator=g) * noise / 16.0
    w_lg = torch.randn(M * L * P, 256, generator=g) / 16.0
    b_off = torch.randn(M * L * P * 2, generator=g) * noise
    b_lg = torch.randn(M * L * P, generator=g) * 0.5
    if ref_dim == 2:
        ref = _encoder_refs(shapes, B).cpu()
    else:
        ref = torch.rand(B, S, L, 4, generator=g)
        ref[..., 2:] = ref[..., 2:] * 0.5 + 0.05
    qmask = (torch.rand(B, S, generator=g) < 0.1) if masked else None

    def group(a, b):   # (head, level, [8 offsets | 4 logits])
        return torch.cat([a.view(M, L, 2 * P, *a.shape[1:]), b.view(M, L, P, *b.shape[1:])], 2).reshape(
            M * L * 3 * P, *a.shape[1:])
    w = group(w_off, w_lg).to(dtype)
    bias = group(b_off, b_lg).float()
    return x, pos, w, bias, ref, qmask, (w_off, w_lg, b_off, b_lg)


def _host_offlog(x, pos, w_off, w_lg, b_off, b_lg, dtype):
    """The projection in f64 from the operands the GEMM sees (x + pos rounded to the compute
    dtype, bf16 weights), [offsets | logits] as ms_deform_attn.py:68-69."""
    q = (x.float() + pos.float()).to(dtype).double()
    wo, wl = w_off.to(dtype).double(), w_lg.to(dtype).double()
    return torch.cat([q @ wo.T + b_off.double(), q @ wl.T + b_lg.double()], -1)


@pytest.mark.parametrize('shapes', [((100, 167), (50, 84), (25, 42), (13, 21)), ((25, 40), (15, 20), (8, 10), (4, 5))])
@pytest.mark.parametrize('noise,ref_dim,masked', [(2.0, 2, False), (12.0, 2, True), (3.0, 4, False)])
def test_sample_records_vs_oracle(shapes, noise, ref_dim, masked):
    """kinet_msda_sample_records (the GEMM with softmax / locations / bilinear setup in its
    epilogue) against oracle.sample_records of the reference's preparation (ms_deform_attn.py:
    68-82, oracle.prep) on the f64 projection of the same operands.  The GEMM's f32
    accumulation moves a projected value by ~1e-6 relative, which can flip a fraction's last
    fixed-point bit: locations agree within 1 LSB (2^-fb pixel), weights within f16 rounding;
    and the two record sets sample the same values (oracle fwd) within 1e-3."""
    from kinet_amd import kernels as K
    from oracle import msda_oracle as O
    B, M = 2, 8
    x, pos, w, bias, ref, qmask, raw = _record_problem(shapes, B, noise, 41 + int(noise), ref_dim, masked)
    fb = K.msda_record_frac_bits(shapes)
    assert fb == (8 if shapes[0][1] > 128 else 10)
    rec, fb2 = K.msda_sample_records(x.cuda(), w.cuda(), bias.cuda(), M, ref.cuda(), shapes, x_add=pos.cuda(),
                                     query_attn_mask=qmask.cuda() if masked else None)
    torch.cuda.synchronize()
    assert fb2 == fb and rec.shape == (M, B, x.shape[1], 24)
    offlog = _host_offlog(x, pos, *raw, torch.bfloat16)
    loc, aw = O.prep(offlog, ref.double(), shapes, qmask, M, 4, 4)
    exp = O.sample_records(loc, aw, ref, shapes, fb)
    got = rec.cpu()
    l_g, a_g = O.decode_records(got, shapes, fb)
    l_e, a_e = O.decode_records(exp, shapes, fb)
    H = torch.tensor([h for h, _ in shapes], dtype=torch.float64)[None, None, None, :, None]
    W = torch.tensor([w_ for _, w_ in shapes], dtype=torch.float64)[None, None, None, :, None]
    dy = ((l_g[..., 1] - l_e[..., 1]) * H).abs()
    dx = ((l_g[..., 0] - l_e[..., 0]) * W).abs()
    lsb = 2.0 ** -fb
    # where a sample points with weight 0 (outside the level, masked query) is free: the kernel and
    # the oracle both pick the query's own pixel, but an f32 vs f64 product may floor to the next one
    live = (a_e != 0) | (a_g != 0)
    near = ((dy <= 1.01 * lsb) & (dx <= 1.01 * lsb)) | ~live
    # a sample whose projected location sits within float noise of a level edge may take the other
    # fold (or validity) branch: those are the only ones allowed to move further
    assert near.double().mean().item() >= 0.9999, near.double().mean().item()
    assert (got[..., :16] == exp[..., :16]).double().mean().item() >= 0.95
    # weights: f16 of exp / rcp / fold products -- within 2 f16 ulps, plus 2^-11 where a fold or
    # validity decision sits within float noise of an edge (the sampled values below bound it all)
    da = (a_g - a_e).abs()
    assert (da[near] <= 2.0 ** -9 * a_e.abs()[near] + 2.0 ** -11).all(), da[near].max().item()
    assert (da[near] <= 2.0 ** -9 * a_e.abs()[near] + 1e-6).double().mean().item() >= 0.9999
    if masked:
        assert (a_g[qmask] == 0).all()
    S = sum(h * w_ for h, w_ in shapes)
    v = torch.randn(B, S, M, 32, generator=torch.Generator().manual_seed(5)).double().numpy()
    ss = np.array(shapes, dtype=np.int64)
    o_g = O.fwd(v, ss, l_g.numpy(), a_g.numpy())
    o_e = O.fwd(v, ss, l_e.numpy(), a_e.numpy())
    # a fraction that rounds to the neighbouring fixed-point step (f32 vs f64 location) moves a
    # sample by 2^-fb pixel: at most 2^-fb x (its weight <= 1) x (neighbouring values' difference)
    dmax, dmean = np.abs(o_g - o_e).max(), np.abs(o_g - o_e).mean()
    assert dmax <= 2.0 ** -fb * 2 * np.abs(v).max() + 2e-3 and dmean <= 1e-5, (dmax, dmean)


@pytest.mark.parametrize('shapes', [((100, 167), (50, 84), (25, 42), (13, 21)), ((25, 40), (15, 20), (8, 10), (4, 5))])
@pytest.mark.parametrize('ref_dim,masked', [(2, False), (2, True), (4, False)])
def test_sample_records_group_variants_bit_identical(shapes, ref_dim, masked):
    """The records GEMM with the position embedding added on load runs one 8-wave 384-column
    group per row tile (default) or two 4-wave 192-column groups (kinet_gemm_set_flags
    268435456): the same K order and epilogue per record, so bit-identical records."""
    from kinet_amd import _native
    from kinet_amd import kernels as K
    B, M = 3, 8
    x, pos, w, bias, ref, qmask, _ = _record_problem(shapes, B, 3.0, 7, ref_dim, masked)
    args = (x.cuda(), w.cuda(), bias.cuda(), M, ref.cuda(), shapes)
    kw = dict(x_add=pos.cuda(), query_attn_mask=qmask.cuda() if masked else None)
    r8, _ = K.msda_sample_records(*args, **kw)
    old = _native.lib().kinet_gemm_set_flags(268435456)
    try:
        r4, _ = K.msda_sample_records(*args, **kw)
    finally:
        _native.lib().kinet_gemm_set_flags(old)
    torch.cuda.synchronize()
    assert torch.equal(r8, r4)


@pytest.mark.parametrize('shapes', [
    ((100, 167), (50, 84), (25, 42), (13, 21)),    # config 2 (800x1333): level 0 gathered, 1-3 staged
    ((60, 70), (40, 50), (45, 50), (10, 13)),      # wide level 2: levels 2-3 staged
    ((25, 40), (15, 20), (8, 10), (4, 5)),         # every level staged whole
])
@pytest.mark.parametrize('noise,masked', [(0.5, False), (3.0, True), (25.0, False)])
def test_encoder_records_kernel_vs_oracle(shapes, noise, masked):
    """The sampling kernel fed records the ORACLE computed on the host (oracle.prep of the
    reference preparation -> oracle.sample_records), not any kinet kernel's: its output against
    the C oracle (cuh:165-237 restated) sampling the decoded records.  Small offsets read the
    strip's staged rows, noise 25 px leaves them (the far path).  Bound: f16 corner-weight
    products (2^-10 relative), each level's 16 taps summed as f16 pairs (2^-7 max|value|), one
    bf16 output rounding."""
    from kinet_amd import kernels as K
    from oracle import msda_oracle as O
    B, M, L, P = 2, 8, 4, 4
    S = sum(h * w for h, w in shapes)
    g = torch.Generator().manual_seed(17 + int(noise))
    value = torch.randn(M, B, S, 32, generator=g).half()
    offlog = torch.cat([noise * torch.randn(B, S, M * L * P * 2, generator=g), torch.randn(B, S, M * L * P, generator=g)],
                       -1).double()
    ref = _encoder_refs(shapes, B).cpu()
    qmask = (torch.rand(B, S, generator=g) < 0.1) if masked else None
    fb = K.msda_record_frac_bits(shapes)
    loc, aw = O.prep(offlog, ref.double(), shapes, qmask, M, L, P)
    rec = O.sample_records(loc, aw, ref, shapes, fb)
    order = K.encoder_tile_order(shapes, 'cuda')
    out = K.msda_encoder_records(value.cuda(), shapes, rec.cuda(), fb, out_dtype=torch.bfloat16,
                                 query_tile_order=order)
    out_nat = K.msda_encoder_records(value.cuda(), shapes, rec.cuda(), fb, out_dtype=torch.bfloat16)
    torch.cuda.synchronize()
    assert torch.equal(out, out_nat)   # tile order / strips change only when a tile runs
    l_d, a_d = O.decode_records(rec, shapes, fb)
    v = value.float().permute(1, 2, 0, 3).contiguous().double().numpy()
    ref_out = torch.from_numpy(O.fwd(v, np.array(shapes, dtype=np.int64), l_d.numpy(), a_d.numpy())).reshape(out.shape)
    d = (out.float().cpu().double() - ref_out).abs()
    vmax = value.float().abs().max().item()
    bound = 2.0 ** -7 * ref_out.abs() + (2.0 ** -7 + 2.0 ** -10) * vmax
    assert (d <= bound).all(), d.max().item()
    assert d.mean().item() <= 2e-3, d.mean().item()
    if masked:
        assert (out.float().cpu()[qmask] == 0).all()


def test_encoder_records_path_matches_offlog_path():
    """MSDeformAttn.sample on an encoder-sized bf16 call: the records path (default) against the
    f16 offsets / logits path (MSDA_RECORDS off) -- two quantisations of the same locations
    (2^-8 pixel fixed point vs f16 offsets), within the encoder kernel's bound."""
    from kinet_amd import kernels as K
    from kinet_amd.msda import MSDeformAttn
    shapes = ((100, 167), (50, 84), (25, 42), (13, 21))
    B, S = 2, sum(h * w for h, w in shapes)
    torch.manual_seed(3)
    attn = MSDeformAttn(256, 4, 8, 4).cuda()
    with torch.no_grad():
        attn.sampling_offsets.weight.normal_(0, 0.02)
        attn.attention_weights.weight.normal_(0, 0.05)
    src = torch.randn(B, S, 256, device='cuda').bfloat16()
    pos = torch.randn(B, S, 256, device='cuda').bfloat16()
    ref = _encoder_refs(shapes, B)
    ss = torch.tensor(shapes, device='cuda')
    with torch.no_grad():
        value = attn.project_value(src)
        o_rec = attn.sample(src, ref, value, ss, query_add=pos, shapes_host=shapes)
        K.MSDA_RECORDS[0] = False
        try:
            o_off = attn.sample(src, ref, value, ss, query_add=pos, shapes_host=shapes)
        finally:
            K.MSDA_RECORDS[0] = True
    torch.cuda.synchronize()
    d = (o_rec.float() - o_off.float()).abs()
    vmax = value.float().abs().max().item()
    assert (d <= o_off.float().abs() * 2.0 ** -6 + 2.0 ** -6 * vmax).all(), d.max().item()
    assert d.mean().item() <= 2e-3, d.mean().item()


@pytest.mark.parametrize('path', ['records', 'headmajor256', 'headmajor288', 'tiled'])
@pytest.mark.parametrize('B', [2, 3])
def test_frame_shared_load_add_bit_identical(path, B):
    """An x_add of ONE frame (the unpadded batch's shared position embedding: forward_flat passes
    frame 0's rows) read by every frame's rows (GemmArgs.a2_rows: row m adds row m % Lq) gives the
    same bits as the same operand materialised per frame -- the records GEMM, the head-major
    offsets projection at K = 256 and K = 288 (resident-weight kernel), and a small problem on the
    tiled kernel; Lq not a multiple of the row tile, so tiles straddle frames."""
    from kinet_amd import kernels as K
    dev = 'cuda'
    if path == 'records':
        shapes = ((25, 40), (15, 20), (8, 10), (4, 5))
        x, pos, w, bias, ref, _, _ = _record_problem(shapes, B, 3.0, 91 + B)
        x, w, bias, ref = x.to(dev), w.to(dev), bias.to(dev), ref.to(dev)
        p1 = pos[:1].to(dev)
        r_sh, fb = K.msda_sample_records(x, w, bias, 8, ref, shapes, x_add=p1)
        r_ex, _ = K.msda_sample_records(x, w, bias, 8, ref, shapes, x_add=p1.expand(B, -1, -1).contiguous())
        torch.cuda.synchronize()
        assert torch.equal(r_sh, r_ex)
        return
    d, Lq = {'headmajor256': (256, 4699), 'headmajor288': (288, 4699), 'tiled': (256, 333)}[path]
    g = torch.Generator().manual_seed(7 + B + d)
    dt = torch.float16
    x = torch.randn(B, Lq, d, generator=g).to(dt).to(dev)
    p1 = (0.5 * torch.randn(1, Lq, d, generator=g)).to(dt).to(dev)
    w = (torch.randn(8 * 48, d, generator=g) / 16).to(dt).to(dev)
    b = torch.randn(8 * 48, generator=g).to(dev)
    y_sh = K.offsets_proj_headmajor(x, w, b, 8, x_add=p1)
    y_ex = K.offsets_proj_headmajor(x, w, b, 8, x_add=p1.expand(B, -1, -1).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(y_sh, y_ex)
    ref = ((x.float() + p1.float()).to(dt).float() @ w.float().T + b).reshape(B, Lq, 8, 48).permute(2, 0, 1, 3)
    assert (y_sh.float() - ref).abs().max().item() < 2e-2 * ref.abs().max().item()
