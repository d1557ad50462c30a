"""GPU numerics of kinet_attn_out_ffn_fused: the encoder layer's attention out-projection +
norm1 folded into the fused FFN launch, y = LN2(x + W2 relu(W1 x + b1) + b2) with
x = LN1(R + A Wo^T + bo), vs a float64 chain with the same two roundings and vs the two-launch
kinet path (K.linear(..., ln=) then K.ffn_fused)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

D, FH = 256, 1024
TOL = {torch.bfloat16: 6e-2, torch.float16: 8e-3}      # test_ffn_fused_vs_fp32's bounds
ULP = {torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}


@pytest.fixture(scope='module')
def K():
    from kinet_amd import kernels
    return kernels


def _modules(seed, d=D):
    """out_proj, norm1, linear1, linear2, norm2 with random LayerNorm gammas / betas."""
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    out_proj, lin1, lin2 = torch.nn.Linear(d, d), torch.nn.Linear(d, FH), torch.nn.Linear(FH, d)
    n1, n2 = torch.nn.LayerNorm(d), torch.nn.LayerNorm(d)
    with torch.no_grad():
        for n in (n1, n2):
            n.weight.copy_(torch.randn(d, generator=g) * 0.5 + 1.0)
            n.bias.copy_(torch.randn(d, generator=g) * 0.5)
    return out_proj, n1, lin1, lin2, n2


def _reference(a, r, mods, dtype, with_norm2=True):
    """float64 (torch, on the inputs' device) on the 16-bit inputs and 16-bit-rounded weights;
    x and the hidden activations rounded to the 16-bit type where the kernels round them."""
    out_proj, n1, lin1, lin2, n2 = mods
    f64 = lambda t: t.detach().double()                                    # noqa: E731
    w16 = lambda lin: lin.weight.detach().to(dtype).double()               # noqa: E731
    x = F.layer_norm(r.double() + F.linear(a.double(), w16(out_proj), f64(out_proj.bias)), (D,),
                     f64(n1.weight), f64(n1.bias), n1.eps).to(dtype).double()
    h = F.relu(F.linear(x, w16(lin1), f64(lin1.bias))).to(dtype).double()
    y = x + F.linear(h, w16(lin2), f64(lin2.bias))
    if with_norm2:
        y = F.layer_norm(y, (D,), f64(n2.weight), f64(n2.bias), n2.eps)
    return y


def _unfused(K, a, r, mods, with_norm2=True):
    out_proj, n1, lin1, lin2, n2 = mods
    x = K.linear(a, out_proj.weight, out_proj.bias, residual=r, ln=(n1.weight, n1.bias, n1.eps))
    return K.ffn_fused(x, lin1, lin2, n2 if with_norm2 else None)


def _assert_ulp_close(y, yk, dtype):
    d = (y.float() - yk.float()).abs()
    ulp = ULP[dtype]
    bound = ulp * torch.maximum(y.float().abs(), yk.float().abs()) + 3 * ulp
    print('vs two-launch path: max |d| %.4g, elements differing %d of %d' % (d.max().item(), int((d > 0).sum()), d.numel()))
    assert (d <= bound).all(), d.max().item()


@pytest.mark.parametrize('M', [1, 300, 16384, 16391, 65836])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_attn_out_ffn_vs_fp64_and_unfused(K, M, dtype):
    """M = 16391: ragged last tile; M = 65836: 258 tiles of 256 rows, so on 256 CUs two
    workgroups walk a second tile and the ring wraps across a tile boundary.  Small M goes
    through the wrapper with the row gate bypassed (force=True)."""
    mods = _modules(M)
    g = torch.Generator().manual_seed(M + 1)
    a = torch.randn(M, D, generator=g).to(dtype)
    r = torch.randn(M, D, generator=g).to(dtype)
    mods = [m.cuda() for m in mods]
    ac, rc = a.cuda(), r.cuda()
    ref = _reference(ac, rc, mods, dtype)
    y = K.attn_out_ffn_fused(ac, mods[0], rc, mods[1], mods[2], mods[3], mods[4], force=True)
    torch.cuda.synchronize()
    assert y.shape == (M, D) and y.dtype == dtype
    err = (y.double() - ref).abs().max().item()
    print('M %d %s: max |y - ref64| %.4g' % (M, dtype, err))
    assert err < TOL[dtype], err
    _assert_ulp_close(y, _unfused(K, ac, rc, mods), dtype)
    # determinism: the sums run in a fixed order
    y2 = K.attn_out_ffn_fused(ac, mods[0], rc, mods[1], mods[2], mods[3], mods[4], force=True)
    assert torch.equal(y, y2)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_attn_out_ffn_residual_staging_bit_identical(K, dtype):
    """kinet_ffn_set_debug 64 loads the residual under the Wo chunks instead of after the last one (RV = 1): another
    kernel, the same sums in the same order, so bit-identical outputs; 16391 rows = 65 tiles with a ragged last one.
    Each call runs the kernel the CPU planner names for it."""
    from kinet_amd import _native
    M = 16391
    mods = [m.cuda() for m in _modules(64)]
    g = torch.Generator().manual_seed(65)
    a, r = torch.randn(M, D, generator=g).to(dtype).cuda(), torch.randn(M, D, generator=g).to(dtype).cuda()
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    outs, ran = [], []
    try:
        for knob in (0, 64):
            _native.lib().kinet_ffn_set_debug(knob)
            outs.append(K.attn_out_ffn_fused(a, mods[0], r, mods[1], mods[2], mods[3], mods[4]))
            ran.append(K.ffn_last_kernel())
            assert ran[-1] == K.ffn_launch_plan('attn_out_ffn', M, D, FH, cus=cus)['kernel']
    finally:
        _native.lib().kinet_ffn_set_debug(0)
    torch.cuda.synchronize()
    assert ran == ['ffn_fused_rt2_kernel<256, true>', 'ffn_fused_rt2_kernel<256, true, 1>']
    assert torch.isfinite(outs[0].float()).all() and torch.equal(outs[0], outs[1])


def test_attn_out_ffn_strides_out_and_no_norm2(K):
    """A and R column slices of wider buffers (lda, ldr > D), out= given, norm2 absent."""
    dtype, M = torch.bfloat16, 700
    mods = _modules(5)
    g = torch.Generator().manual_seed(6)
    wide_a = torch.randn(M, D + 64, generator=g).to(dtype)
    wide_r = torch.randn(M, 2 * D, generator=g).to(dtype)
    mods = [m.cuda() for m in mods]
    ac, rc = wide_a.cuda()[:, 32:32 + D], wide_r.cuda()[:, D:]
    ref = _reference(ac, rc, mods, dtype)
    ref_nonorm = _reference(ac, rc, mods, dtype, with_norm2=False)
    assert ac.stride(0) == D + 64 and rc.stride(0) == 2 * D
    out = torch.full((M, D), float('nan'), dtype=dtype, device='cuda')
    y = K.attn_out_ffn_fused(ac, mods[0], rc, mods[1], mods[2], mods[3], mods[4], out=out, force=True)
    torch.cuda.synchronize()
    assert y.data_ptr() == out.data_ptr()
    assert (out.double() - ref).abs().max().item() < TOL[dtype]
    _assert_ulp_close(out, _unfused(K, ac, rc, mods), dtype)
    y0 = K.attn_out_ffn_fused(ac, mods[0], rc, mods[1], mods[2], mods[3], None, force=True)
    assert (y0.double() - ref_nonorm).abs().max().item() < TOL[dtype]
    _assert_ulp_close(y0, _unfused(K, ac, rc, mods, with_norm2=False), dtype)


def test_attn_out_ffn_errors(K):
    for d, msg in ((288, 'D = 288 is not supported'), (128, 'D must be 256')):
        mods = [m.cuda() for m in _modules(d, d)]
        a = torch.randn(40, d, device='cuda').bfloat16()
        with pytest.raises(RuntimeError, match=msg):
            K.attn_out_ffn_fused(a, mods[0], a.clone(), mods[1], mods[2], mods[3], mods[4], force=True)
    mods = [m.cuda() for m in _modules(3)]
    x = torch.empty(20000, D, device='cuda', dtype=torch.bfloat16)
    assert K.attn_out_ffn_supported(x, mods[0], mods[2], mods[3])
    nobias = torch.nn.Linear(D, D, bias=False).cuda()
    assert not K.attn_out_ffn_supported(x, nobias, mods[2], mods[3])
    with pytest.raises(RuntimeError, match='unsupported'):
        K.attn_out_ffn_fused(x[:100], mods[0], x[:100], mods[1], mods[2], mods[3], mods[4])   # below the row gate


def test_encoder_layer_flag_on_off():
    """One encoder layer at d_model 256, bf16, 10 frames x 1700 tokens = 17000 rows: the fused
    tail agrees with the two launches to output rounding and no (M, 256, 256) GEMM is launched."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    from weights import randomize
    from kinet_amd import _native as N
    from kinet_amd.models import deformable_transformer as dt
    shapes = [(32, 40), (16, 20), (8, 10), (4, 5)]
    S, B = sum(h * w for h, w in shapes), 10
    enc = randomize(dt.DeformableTransformerEncoderLayer(256, 1024, 0.1, 'relu', 4, 8, 4), seed=7).cuda().eval()
    g = torch.Generator().manual_seed(11)
    src = torch.randn(B, S, 256, generator=g).cuda().bfloat16()
    pos = torch.randn(B, S, 256, generator=g).cuda().bfloat16()
    ref_pts = torch.rand(B, S, 4, 2, generator=g).cuda()
    sp = torch.tensor(shapes, dtype=torch.long, device='cuda')
    outs, traces = {}, {}
    prev = dt.FUSE_ATTN_OUT_FFN
    try:
        for flag in (True, False):
            dt.FUSE_ATTN_OUT_FFN = flag
            with torch.no_grad():
                enc(src, pos, ref_pts, sp, None, shapes_host=shapes)   # warm-up: packs the weights
                N.trace_begin()
                try:
                    outs[flag] = enc(src, pos, ref_pts, sp, None, shapes_host=shapes)
                finally:
                    traces[flag] = N.trace_end()
            torch.cuda.synchronize()
    finally:
        dt.FUSE_ATTN_OUT_FFN = prev
    M = B * S
    shapes_on = [(n, w.get('shape')) for n, w, _, _ in traces[True]]
    shapes_off = [(n, w.get('shape')) for n, w, _, _ in traces[False]]
    assert ('kinet_gemm_ex', (M, 256, 256)) in shapes_off
    assert ('kinet_gemm_ex', (M, 256, 256)) not in shapes_on
    assert shapes_on[-1] == ('kinet_attn_out_ffn_fused', ('ffn', M, 256, 1024, 'attn_out'))
    assert len(shapes_on) == len(shapes_off) - 1
    assert torch.isfinite(outs[True].float()).all()
    _assert_ulp_close(outs[True].reshape(M, 256), outs[False].reshape(M, 256), torch.bfloat16)
