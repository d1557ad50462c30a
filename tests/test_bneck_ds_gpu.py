"""kinet_bottleneck_pair_ds: stage 1's first bottleneck pair with block 0's downsample conv folded
into phase A (one GEMM over K = 64 + 64), alone against fp32 and inside the ResNet body."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('B,H,W', [(1, 1, 5), (2, 37, 53), (4, 100, 167)])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_bottleneck_pair_ds_vs_fp32(B, H, W, dtype):
    """Against torch fp32 on the same rounded, scale-folded weights: y within 2 output ulps of
    relu(x W3r^T + x0 Wdsr^T + b3 + b_ds), t within 2 ulps of the fp32 conv1 of OUR y.  5 rows =
    one ragged tile; 3,922 rows = several workgroups and a ragged tail; 66,800 rows = more 16-row
    tiles than a 256-CU part has waves, so some waves take a second tile (the next-tile t2 / x0
    prefetch) and the others prefetch out of range."""
    from kinet_amd import kernels as K
    D, F_, DB = 64, 256, 64
    g = torch.Generator().manual_seed(1000 * B + H)
    dev = 'cuda'
    x = torch.relu(torch.randn(B, H, W, D, generator=g)).to(dtype).to(dev)
    x0 = torch.relu(torch.randn(B, H, W, D, generator=g)).to(dtype).to(dev)
    w3 = (torch.randn(F_, D, 1, 1, generator=g) * (2.0 / D) ** 0.5).to(dev)
    wd = (torch.randn(F_, D, 1, 1, generator=g) * (2.0 / D) ** 0.5).to(dev)
    w1 = (torch.randn(DB, F_, 1, 1, generator=g) * (2.0 / F_) ** 0.5).to(dev)
    s3, b3 = (torch.rand(F_, generator=g) + 0.5).to(dev), (torch.randn(F_, generator=g) * 0.1).to(dev)
    sd, bd = (torch.rand(F_, generator=g) + 0.5).to(dev), (torch.randn(F_, generator=g) * 0.1).to(dev)
    s1, b1 = (torch.rand(DB, generator=g) + 0.5).to(dev), (torch.randn(DB, generator=g) * 0.1).to(dev)
    packed, b3ds = K.bottleneck_pack_ds(w3, wd, w1, s3, sd, s1, b3, bd, dtype)
    y, t = K.bottleneck_pair_ds(x, x0, packed, b3ds, b1)
    torch.cuda.synchronize()
    w3r = (w3.reshape(F_, D) * s3[:, None]).to(dtype).float()
    wdr = (wd.reshape(F_, D) * sd[:, None]).to(dtype).float()
    w1r = (w1.reshape(DB, F_) * s1[:, None]).to(dtype).float()
    y_ref = torch.relu(x.reshape(-1, D).float() @ w3r.T + x0.reshape(-1, D).float() @ wdr.T + b3 + bd)
    ulp = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    ey = (y.reshape(-1, F_).float() - y_ref).abs()
    print(f'max |y - y_ref| = {ey.max().item():.3e}, worst margin = '
          f'{(ey - (2 * ulp * y_ref.abs() + 1e-3)).max().item():.3e}')
    assert (ey <= 2 * ulp * y_ref.abs() + 1e-3).all(), ey.max().item()
    t_ref = torch.relu(y.reshape(-1, F_).float() @ w1r.T + b1)
    et = (t.reshape(-1, DB).float() - t_ref).abs()
    print(f'max |t - t_ref| = {et.max().item():.3e}, worst margin = '
          f'{(et - (2 * ulp * t_ref.abs() + 1e-3)).max().item():.3e}')
    assert (et <= 2 * ulp * t_ref.abs() + 1e-3).all(), et.max().item()


@pytest.mark.parametrize('M', [5, 3922, 140005])
def test_bottleneck_pair_ds_tile_variants_bit_identical(M):
    """The 2 x 16-row-tile variant (kinet_ffn_set_debug 512, the A/B knob of tools/bneck_ab.py) sums
    every element in the same order as the default 16-row tiles: bit-identical y and t, incl. row
    counts that are no multiple of 32 and, at 140,005 rows, more 32-row tiles than a 256-CU part has
    waves (the 2-tile variant's own next-tile loads)."""
    from kinet_amd import _native
    from kinet_amd import kernels as K
    g = torch.Generator().manual_seed(M)
    x = torch.relu(torch.randn(M, 1, 1, 64, generator=g)).bfloat16().cuda()
    x0 = torch.relu(torch.randn(M, 1, 1, 64, generator=g)).bfloat16().cuda()
    w3 = (torch.randn(256, 64, 1, 1, generator=g) * 0.2).cuda()
    wd = (torch.randn(256, 64, 1, 1, generator=g) * 0.2).cuda()
    w1 = (torch.randn(64, 256, 1, 1, generator=g) * 0.1).cuda()
    s3, sd, s1 = torch.ones(256).cuda(), torch.ones(256).cuda(), torch.ones(64).cuda()
    b3, bd, b1 = (torch.randn(256, generator=g) * 0.1).cuda(), torch.zeros(256).cuda(), torch.zeros(64).cuda()
    packed, b3ds = K.bottleneck_pack_ds(w3, wd, w1, s3, sd, s1, b3, bd, torch.bfloat16)
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    outs, ran = [], []
    try:
        for knob in (0, 512):
            _native.lib().kinet_ffn_set_debug(knob)
            outs.append(K.bottleneck_pair_ds(x, x0, packed, b3ds, b1))
            ran.append(K.ffn_last_kernel())
            assert ran[-1] == K.ffn_launch_plan('pair_ds', M, 64, cus=cus)['kernel']   # the CPU plan of this call
    finally:
        _native.lib().kinet_ffn_set_debug(0)
    torch.cuda.synchronize()
    assert ran[0] != ran[1]   # the knob took
    assert torch.isfinite(outs[0][0].float()).all() and outs[0][0].float().abs().sum() > 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_backbone_downsample_fold_matches_unfused(dtype):
    """ResNet-50 body with stage 1's downsample folded into the first pair vs the downsample conv
    on its own (FUSE_DOWNSAMPLE = False): the fold keeps the identity branch in f32 and rounds
    s_ds into the weights, so the four stage outputs agree to bf16 / f16 accumulation level (the
    bounds of the fused-pairs test), not bit for bit."""
    from kinet_amd import _native
    from kinet_amd.models import backbone as BB
    torch.manual_seed(0)
    body = BB.ResNetBody([3, 4, 6, 3]).cuda().eval()
    with torch.no_grad():
        for m in body.modules():
            if isinstance(m, BB.FrozenBatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.1)
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    img = torch.randn(2, 3, 160, 224, device='cuda')
    old = BB.FUSE_BOTTLENECK_PAIRS, BB.FUSE_PAIR_WIDTHS, BB.FUSE_DOWNSAMPLE
    try:
        BB.FUSE_BOTTLENECK_PAIRS, BB.FUSE_PAIR_WIDTHS, BB.FUSE_DOWNSAMPLE = True, (64, 128, 256), True
        _native.trace_begin()
        try:
            fused = body.forward_nhwc(img, dtype)
        finally:
            names = [n for n, *_ in _native.trace_end()]
        BB.FUSE_DOWNSAMPLE = False
        plain = body.forward_nhwc(img, dtype)
    finally:
        BB.FUSE_BOTTLENECK_PAIRS, BB.FUSE_PAIR_WIDTHS, BB.FUSE_DOWNSAMPLE = old
    torch.cuda.synchronize()
    assert names.count('kinet_bottleneck_pair_ds') == 1   # the fold really ran
    for a, b in zip(fused, plain):
        assert a.shape == b.shape
        rel = ((a.float() - b.float()).norm() / b.float().norm()).item()
        print(f'stage output {tuple(a.shape)}: relative norm difference {rel:.3e}')
        assert rel < (3e-2 if dtype == torch.bfloat16 else 5e-3), rel
