"""Dispatch of stage 1's downsample fold (no GPU): which shapes bottleneck_pair_ds_supported takes,
and which kernel wrappers forward_layer_nhwc calls with FUSE_DOWNSAMPLE on / off."""
import pytest
import torch

from kinet_amd import kernels as K
from kinet_amd.models import backbone as BB


def _w(*shape):
    return torch.empty(*shape)


def test_bottleneck_pair_ds_supported_only_stage1():
    ok = (_w(256, 64, 1, 1), _w(256, 64, 1, 1), _w(64, 256, 1, 1))
    for dt in (torch.bfloat16, torch.float16):
        assert K.bottleneck_pair_ds_supported(dt, *ok)
    assert not K.bottleneck_pair_ds_supported(torch.float32, *ok)
    # stages 2-4: wider bottlenecks and 256 / 512 / 1024 input channels
    assert not K.bottleneck_pair_ds_supported(torch.bfloat16, _w(512, 128, 1, 1), _w(512, 256, 1, 1), _w(128, 512, 1, 1))
    assert not K.bottleneck_pair_ds_supported(torch.bfloat16, _w(1024, 256, 1, 1), _w(1024, 512, 1, 1), _w(256, 1024, 1, 1))
    # stage 1's last pair (next conv1 128 wide), a 128-channel block input, a 3x3 identity conv
    assert not K.bottleneck_pair_ds_supported(torch.bfloat16, ok[0], ok[1], _w(128, 256, 1, 1))
    assert not K.bottleneck_pair_ds_supported(torch.bfloat16, ok[0], _w(256, 128, 1, 1), ok[2])
    assert not K.bottleneck_pair_ds_supported(torch.bfloat16, ok[0], _w(256, 64, 3, 3), ok[2])


@pytest.fixture
def calls(monkeypatch):
    """Shape-only stand-ins for the kernel wrappers forward_layer_nhwc uses; records their names."""
    log = []

    def conv_bn(x, conv, bn, relu, residual=None, cin_pad=None):
        log.append(('conv_bn', conv))
        B, H, W, _ = x.shape
        s = conv.stride[0]
        return torch.zeros(B, (H - 1) // s + 1, (W - 1) // s + 1, conv.out_channels, dtype=x.dtype)

    def pair(x, residual, packed, b3, b1):
        log.append(('pair', None))
        assert residual is not None
        B, H, W, D = x.shape
        return torch.zeros(B, H, W, 4 * D, dtype=x.dtype), torch.zeros(B, H, W, b1.numel(), dtype=x.dtype)

    def pair_ds(x, x0, packed, b3ds, b1):
        log.append(('pair_ds', None))
        B, H, W, D = x.shape
        return torch.zeros(B, H, W, 256, dtype=x.dtype), torch.zeros(B, H, W, 64, dtype=x.dtype)

    monkeypatch.setattr(BB, 'conv_bn', conv_bn)
    monkeypatch.setattr(K, 'bottleneck_pair', pair)
    monkeypatch.setattr(K, 'bottleneck_pair_ds', pair_ds)
    monkeypatch.setattr(K, 'bottleneck_pack', lambda *a: None)
    monkeypatch.setattr(K, 'bottleneck_pack_ds', lambda *a: (None, None))
    monkeypatch.setattr(BB, 'FUSE_BOTTLENECK_PAIRS', True)
    monkeypatch.setattr(BB, 'FUSE_PAIR_WIDTHS', (64, 128, 256))
    return log


def _run(layer, nxt, dtype, cin):
    x = torch.zeros(1, 6, 7, cin, dtype=dtype)
    return BB.forward_layer_nhwc(layer, x, None, nxt)


def test_forward_layer_flag_off_takes_no_new_path(calls, monkeypatch):
    body = BB.ResNetBody([3, 4, 6, 3])
    ds = body.layer1[0].downsample[0]
    monkeypatch.setattr(BB, 'FUSE_DOWNSAMPLE', False)
    y, t = _run(body.layer1, body.layer2[0], torch.bfloat16, 64)
    assert y.shape == (1, 6, 7, 256) and t.shape == (1, 6, 7, 128)
    assert [n for n, _ in calls].count('pair_ds') == 0
    assert [n for n, _ in calls].count('pair') == 3
    assert ('conv_bn', ds) in calls   # the downsample conv ran on its own


def test_forward_layer_flag_on_folds_stage1_only(calls, monkeypatch):
    body = BB.ResNetBody([3, 4, 6, 3])
    monkeypatch.setattr(BB, 'FUSE_DOWNSAMPLE', True)
    y, t = _run(body.layer1, body.layer2[0], torch.bfloat16, 64)
    assert y.shape == (1, 6, 7, 256) and t.shape == (1, 6, 7, 128)
    names = [n for n, _ in calls]
    assert names.count('pair_ds') == 1 and names.count('pair') == 2
    assert ('conv_bn', body.layer1[0].downsample[0]) not in calls
    # f32 (the training path's frozen stem + layer1): every conv on its own, as before
    del calls[:]
    _run(body.layer1, None, torch.float32, 64)
    names = [n for n, _ in calls]
    assert names.count('pair_ds') == 0 and names.count('pair') == 0
    assert ('conv_bn', body.layer1[0].downsample[0]) in calls
    # stage 2: a strided downsample over 256 channels stays a launch of its own
    del calls[:]
    _run(body.layer2, body.layer3[0], torch.bfloat16, 256)
    names = [n for n, _ in calls]
    assert names.count('pair_ds') == 0 and names.count('pair') == 3   # 128 -> 256 across the stage end is not a pair
    assert ('conv_bn', body.layer2[0].downsample[0]) in calls
    # pairs switched off: no fold either
    del calls[:]
    monkeypatch.setattr(BB, 'FUSE_BOTTLENECK_PAIRS', False)
    _run(body.layer1, body.layer2[0], torch.bfloat16, 64)
    names = [n for n, _ in calls]
    assert names.count('pair_ds') == 0 and names.count('pair') == 0
    assert ('conv_bn', body.layer1[0].downsample[0]) in calls
