"""The attention out-projection + norm1 fold into the fused FFN (kinet_attn_out_ffn_fused): the
gate, the switch and the launch record -- no GPU needed."""
import torch

from kinet_amd import _native as N
from kinet_amd import kernels as K
from kinet_amd.models import deformable_transformer as dt


def _mods(d=256, f=1024, **kw):
    with torch.device('meta'):
        return (torch.nn.Linear(d, d, bias=kw.get('bo', True)), torch.nn.Linear(d, f, bias=kw.get('b1', True)),
                torch.nn.Linear(f, d, bias=kw.get('b2', True)))


def _x(m, d=256, dtype=torch.bfloat16):
    return torch.empty(m, d, dtype=dtype, device='meta')


def test_gate_dtype_width_rows_and_biases():
    ok = _mods()
    assert K.attn_out_ffn_supported(_x(16384), *ok)
    assert K.attn_out_ffn_supported(_x(16384, dtype=torch.float16), *ok)
    assert K.attn_out_ffn_supported(torch.empty(28, 1000, 256, dtype=torch.bfloat16, device='meta'), *ok)   # 28000 rows
    assert not K.attn_out_ffn_supported(_x(16384, dtype=torch.float32), *ok)
    assert not K.attn_out_ffn_supported(_x(16383), *ok)       # below the 8-wave x 32-row tile's threshold
    assert not K.attn_out_ffn_supported(_x(0), *ok)
    assert not K.attn_out_ffn_supported(_x(20000, 288), *_mods(288))
    assert not K.attn_out_ffn_supported(_x(20000, 128), *_mods(128))
    for missing in ('bo', 'b1', 'b2'):
        assert not K.attn_out_ffn_supported(_x(20000), *_mods(**{missing: False}))
    assert K.ATTN_OUT_FFN_MIN_ROWS == 16384


def test_flag_default_on():
    assert dt.FUSE_ATTN_OUT_FFN is True


def test_work_record_stays_in_the_ffn_bucket(monkeypatch):
    """bench.py's roofline buckets GEMM launches whose shape tuple starts with 'ffn'."""
    seen = {}

    def fake_call(name, *args, work=None):
        seen[name] = work
    monkeypatch.setattr(N, 'call', fake_call)
    monkeypatch.setattr(N, 'require_gpu', lambda *t: None)
    monkeypatch.setattr(N, 'ptr', lambda t: 0)
    monkeypatch.setattr(N, 'stream', lambda dev: 0)
    M, D, Fh = 16384, 256, 1024
    out_proj, lin1, lin2 = torch.nn.Linear(D, D), torch.nn.Linear(D, Fh), torch.nn.Linear(Fh, D)
    n1, n2 = torch.nn.LayerNorm(D), torch.nn.LayerNorm(D)
    a = torch.zeros(M, D, dtype=torch.bfloat16)
    y = K.attn_out_ffn_fused(a, out_proj, a, n1, lin1, lin2, n2)
    assert y.shape == (M, D)
    assert 'kinet_ffn_pack_attn' in seen
    w = seen['kinet_attn_out_ffn_fused']
    assert w['family'] == 'gemm' and w['shape'][0] == 'ffn' and w['shape'] == ('ffn', M, D, Fh, 'attn_out')
    assert w['flops'] == 4.0 * M * D * Fh + 2.0 * M * D * D
    assert w['bytes'] == (3 * M * D + D * D + 2 * D * Fh) * 2
