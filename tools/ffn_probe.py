"""Run only the fused FFN kernel (config-2 encoder shape at batch 8 unless --rows) a few
times -- a short program for rocprofv3 --pmc passes (tools/pmc_probe.sh).  --attn-out times the
encoder layer tail instead: the out-projection GEMM + fused FFN against kinet_attn_out_ffn_fused."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kinet_amd import kernels as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rows', type=int, default=8 * 22223)
ap.add_argument('--iters', type=int, default=5)
ap.add_argument('--d', type=int, default=256)
ap.add_argument('--knobs', default='0,2,8', help='kinet_ffn_set_debug values (the FfnDebug bits of csrc/ffn_plan.h)')
ap.add_argument('--dtype', default='bf16', choices=['bf16', 'f16'])
ap.add_argument('--attn-out', action='store_true',
                help='time the encoder tail instead: K.linear(out_proj, residual, ln) + K.ffn_fused against '
                     'K.attn_out_ffn_fused (late and staged residual loads), config-2 encoder rows at --batches')
ap.add_argument('--batches', default='24,28')
ap.add_argument('--launches', type=int, default=20)
ap.add_argument('--repeats', type=int, default=5)
a = ap.parse_args()
D = a.d
dt = torch.bfloat16 if a.dtype == 'bf16' else torch.float16


def attn_out_mode():
    """Per batch: events over --launches launches, --repeats times, the variants interleaved;
    clocks warmed first (~0.3 s of the same work, as tools/conv_ab.py does)."""
    import time
    from kinet_amd import _native as N
    tokens = 22223   # config-2 encoder tokens per frame
    out_proj, lin1, lin2 = torch.nn.Linear(D, D).cuda(), torch.nn.Linear(D, 1024).cuda(), torch.nn.Linear(1024, D).cuda()
    n1, n2 = torch.nn.LayerNorm(D).cuda(), torch.nn.LayerNorm(D).cuda()

    def pair(samp, src):
        x = K.linear(samp, out_proj.weight, out_proj.bias, residual=src, ln=(n1.weight, n1.bias, n1.eps))
        return K.ffn_fused(x, lin1, lin2, n2)

    def gemm_only(samp, src):
        return K.linear(samp, out_proj.weight, out_proj.bias, residual=src, ln=(n1.weight, n1.bias, n1.eps))

    def fused(knob):
        def run(samp, src):
            N.lib().kinet_ffn_set_debug(knob)
            y = K.attn_out_ffn_fused(samp, out_proj, src, n1, lin1, lin2, n2)
            N.lib().kinet_ffn_set_debug(0)
            return y
        return run
    variants = [('two launches', pair), ('  out_proj+LN1 GEMM alone', gemm_only), ('fused, residual late', fused(0)),
                ('fused, residual staged', fused(64))]
    for batch in [int(b) for b in a.batches.split(',')]:
        M = batch * tokens
        samp = torch.randn(M, D, device='cuda', dtype=dt)
        src = torch.randn(M, D, device='cuda', dtype=dt)
        t_end = time.perf_counter() + 0.3
        while time.perf_counter() < t_end:
            pair(samp, src)
            fused(0)(samp, src)
            torch.cuda.synchronize()
        times = {name: [] for name, _ in variants}
        outs = {}
        for _ in range(a.repeats):
            for name, fn in variants:
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(a.launches):
                    outs[name] = fn(samp, src)
                e.record()
                torch.cuda.synchronize()
                times[name].append(s.elapsed_time(e) * 1e3 / a.launches)
        for name, _ in variants:
            t = sorted(times[name])
            print('attn_out_ffn batch %d rows %d %s: %-28s median %.1f us  min %.1f  max %.1f' %
                  (batch, M, a.dtype, name, t[len(t) // 2], t[0], t[-1]))
        d = (outs['fused, residual staged'].float() - outs['two launches'].float()).abs()
        print('attn_out_ffn batch %d: fused vs two launches max |d| %.4g, %d of %d elements differ; staged vs late %s' %
              (batch, d.max().item(), int((d > 0).sum()), d.numel(),
               'bit-identical' if torch.equal(outs['fused, residual staged'], outs['fused, residual late']) else 'DIFFER'))
    print('ffn_probe done')


if a.attn_out:
    attn_out_mode()
    sys.exit(0)
lin1, lin2, norm = torch.nn.Linear(D, 1024).cuda(), torch.nn.Linear(1024, D).cuda(), torch.nn.LayerNorm(D).cuda()
x = torch.randn(a.rows, D, device='cuda', dtype=dt)
from kinet_amd import _native as N  # noqa: E402
ref = None
for knob in [int(k) for k in a.knobs.split(',')]:
    N.lib().kinet_ffn_set_debug(knob)
    for _ in range(2):
        y = K.ffn_fused(x, lin1, lin2, norm)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(a.iters):
        y = K.ffn_fused(x, lin1, lin2, norm)
    e.record()
    torch.cuda.synchronize()
    us = s.elapsed_time(e) * 1e3 / a.iters
    tf = 4.0 * a.rows * D * 1024 / (us * 1e-6) / 1e12
    same = 'ref' if ref is None else ('bit-identical' if torch.equal(ref, y) else
                                     'max diff %.3g' % (ref.float() - y.float()).abs().max().item())
    ref = y if ref is None else ref
    print('ffn_probe knob %d: rows %d, %.1f us, %.0f TF/s, %s' % (knob, a.rows, us, tf, same))
N.lib().kinet_ffn_set_debug(0)
print('ffn_probe done')
