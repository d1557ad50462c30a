"""Microbenchmark of the attention core (`kernels.mha_core`), batch 16, 8 heads, at vanilla DETR's
shapes -- one 800x1333 frame is a 25x42 stride-32 map = 1050 keys, for the encoder self-attention
(Lq = Lk = 1050) and the decoder cross-attention (Lq = 100 at d 256, 500 at d 288) -- and at the
decoder query self-attention shapes of the Deformable DETR models (300 queries at d 256; 500 + 20
and 500 x 640 at d 288), whose keys stay resident in LDS.

Each shape is timed on the default dispatch (the MFMA kernels of csrc/attn.hip: `kernel` names
which one ran) and with kinet_mha_set_mfma(0) (the FMA kernel), alternating the two in one
process: per variant a warm-up, then `--repeats` windows of `--iters` calls between HIP events, median and spread of the
windows.  The outputs of the two are compared on the timed inputs first.  One JSON line per shape;
`mfma_peak_frac` is the useful attention FLOPs (4 * B * heads * Lq * Lk * head_dim, padding
excluded) per second over the 2.5 PFLOP/s dense 16-bit MFMA peak.

usage: python tools/bench_mha.py [--dtype bf16|f16] [--iters N] [--repeats R] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kinet_amd import _native  # noqa: E402
from kinet_amd import kernels as K  # noqa: E402

PEAK_16BIT_FLOPS = 2.5e15   # dense bf16 / f16 MFMA, MI355X
SHAPES = [  # (tag, head_dim, Lq, Lk)
    ('enc_self_d32', 32, 1050, 1050),
    ('enc_self_d36', 36, 1050, 1050),
    ('dec_cross_d32', 32, 100, 1050),
    ('dec_cross_d36', 36, 500, 1050),
    ('dec_self_d32', 32, 300, 300),
    ('dec_self_d36', 36, 520, 520),
    ('dec_self_d36_640', 36, 500, 640),
]
BATCH, HEADS = 16, 8


def window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3   # us per call


def bench_shape(tag, D, Lq, Lk, dtype, iters, repeats):
    lib = _native.lib()
    E = HEADS * D
    g = torch.Generator(device='cuda').manual_seed(Lq + Lk + D)
    q, k, v = (torch.randn(BATCH, n, E, device='cuda', generator=g).to(dtype) for n in (Lq, Lk, Lk))
    mask = torch.rand(BATCH, Lk, device='cuda', generator=g) < 0.1
    mask[:, 0] = False
    mask = mask.to(torch.uint8)
    out = torch.empty(BATCH, Lq, E, dtype=dtype, device='cuda')

    def run(knob):
        old = lib.kinet_mha_set_mfma(knob)
        try:
            K.mha_core(q, k, v, HEADS, D ** -0.5, key_mask=mask, out=out)
        finally:
            lib.kinet_mha_set_mfma(old)

    run(1)
    # (a library from before kinet_mha_last_kernel, under KINET_AMD_LIB: no name)
    kernel = K.mha_last_kernel() if _native.exported('kinet_mha_last_kernel') else None
    y = out.float().clone()
    run(0)
    y_fma = out.float().clone()
    rel = ((y - y_fma).abs().max() / y_fma.abs().max()).item()
    times = {1: [], 0: []}
    for knob in (1, 0):
        for _ in range(10):
            run(knob)
    torch.cuda.synchronize()
    for _ in range(repeats):        # alternate the two variants window by window
        for knob in (1, 0):
            times[knob].append(window(lambda: run(knob), iters))
    flops = 4.0 * BATCH * HEADS * Lq * Lk * D
    us, us_fma = statistics.median(times[1]), statistics.median(times[0])
    return {'shape': tag, 'dtype': str(dtype).replace('torch.', ''), 'B': BATCH, 'heads': HEADS, 'head_dim': D,
            'Lq': Lq, 'Lk': Lk, 'kernel': kernel, 'default_us': round(us, 2),
            'default_us_min_max': [round(min(times[1]), 2), round(max(times[1]), 2)],
            'fma_us': round(us_fma, 2), 'fma_us_min_max': [round(min(times[0]), 2), round(max(times[0]), 2)],
            'speedup': round(us_fma / us, 2), 'default_tflops': round(flops / us / 1e6, 1),
            'mfma_peak_frac': round(flops / (us * 1e-6) / PEAK_16BIT_FLOPS, 4),
            'max_rel_diff_vs_fma': float(f'{rel:.3g}'), 'iters': iters, 'repeats': repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', choices=['bf16', 'f16'], default='bf16')
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_mha: needs a GPU')
    dtype = torch.bfloat16 if a.dtype == 'bf16' else torch.float16
    for tag, D, Lq, Lk in SHAPES:
        line = json.dumps(bench_shape(tag, D, Lq, Lk, dtype, a.iters, a.repeats))
        print(line, flush=True)
        if a.out:
            with open(a.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
