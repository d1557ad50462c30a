"""A/B of the fused stem + max-pool launch (kinet_stem_pool_image) against kinet_stem_conv_image
followed by kinet_maxpool2d_3x3s2, 800 x 1333 bf16 at batch 28 and 16: HIP events, the median
of 7 alternating windows per variant, and a bit-for-bit comparison of the two results.
usage: python tools/stem_pool_ab.py [--batches 28,16] [--iters 20] [--windows 7] [--seg 0]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kinet_amd import kernels as K  # noqa: E402


def time_call(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='28,16')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--seg', default='0', help='comma list of seg_tiles values for the fused launch (0 = its own choice)')
    a = ap.parse_args()
    dt, H, W = torch.bfloat16, 800, 1333
    g = torch.Generator().manual_seed(0)
    w = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    scale, bias = (torch.rand(64, generator=g) + 0.5).cuda(), (torch.randn(64, generator=g) * 0.1).cuda()
    wp = K.pack_stem_weight(w.cuda(), dt, 24)
    for B in [int(b) for b in a.batches.split(',')]:
        img = torch.randn(B, 3, H, W, generator=g).cuda()
        variants = {'stem': lambda: K.stem_conv_image(img, wp, scale, bias, dt),
                    'stem + pool': lambda: K.maxpool_3x3s2(K.stem_conv_image(img, wp, scale, bias, dt))}
        for seg in [int(s) for s in a.seg.split(',')]:
            variants[f'fused seg_tiles={seg}'] = lambda seg=seg: K.stem_pool_image(img, wp, scale, bias, dt, seg)
        two = variants['stem + pool']()
        for name in variants:
            if name.startswith('fused'):
                print(f'batch {B}: {name} equals stem + pool bit for bit: {torch.equal(variants[name](), two)}', flush=True)
        times = {name: [] for name in variants}
        for _ in range(a.windows):
            for name, fn in variants.items():
                times[name].append(time_call(fn, a.iters))
        for name, ts in times.items():
            print(f'stem_pool batch {B} {H}x{W} bf16: {name:22s} median {statistics.median(ts):7.1f} us  '
                  f'min {min(ts):7.1f}  max {max(ts):7.1f}', flush=True)


if __name__ == '__main__':
    main()
