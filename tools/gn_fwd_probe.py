#!/usr/bin/env python
"""Time kinet_groupnorm (forward, three launches) at the largest input-projection level, 2 frames x
16700 pixels, d = 288 (groups of 9: straddle kernels) and d = 256 (vector kernels), 32 groups, f32 and
bf16; best of 5 windows of 200 calls: python tools/gn_fwd_probe.py [label]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from kinet_amd import kernels as K
    label = sys.argv[1] if len(sys.argv) > 1 else ''
    for C in (288, 256):
        for dtype in (torch.float32, torch.bfloat16):
            x = (30 + torch.randn(2, 16700, C, device='cuda')).to(dtype)
            g, b = torch.rand(C, device='cuda') + 0.5, torch.randn(C, device='cuda')
            out = torch.empty_like(x)
            fn = lambda: K.groupnorm_nhwc(x, g, b, 32, 1e-5, out=out, out_batch_stride=16700 * C)
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            best = float('inf')
            for _ in range(5):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(200):
                    fn()
                e.record()
                torch.cuda.synchronize()
                best = min(best, s.elapsed_time(e) / 200 * 1e3)
            nbytes = 3 * x.numel() * x.element_size()
            name = str(dtype).replace('torch.', '')
            print(f'{label} groupnorm_nhwc 2 x 16700 x {C} {name}: {best:7.1f} us ({nbytes / best / 1e3:6.0f} GB/s, '
                  f'x twice + y)', flush=True)


if __name__ == '__main__':
    main()
