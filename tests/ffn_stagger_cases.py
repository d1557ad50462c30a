"""Cases, operands and the launch of tests/test_ffn_stagger_gpu.py, shared with the generator of its golden digests
(tests/gen_ffn_stagger_digests.py) so that both run byte for byte the same calls.

D = 256; entries kinet_ffn_fused ('ffn') and kinet_attn_out_ffn_fused ('attn_out_ffn'); bf16 and f16; F = 32 (one
hidden chunk: waves 4-7 have only the phase B they run behind their phase A), 64, 96 (as many chunks as the ring has
slots), 160 and 1024.  Rows: `tiles` in {1, 2, 5} row tiles of 256, the last one holding r in {5, 133, 251} rows (5:
waves 4-7 are out of range altogether; 133: the range ends inside wave 4).  kinet_ffn_fused takes the 8-wave x
32-row kernel only from 16384 rows (ffn_plan.h), so its cases stand on 64 full tiles more: M = 256 (64 + tiles - 1)
+ r; the attention entry runs on that kernel at any M: M = 256 (tiles - 1) + r.  Grid caps 0 (one tile per
workgroup), 1 (one workgroup walks every tile: the ring, the pre-chunks and the roles' lag carried from tile to
tile) and 2 (an uneven split).

Operands are seeded randn made on the CPU (the same on every machine), LayerNorms on; the output is an (M + 8, D)
buffer filled with a sentinel, hashed whole."""
import hashlib

import torch

D = 256
ENTRIES = ('ffn', 'attn_out_ffn')
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16}
FS = (32, 64, 96, 160, 1024)
TILES = (1, 2, 5)
LAST_ROWS = (5, 133, 251)
CAPS = (0, 1, 2)
RT2_BASE_TILES = 64          # kFfnRt2MinRows / 256
SENTINEL = 77.0
TAIL_ROWS = 8
MAX_ROWS = 256 * (RT2_BASE_TILES + max(TILES))


def rows_of(entry, tiles, r):
    return 256 * ((RT2_BASE_TILES if entry == 'ffn' else 0) + tiles - 1) + r


def case_key(entry, dtype_name, F_, M):
    return f'{entry}-{dtype_name}-F{F_}-M{M}'


def operands(F_):
    """CPU f32 operands for hidden width F_ (row operands MAX_ROWS long: a case takes the first M rows)."""
    g = torch.Generator().manual_seed(1000 + F_)

    def rn(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale
    return dict(x=rn(MAX_ROWS, D), A=rn(MAX_ROWS, D), R=rn(MAX_ROWS, D),
                Wo=rn(D, D, scale=D ** -0.5), bo=rn(D, scale=0.1), g1=1 + rn(D, scale=0.1), be1=rn(D, scale=0.1),
                W1=rn(F_, D, scale=D ** -0.5), b1=rn(F_, scale=0.1), W2=rn(D, F_, scale=F_ ** -0.5), b2=rn(D, scale=0.1),
                g2=1 + rn(D, scale=0.1), be2=rn(D, scale=0.1))


class Launcher:
    """The operands of one (entry, dtype, F) on the GPU, packed once; run(M) -> the whole sentinel-filled buffer."""

    def __init__(self, entry, dtype, F_):
        from kinet_amd import _native as N
        self.N, self.entry, self.dtype, self.F = N, entry, dtype, F_
        self.code, self.st = N.dtype_code(dtype), N.stream(torch.device('cuda:0'))
        d = operands(F_)
        self.f32 = {k: d[k].cuda() for k in ('bo', 'g1', 'be1', 'b1', 'b2', 'g2', 'be2')}
        self.rows = {k: d[k].to(dtype).cuda() for k in (('x',) if entry == 'ffn' else ('A', 'R'))}
        w = {k: d[k].to(dtype).cuda().contiguous() for k in ('Wo', 'W1', 'W2')}
        if entry == 'ffn':
            self.packed = torch.empty(2 * D * F_, dtype=dtype, device='cuda')
            N.call('kinet_ffn_pack', N.ptr(w['W1']), N.ptr(w['W2']), N.ptr(self.packed), D, F_, self.code, self.st)
        else:
            self.packed = torch.empty(D * D + 2 * D * F_, dtype=dtype, device='cuda')
            N.call('kinet_ffn_pack_attn', N.ptr(w['Wo']), N.ptr(w['W1']), N.ptr(w['W2']), N.ptr(self.packed), D, F_,
                   self.code, self.st)

    def run(self, M):
        N, p, f = self.N, self.N.ptr, self.f32
        y = torch.full((M + TAIL_ROWS, D), SENTINEL, dtype=self.dtype, device='cuda')
        if self.entry == 'ffn':
            N.call('kinet_ffn_fused', p(self.rows['x']), D, p(self.packed), p(f['b1']), p(f['b2']), p(f['g2']), p(f['be2']),
                   1e-5, p(y), D, M, D, self.F, self.code, self.st)
        else:
            N.call('kinet_attn_out_ffn_fused', p(self.rows['A']), D, p(self.rows['R']), D, p(self.packed), p(f['bo']),
                   p(f['g1']), p(f['be1']), 1e-5, p(f['b1']), p(f['b2']), p(f['g2']), p(f['be2']), 1e-5, p(y), D, M, D,
                   self.F, self.code, self.st)
        torch.cuda.synchronize()
        return y


def digest(y):
    return hashlib.sha256(y.cpu().contiguous().view(torch.int16).numpy().tobytes()).hexdigest()
