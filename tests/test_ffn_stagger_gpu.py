"""The 8-wave x 32-row FFN kernel (ffn_fused_rt2_kernel, plain and with the attention out-projection in front) must
compute, bit for bit, what it computed before its waves 4-7 were staggered against their SIMD partners and its ring
was recycled by halves (csrc/ffn_sched.h) -- on the shapes where that schedule can go wrong: one hidden chunk, as
many chunks as ring slots, chunk counts that are multiples of neither, last tiles that leave waves 4-7 out of range
or cut through wave 4, and one workgroup walking every tile (tests/ffn_stagger_cases.py).

(a) kinet_ffn_fused: the output equals the run under debug bit 8, the 8-wave x 16-row ffn_fused_kernel, which keeps
    the same sums in the same order by design; kinet_ffn_last_kernel proves the two runs were different kernels.
(b) both entries: the SHA-256 of the whole output buffer (sentinel rows included) equals the digest recorded from the
    library of the commit named in tests/golden/ffn_stagger_digests.json (tests/gen_ffn_stagger_digests.py), under
    every grid cap.  This holds the kernels to that commit, not to themselves.

The issue that asked for this test gave M = 256 t + r with 1, 2 and 5 tiles; kinet_ffn_fused only takes the kernel
under test from 16384 rows, so its cases carry 64 full tiles more (ffn_stagger_cases.rows_of)."""
import json
import os

import pytest
import torch

import ffn_stagger_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ffn_stagger_digests.json')
RT2 = {'ffn': 'ffn_fused_rt2_kernel<256>', 'attn_out_ffn': 'ffn_fused_rt2_kernel<256, true>'}
RT1 = 'ffn_fused_kernel<256, 1, 8>'
FFN_DBG_8W_RT1 = 8


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture
def knobs():
    from kinet_amd import _native, kernels
    L = _native.lib()
    old = L.kinet_ffn_set_debug(0), kernels.ffn_grid_cap(0)

    class Knobs:
        debug = staticmethod(L.kinet_ffn_set_debug)
        cap = staticmethod(kernels.ffn_grid_cap)
        last = staticmethod(kernels.ffn_last_kernel)
    yield Knobs
    L.kinet_ffn_set_debug(old[0])
    kernels.ffn_grid_cap(old[1])


def same_bytes(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize('F_', C.FS)
@pytest.mark.parametrize('dtype_name', sorted(C.DTYPES))
@pytest.mark.parametrize('entry', C.ENTRIES)
def test_stagger_bit_identical(knobs, golden, entry, dtype_name, F_):
    run = C.Launcher(entry, C.DTYPES[dtype_name], F_)
    for tiles in C.TILES:
        for r in C.LAST_ROWS:
            M = C.rows_of(entry, tiles, r)
            tag = C.case_key(entry, dtype_name, F_, M)
            outs = {}
            for cap in C.CAPS:
                knobs.cap(cap)
                outs[cap] = run.run(M)
                assert knobs.last() == RT2[entry], f'{tag} cap {cap}: {knobs.last()} served the call'
            # (b) the commit the digests were recorded from, under every cap
            got = C.digest(outs[0])
            print(f'{tag}: {got[:16]} (golden {golden["digests"][tag][:16]})')
            assert got == golden['digests'][tag], f'{tag}: the output differs from commit {golden["parent_commit"]}'
            for cap in C.CAPS[1:]:
                assert same_bytes(outs[cap], outs[0]), f'{tag}: grid cap {cap} changed the output'
            assert (outs[0][M:] == C.SENTINEL).all(), f'{tag}: rows past M were written'
            # (a) the 16-row kernel: same sums, same order
            if entry == 'ffn':
                knobs.cap(0)
                knobs.debug(FFN_DBG_8W_RT1)
                try:
                    ref = run.run(M)
                    assert knobs.last() == RT1, f'{tag}: {knobs.last()} served the reference call'
                finally:
                    knobs.debug(0)
                assert same_bytes(outs[0], ref), f'{tag}: differs from {RT1}'
