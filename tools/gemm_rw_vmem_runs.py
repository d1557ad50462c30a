#!/usr/bin/env python3
"""Check the vector-memory instruction counts that gemm_rw_kernel's counted waits rely on, in the
built code of every instantiation.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S kinet_amd/csrc/gemm_rw.hip -o rw.s
    python tools/gemm_rw_vmem_runs.py rw.s [-v]

The ring's waits (s_waitcnt vmcnt(k * (D + S)) and kin) assume that between the DMA of two row tiles
every lane issues S buffer stores, and that a tile's DMA is D instructions.  Per kernel, the buffer
stores (s) and LDS-DMA loads (d) are listed in text order as runs; S and D are recomputed here from the
template arguments in the symbol name (RwCfg and the constants next to store_pending).  A run of stores
shorter than S, or a run of DMA that is no multiple of D, means the optimiser merged or dropped
instructions the waits count on: the waits would then retire a tile early.  A run may be longer than
S: a store under a lane-divergent select is emitted on both sides of a branch, and the kernels that
can store 32-column heads through the LDS transpose carry both forms of the store (more stores than
counted only make a wait stricter).  Exit status 1 if any kernel fails."""
import re
import sys


def template_args(symbol):
    s = re.search(r'gemm_rw_kernelI(.*?)EEvNS_8GemmArgsEi', symbol).group(1)
    toks = re.findall(r'NS_6bf16_tE|DF16_|f|S\d_|Li\d+E|Lb[01]E', s)
    types = [t for t in toks if not t.startswith('L')]
    return types, [int(t[2:-1]) for t in toks if t.startswith('L')]


def counts(types, n):
    """(D, S) of RwCfg<...> / gemm_rw_kernel<T, TO, KC, NT, BMR, NS, HAS_R, LN, HAS_A2, CR, PREP, OCC, NW>."""
    KC, NT, BMR, NS, HAS_R, LN, A2, CR, PREP, OCC, NW = n
    opb = NW * 64 * 16
    a_ops = -(-BMR * KC * 64 // opb)
    r_ops = -(-BMR * NW * NT * 32 // opb) if HAS_R else 0
    D = a_ops * (2 if A2 else 1) + r_ops + 1 + (BMR // 16 if PREP else 0)
    size = 4 if types[1] == 'f' else 2
    NC, epc = NT * 4, 16 // size
    su = epc if (NC % epc == 0 and not (KC == 9 and NT == 2 and not LN)) else 4
    return D, BMR // 16 * (2 if PREP else NC // su)


def kernels(path):
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r'^(_Z\S*gemm_rw_kernel\S*):', ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif ln.startswith('.Lfunc_end'):
            cur = None
        elif cur is not None:
            cur.append(ln)
    return out


def runs(lines):
    seq = []
    for ln in lines:
        if re.match(r'\s+buffer_store_', ln):
            t = 's'
        elif re.match(r'\s+buffer_load_\S+\s.*\blds\b', ln):
            t = 'd'
        else:
            continue
        if seq and seq[-1][0] == t:
            seq[-1][1] += 1
        else:
            seq.append([t, 1])
    return seq


def main(path, verbose):
    ks = kernels(path)
    bad = 0
    for sym, lines in ks.items():
        types, n = template_args(sym)
        D, S = counts(types, n)
        r = runs(lines)
        short = [f'{c}{t}' for t, c in r if (c < S if t == 's' else c % D)]
        bad += bool(short)
        if short or verbose:
            print(f'{"/".join(types)} {n} D={D} S={S}: ' + ' '.join(f'{c}{t}' for t, c in r) +
                  (f'   <-- {" ".join(short)}' if short else ''))
    print(f'{len(ks)} kernels, {bad} with a run of fewer than S stores or a run of DMA that is no multiple of D')
    return 1 if bad or not ks else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], '-v' in sys.argv[2:]))
