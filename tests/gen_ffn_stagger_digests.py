"""Records tests/golden/ffn_stagger_digests.json: the SHA-256 of the output buffer of every case of
tests/ffn_stagger_cases.py (grid cap 0), from the library that is loaded -- run it on the GPU against a build of the
commit that test_ffn_stagger_gpu.py is to hold later changes to:

    KINET_AMD_LIB=/path/to/that/build/libkinet_amd.so python tests/gen_ffn_stagger_digests.py <commit> [out.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ffn_stagger_cases as C  # noqa: E402


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, 'golden', 'ffn_stagger_digests.json')
    from kinet_amd import _native, kernels
    L = _native.lib()
    L.kinet_ffn_set_debug(0)
    kernels.ffn_grid_cap(0)
    digests, names = {}, set()
    for entry in C.ENTRIES:
        for dn, dt in C.DTYPES.items():
            for F_ in C.FS:
                run = C.Launcher(entry, dt, F_)
                for tiles in C.TILES:
                    for r in C.LAST_ROWS:
                        M = C.rows_of(entry, tiles, r)
                        digests[C.case_key(entry, dn, F_, M)] = C.digest(run.run(M))
                        names.add(kernels.ffn_last_kernel())
    rec = dict(parent_commit=commit, library=L.kinet_version().decode(),
               kernels=sorted(names), sentinel=C.SENTINEL, tail_rows=C.TAIL_ROWS, digests=digests)
    with open(out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'{len(digests)} digests from {sorted(names)} -> {out}')


if __name__ == '__main__':
    main()
