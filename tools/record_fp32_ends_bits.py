"""Record the output bits of the fp32 ends (csrc/small.hip: output head, input conv, 1x1 quant convs, conv weight packers, GELUs) on one
MI355X: every case of tests/fp32_ends_cases.py through the public C entries of the library that is loaded (SDMI_LIB_PATH picks another
build), SHA-256 of the inputs and of the outputs per case, and the commit the library was built from.

    python tools/record_fp32_ends_bits.py [--commit HASH] [--out tests/golden/fp32_ends_parent_bits.json]

Every case runs twice; a case whose two digests differ is not deterministic and nothing is written.  tests/test_fp32_ends_bits_gpu.py
compares a build against this record: re-record only when the bits are meant to move (a compiler upgrade)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default=None, help='the commit the loaded library was built from (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'fp32_ends_parent_bits.json'))
    args = ap.parse_args()
    import fp32_ends_cases as FC
    commit = args.commit or subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    cases, unstable = {}, []
    for name in FC.CASES:
        first, second = FC.run_case(name), FC.run_case(name)
        print(f'{name:28s} {len(FC.launches(name)):3d} launches  {first[:16]}  {"ok" if first == second else "DIFFERS BETWEEN TWO RUNS"}', flush=True)
        if first != second:
            unstable.append(name)
        cases[name] = dict(output_sha256=first, input_sha256=FC.input_digest(name), commit=commit)
    if unstable:
        print(f'not written: {len(unstable)} case(s) gave two different digests: {", ".join(unstable)}', file=sys.stderr)
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(cases, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'wrote {len(cases)} cases to {args.out}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
