#!/usr/bin/env python
"""Write tests/decode_seeds.py: for every planned call of tests/decode_cases.py whose default seed (crc32 of its name) gives an input
that misses a condition of tests/test_decode_cases.py (a parity-stop call needs an early leaver and a straggler, a fixed-iteration
call must leave every codeword unconverged and away from the all-zero word), the first later seed that meets it.  CPU only: the
oracle is asked.  Run it again whenever the plan changes; test_decode_cases.py fails until the file fits the plan.

    python tools/find_decode_seeds.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "decode_seeds.py")
HEAD = '''"""Seeds of the planned calls of decode_cases.py whose default seed (crc32 of the name) gives an input that misses a condition of
test_decode_cases.py: the first later seed that meets it.  Data, written by tools/find_decode_seeds.py; decode_cases.py reads it."""
SEEDS = {
'''


def main():
    if not os.path.exists(OUT):
        with open(OUT, "w") as f:
            f.write(HEAD + "}\n")
    import oracle
    oracle.lib()
    from conftest import awgn_llr
    import decode_cases as D
    D.SEEDS.clear()  # the search starts from every call's default seed
    out = {}
    for c in D.build_plan():
        if not D.conditions(c, oracle, awgn_llr):
            continue
        for k in range(1, 400):
            c2 = c._replace(seed=(c.seed + k) & 0x7FFFFFFF)
            if not D.conditions(c2, oracle, awgn_llr):
                out[c.name] = c2.seed
                break
        else:
            raise SystemExit("no seed within 400 meets the conditions of %s: change its operating point in the plan" % c.name)
    with open(OUT, "w") as f:
        f.write(HEAD)
        for k in sorted(out):
            f.write("    %r: %d,\n" % (k, out[k]))
        f.write("}\n")
    print("%s: %d of %d planned calls carry another seed" % (OUT, len(out), len(D.build_plan())))


if __name__ == "__main__":
    main()
