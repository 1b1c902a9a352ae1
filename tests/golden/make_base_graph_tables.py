#!/usr/bin/env python3
"""Generate tests/golden/base_graph_tables.npz: TS 38.212 Tables 5.3.2-2 (BG1) and 5.3.2-3 (BG2) as the reference's
get_3gpp_base_graph.m states them -- one row per edge: row, column, then the shift for set index 0..7 (int16).

tests/test_tables.py compares the build's tables with this file entry by entry, so the check runs wherever the
repository does.  Run with the path of a checkout of the reference:
    python tests/golden/make_base_graph_tables.py <reference checkout>/get_3gpp_base_graph.m
"""
import os
import re
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "base_graph_tables.npz")


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    txt = open(sys.argv[1]).read()
    tabs = re.findall(r"table\{(\d)\}\s*=\s*\[(.*?)\];", txt, re.S)
    assert [bg for bg, _ in tabs] == ["1", "2"], [bg for bg, _ in tabs]
    out = {}
    for bg, body in tabs:
        rows = np.array([[int(t) for t in ln.split()] for ln in body.strip().splitlines() if ln.strip()], dtype=np.int16)
        assert rows.ndim == 2 and rows.shape[1] == 10, rows.shape
        out["bg%s" % bg] = rows
    np.savez_compressed(OUT, **out)
    print(OUT, {k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
