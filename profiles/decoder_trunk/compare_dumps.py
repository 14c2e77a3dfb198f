#!/usr/bin/env python3
"""The lines of hash_outputs.py that a checkout does not reproduce against itself, compared numerically:

    python profiles/decoder_trunk/compare_dumps.py hashes.txt PARENT_1 PARENT_2 NEW

reads the tensors that `hash_outputs.py --dump DIR WORDS` wrote in three runs and prints, per line, the largest deviation relative
to the largest magnitude: parent run 1 against parent run 2, and parent run 1 against the new checkout, side by side.  The second
may not exceed the first; the last line says whether any does."""
import os
import sys

import numpy as np


def rel(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.abs(a - b).max() / max(np.abs(a).max(), 1e-300))


def main(hashes, p1, p2, new):
    labels = {ln[:3]: ln[4:ln.index(":")] for ln in open(hashes) if " sha256 " in ln}
    worst = 0
    for f in sorted(os.listdir(p1)):
        a, b, c = (np.load(os.path.join(d, f)) for d in (p1, p2, new))
        pp, pn = rel(a, b), rel(a, c)
        worst += pn > pp
        print(f"{f[:-4]} {labels[f[:3]]}: parent/parent {pp:.3e}  parent/new {pn:.3e}  {'ok' if pn <= pp else 'ABOVE'}")
    print(f"{worst} line(s) above the parent's own deviation")


if __name__ == "__main__":
    main(*sys.argv[1:5])
