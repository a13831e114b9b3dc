#!/usr/bin/env python3
"""p7: groups of 64 and of 32 phases in loci of at most 64 phased patterns, from the real front end.  A column that occurs more than
once gets no symmetry break (AlignmentProcessor.c:1767), so locus 1 -- 24 repeats of one column in which all six diploid samples
are heterozygous -- is ONE pattern of 2^6 = 64 phases: 64 phased patterns, the whole wavefront one group.  Locus 2 repeats a column
with five heterozygotes (32 phases) next to a few ordinary columns; three ordinary loci follow.  12 leaves: library variant s, the
lane-per-pattern path of the root sum (add_phases, csrc/gph_locus.h).  Writes p7.ctl / p7.seq (own generator); make_goldens.sh
then runs the real reference on them for p7.trace."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tools"))
import gen_synth  # noqa: E402

LOCI, ITERS = 5, 40
cfg = dict(pops=[2, 2, 2], bands=[(0, 1)], loci=LOCI)
gen_synth.write_ctl(os.path.join(HERE, "p7.ctl"), cfg, "p7.seq", "p7.trace", LOCI, 4242, ITERS, 10, mig_beta=1e-5)
rng = np.random.default_rng(7)
with open(os.path.join(HERE, "p7.seq"), "w") as f:
    f.write(f"{LOCI}\n\n")
    for g in range(LOCI):
        L = 24 if g == 0 else 40
        f.write(f"locus{g + 1} 6 {L}\n")
        base = rng.integers(0, 4, L)
        for d in range(6):
            s = ["TCAG"[b] for b in base]
            if g == 0:
                s = ["Y"] * L                                  # every sample heterozygous in the one, repeated column
            else:
                for i in rng.choice(np.arange(20, L), 2, replace=False):
                    s[i] = "TCAG"[rng.integers(0, 4)]
                if g == 1:
                    s[:20] = ["R" if d < 5 else "A"] * 20      # the repeated column with five hets
                elif d == g:
                    s[30] = "K"                                # one het in a column of its own: broken by symmetry, 1 phase
            f.write(f"s{d}\t{''.join(s)}\n")
        f.write("\n")
