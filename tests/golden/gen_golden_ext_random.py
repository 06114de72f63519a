#!/usr/bin/env python3
"""Generate ext_random.npz: the reference's own C++ core (oracle/_ref, built by oracle/Makefile next to the reference)
on the seeded two-batch inputs of tests/test_oracle_ext.py::test_restatement_vs_ref_random, inputs and outputs both
stored, so that the test compares the restatement against the reference core wherever oracle/_ref was not built.
No reference source is copied: the fixture is data."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))

from oracle import capi  # noqa: E402
from helpers import ext_random_case  # noqa: E402


def main():
    capi.build()
    assert capi.have_ref(), "oracle/_ref is not built: the fixture can only be generated next to the reference"
    out = {}
    for seed in (3, 4):
        c = ext_random_case(seed)
        nb = capi.ref_radius_neighbors(c["q"], c["s"], c["q_lengths"], c["s_lengths"], c["radius"])
        sp, sl = capi.ref_grid_subsampling(c["s"], c["s_lengths"], c["voxel"])
        out.update({f"q_{seed}": c["q"], f"s_{seed}": c["s"], f"neighbors_{seed}": nb.astype(np.int32),
                    f"s_points_{seed}": sp, f"sub_lengths_{seed}": sl})
    np.savez_compressed(os.path.join(HERE, "ext_random.npz"), **out)


if __name__ == "__main__":
    main()
