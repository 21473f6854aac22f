#!/usr/bin/env python3
"""Record the REAL reference's answers on the inputs of tests/test_oracle_vs_ref.py and tests/test_gpu_vs_reference.py.

Needs the reference build, oracle/_ref (make -C oracle ref REF=<reference tree>):
    make -C oracle ref && python tests/golden/gen_ref_digests.py

Those inputs are seeded (up to 1.3e6 blocks) and their outputs too large to store, so ref_digests.json keeps the SHA-256 of
each output array's bytes (little-endian, C order) with its shape and dtype; the tests compare the same digest of what the
oracle or the kernels computed.  Fixtures are recorded results; no reference source is stored.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from _util import Reference, dct_edge_blocks, digest, satd_edge_blocks   # noqa: E402
import test_gpu_vs_reference as G                                  # noqa: E402
import test_oracle_vs_ref as O                                     # noqa: E402


def main():
    ref = Reference()
    out = {}
    out["oracle_vs_ref.table"] = digest(ref.table())
    out["oracle_vs_ref.dct32_fwd"] = digest(ref.dct32_fwd(O._mixed(3000, 1024, 11)))
    x = O._mixed(40, 1024, 21)
    out["oracle_vs_ref.dct32_pass"] = digest(np.stack([ref.dct32_pass(blk, shift) for blk in x for shift in (4, 11)]))
    out["oracle_vs_ref.satd8x8"] = digest(ref.satd8x8(O._mixed(100000, 64, 31)))
    out["gpu_vs_reference.dct32_fwd"] = digest(ref.dct32_fwd(G._mixed(80000, 30000, 10000, 1024, 0x51, dct_edge_blocks()[0])))
    out["gpu_vs_reference.satd8x8"] = digest(ref.satd8x8(G._mixed(900000, 300000, 100000, 64, 0x52, satd_edge_blocks()[0])))
    for shift in (4, 11):
        x = G._mixed(600, 300, 84, 1024, 0x53 + shift, dct_edge_blocks()[0])[:1000]
        out["gpu_vs_reference.dct32_pass_%d" % shift] = digest(np.stack([ref.dct32_pass(blk, shift) for blk in x]))
    out["gpu_vs_reference.fused_forward"] = digest(ref.dct32_fwd(G._mixed(6000, 1500, 500, 1024, 0x54, dct_edge_blocks()[0])))
    with open(os.path.join(HERE, "ref_digests.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("ref_digests.json written: %d records" % len(out))


if __name__ == "__main__":
    main()
