"""Generates tests/golden/ref_random_clouds.npz: outputs of the reference's own native code (oracle/_ref) on the seeded
random clouds of tests/test_oracle_native.py (random_clouds): per case the subsampled points and lengths, and the radius
search table in the canonical (d2, index) order.  Needs oracle/_ref built (make -C oracle ref with the reference tree)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import native  # noqa: E402
from test_oracle_native import random_clouds  # noqa: E402


def main():
    ref = native.reference()
    assert ref is not None, 'oracle/_ref not built'
    out = {}
    for key, pts, lens, voxel in random_clouds():
        pr, lr = ref.grid_subsampling(pts, lens, np.float32(voxel))
        ir = native.canonicalize_ties(pr, pts, ref.radius_neighbors(pr, pts, lr, lens, np.float32(voxel * 2.125)))
        out[key + '/points'], out[key + '/lengths'], out[key + '/neighbors'] = pr, lr, ir
    np.savez_compressed(os.path.join(HERE, 'ref_random_clouds.npz'), **out)


if __name__ == '__main__':
    main()
