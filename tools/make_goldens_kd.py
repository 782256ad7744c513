#!/usr/bin/env python3
"""Generate tests/golden/kd_order.npz: what scikit-learn's own KDTree makes of the adversarial voxel lists of tests/kd_lists.py.

Run with the reference's interpreter (Python 3.9, scikit-learn 0.24.2 -- the version is asserted):

    PYTHONDONTWRITEBYTECODE=1 python3.9 tools/make_goldens_kd.py

Imports scikit-learn and tests/kd_lists.py (NumPy only), nothing else.  The fixture holds no voxel lists -- the recipes regenerate
them -- but, per list: the SHA-256 of KDTree(list, leaf_size=30).get_arrays()[1] as little-endian int32, the tree's node count and
the first and last 32 entries of that index array (so that a mismatch says more than "the hash differs").
tests/test_kd_order_host.py holds the oracle's tree to it; tests/test_kd_order_gpu.py holds the device's tree to the oracle's.
"""
import hashlib
import os
import sys

import numpy as np

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "kd_order.npz")
ENDS = 32


def index_sha(idx):
    return hashlib.sha256(np.ascontiguousarray(idx, dtype="<i4").tobytes()).hexdigest()


def main():
    import sklearn
    from sklearn.neighbors import KDTree
    assert sklearn.__version__.startswith("0.24"), sklearn.__version__
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import kd_lists
    lists = [(kd_lists.recipe_id(r), kd_lists.make_list(*r)) for r in kd_lists.recipes()] + sorted(kd_lists.extra_lists().items())
    names, sha, n_nodes, head, tail = [], [], [], [], []
    for name, vox in lists:
        arrays = KDTree(vox.astype(np.float64), leaf_size=30).get_arrays()   # (data, idx_array, node_data, node_bounds)
        idx = np.asarray(arrays[1])
        assert sorted(idx.tolist()) == list(range(len(vox)))
        names.append(name); sha.append(index_sha(idx)); n_nodes.append(len(arrays[2]))
        head.append(idx[:ENDS]); tail.append(idx[-ENDS:])
    np.savez_compressed(OUT, names=np.array(names), sha256=np.array(sha), n_nodes=np.array(n_nodes, np.int32),
                        head=np.array(head, np.int32), tail=np.array(tail, np.int32), sklearn_version=np.array(sklearn.__version__))
    print("%s: %d lists, %d bytes" % (OUT, len(names), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
