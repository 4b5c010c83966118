"""Generate tests/golden/grid1460.npz from the reference's data (build container only):

    python tests/golden/make_grid1460.py

Two columns of the reference's ``opacities/grid1460.csv``, in file order: ``temperature_K`` and ``pressure_bar`` of the 1 460
P-T points of its cross-section directories.  Data only:
tests/test_ck_premixed.py selects the rows of the 2121-point chemistry table (chemistry.npz, ``t2121/*``) by them, as the
reference's ``compute_sum_molecular`` does (opacity_factory.py:1577-1584).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tools"))

import ref_shim  # noqa: E402

if __name__ == "__main__":
    grid = np.genfromtxt(os.path.join(ref_shim.REF_ROOT, "reference", "opacities", "grid1460.csv"), delimiter=",", names=True)
    assert grid.shape == (1460,) and np.array_equal(grid["file_number"], np.arange(1, 1461))
    np.savez_compressed(os.path.join(HERE, "grid1460.npz"), temperature_K=np.asarray(grid["temperature_K"], dtype=float),
                        pressure_bar=np.asarray(grid["pressure_bar"], dtype=float))
    print("wrote grid1460.npz: %d points, %d temperatures, %d pressures"
          % (grid.size, np.unique(grid["temperature_K"]).size, np.unique(grid["pressure_bar"]).size))
