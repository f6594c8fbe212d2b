"""The molecules and index lists of the padding tests."""
import numpy as np

from device_dataset_cases import mixed_molecules

FILLERS = (1, 2)

# positions in molecules(): 0-5 S160, 6 S5A, 7 the 2-atom molecule, 8 S160, 9 / 10 / 11 of 5 / 9 / 13 atoms.
# Three molecules per list; the lists differ in real N, in E and in T (test_padding.py checks it); list 0 has the
# 2-atom molecule first, list 1 the S5A molecule (the most rows), list 4 the fewest rows.
INDEX_LISTS = [[7, 0, 1], [6, 2, 9], [3, 10, 4], [11, 5, 8], [0, 9, 11]]


def molecules():
    """mixed_molecules() without its non-symmetric molecule, plus three smaller ones."""
    from x2gnn.synth import molecule_from_geometry, random_geometry

    mols = [m for i, m in enumerate(mixed_molecules()) if i != 8]
    rng = np.random.default_rng(5)
    for k in (5, 9, 13):
        z, pos = random_geometry(rng, 1.8, n_heavy=(k + 1) // 2, n_h=k // 2)
        mols.append(molecule_from_geometry(z, pos, feat_rng=np.random.default_rng(k), y=0.3 * k - 2.0))
    return mols
