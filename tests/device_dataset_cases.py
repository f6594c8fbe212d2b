"""The molecules the DeviceDataset tests share (host and GPU)."""
import numpy as np


def odd_molecule():
    """Three atoms, edges 0->1, 1->0, 1->2: an odd edge count, and 1->2 has no reverse (not symmetric)."""
    ei = np.array([[0, 1, 1], [1, 0, 2]], dtype=np.int64)
    rng = np.random.default_rng(8)
    return {"x": np.array([6, 8, 1], dtype=np.int64), "atom_pos": rng.normal(size=(3, 3)).astype(np.float32),
            "edge_index": ei, "edge_num": 3, "triplet_num": 1,
            "edge_attr": (0.1 * rng.standard_normal((3, 338))).astype(np.float32), "y": np.float32(0.25)}


def pair_molecule():
    """Two atoms joined both ways: E = 2, no triplet."""
    ei = np.array([[0, 1], [1, 0]], dtype=np.int64)
    rng = np.random.default_rng(7)
    return {"x": np.array([7, 1], dtype=np.int64), "atom_pos": rng.normal(size=(2, 3)).astype(np.float32),
            "edge_index": ei, "edge_num": 2, "triplet_num": 0,
            "edge_attr": (0.1 * rng.standard_normal((2, 338))).astype(np.float32), "y": np.float32(-1.5)}


def mixed_molecules():
    """The ten molecules of the GPU tests: 6 S160, 1 S5A (a larger slab), the 2-atom molecule (a slab smaller
    than any copy chunk) between large ones, the 3-atom non-symmetric one (odd E: every later slab is 8-byte
    aligned only), and one more S160 behind it."""
    from x2gnn.synth import synthetic_molecules

    return (synthetic_molecules(6, "S160", seed=31) + synthetic_molecules(1, "S5A", seed=32)
            + [pair_molecule(), odd_molecule()] + synthetic_molecules(1, "S160", seed=33))
