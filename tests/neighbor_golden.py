"""Loader for tests/golden/neighbors/*.npz (written by tools/gen_golden_neighbors.py from the reference with a non-default neighbor_filter)."""
from __future__ import annotations

import glob
import os
from typing import NamedTuple, Optional

import numpy as np

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "neighbors")


class NbGolden(NamedTuple):
    name: str
    filter: np.ndarray      # [3, 3] f32
    g_ratio: float
    Tmax: float
    training: bool
    map_designs: np.ndarray  # [B,1,H,W] f32
    start_maps: np.ndarray
    goal_maps: np.ndarray
    cost_maps: np.ndarray
    histories: np.ndarray
    paths: np.ndarray        # int64
    sel_log: np.ndarray      # [B, t_batch + 1] flat index selected at each loop step of the reference
    t_batch: int
    target: Optional[np.ndarray]
    grad_cost: Optional[np.ndarray]
    inter_hist: Optional[np.ndarray]  # [T + 1, B, 1, H, W] the reference's intermediate_results
    inter_path: Optional[np.ndarray]

    @property
    def max_iters(self) -> int:
        W = self.map_designs.shape[-1]
        return int((self.Tmax if self.training else 1.0) * W * W)


def names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DIR, "*.npz")))


def _unpack(bits, B, H, W):
    return np.unpackbits(bits, axis=-1)[..., :H * W].reshape(bits.shape[:-1] + (1, H, W))


def load(name: str) -> NbGolden:
    z = np.load(os.path.join(DIR, name + ".npz"))
    B, H, W = int(z["B"]), int(z["H"]), int(z["W"])
    maps = _unpack(z["map_bits"], B, H, W).astype(np.float32)
    eye = np.eye(H * W, dtype=np.float32)
    start = eye[z["start_idx"]].reshape(B, 1, H, W)
    goal = eye[z["goal_idx"]].reshape(B, 1, H, W)
    return NbGolden(
        name=name, filter=z["filter"].astype(np.float32), g_ratio=float(z["g_ratio"]), Tmax=float(z["Tmax"]), training=bool(z["training"]),
        map_designs=maps, start_maps=start, goal_maps=goal, cost_maps=z["cost"].astype(np.float32) if "cost" in z else maps,
        histories=_unpack(z["hist_bits"], B, H, W).astype(np.float32), paths=_unpack(z["path_bits"], B, H, W).astype(np.int64),
        sel_log=z["sel_log"], t_batch=int(z["t_batch"]),
        target=_unpack(z["target_bits"], B, H, W).astype(np.float32) if "target_bits" in z else None,
        grad_cost=z["grad_cost"] if "grad_cost" in z else None,
        inter_hist=_unpack(z["inter_hist_bits"], B, H, W).astype(np.float32) if "inter_hist_bits" in z else None,
        inter_path=_unpack(z["inter_path_bits"], B, H, W).astype(np.float32) if "inter_path_bits" in z else None,
    )


def mask_of(filt) -> int:
    """bit r*3+c <=> filter cell (r, c) is 1 (include/nastar.h NASTAR_NEIGHBORS_*)"""
    f = np.asarray(filt, np.float32).reshape(-1)
    return int(sum(1 << i for i in range(9) if f[i] == 1.0))
