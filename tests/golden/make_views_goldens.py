#!/usr/bin/env python3
"""Generate tests/golden/views.npz from the reference's own utils/visualizer.py (threeviews_log, volume_log), run on the CPU.

Run in the dev container only:   python tests/golden/make_views_goldens.py

utils/visualizer.py imports wandb and tqdm at module level and never calls them on these paths: empty stand-ins are
installed for the import.  matplotlib runs on the Agg backend with `plt.imshow` replaced by a recorder and `plt.savefig` by
a no-op, inside a temporary working directory (volume_log reads its joints from `./1.txt` and both loggers create
directories).  Only the input and the arrays the reference passed to imshow are stored:

x          (2, 2, 12, 10, 14) float32, about half of it negative
joints     (24, 3) (d, h, w): every 2 x 2 mark stays inside its image
tv_front   (10, 14), tv_top (12, 14), tv_left (10, 12)   threeviews_log(x): plane [0, -1], normalised and rotated
vl_front   (10, 14), vl_top (12, 14), vl_left (12, 10)   volume_log(x): plane [0, 0] sums with the joint marks
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = "/root/reference"


def main():
    sys.dont_write_bytecode = True
    sys.path.insert(0, REF_ROOT)
    for name in ("wandb", "tqdm"):
        sys.modules[name] = types.ModuleType(name)
    import matplotlib

    matplotlib.use("Agg")
    import matplotlib.pyplot as plt

    from utils import visualizer as RV

    shown = []
    plt.imshow = lambda im, *a, **k: shown.append(np.array(im, copy=True))
    plt.savefig = lambda *a, **k: None

    g = np.random.Generator(np.random.PCG64(2025))
    x = (g.standard_normal((2, 2, 12, 10, 14)) * 1.5 - 0.2).astype(np.float32)
    joints = np.stack([g.integers(0, 11, 24), g.integers(0, 9, 24), g.integers(0, 13, 24)], axis=1).astype(np.float64)
    joints += g.random((24, 3)) * 0.9          # fractional coordinates: the reference truncates them with int()
    out = {"x": x, "joints": joints}

    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            np.savetxt("./1.txt", joints)
            joints_read = np.loadtxt("./1.txt")
            assert np.array_equal(joints_read, joints), "savetxt / loadtxt must round-trip the joints"
            # threeviews_log clamps the array it is given in place (a CPU tensor shares memory with .numpy()): hand it a copy
            RV.threeviews_log(torch.from_numpy(x.copy()), "./tv", "golden", 0)
            assert len(shown) == 3
            out.update(tv_front=shown[0], tv_top=shown[1], tv_left=shown[2])
            del shown[:]
            RV.volume_log(torch.from_numpy(x.copy()), "./vl", "golden", 0)
            assert len(shown) == 3
            out.update(vl_front=shown[0], vl_top=shown[1], vl_left=shown[2])
        finally:
            os.chdir(cwd)
    for k in ("tv_front", "tv_top", "tv_left"):
        assert np.isfinite(out[k]).all() and out[k].max() == 1.0, k     # a positive maximum in every view: no 0 / 0
    for k, v in out.items():
        print(k, v.shape, v.dtype)
    path = os.path.join(HERE, "views.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
