#!/usr/bin/env python3
"""What the three views of a volume cost.  One JSON line.

    python tools/time_views.py [--calls 30] [--rounds 3] [--host-calls 3] [--shapes 512x128x128,1024x256x256]

Per shape (T, H, W), P = 1, one device, three routes to the three oriented, normalised images of threeviews_log:
  (1) "hip":       hp_volume_views + hp_views_orient on preallocated outputs and workspace (event-timed, host launch cost
                   included), and the same through hiddenpose_amd.visualizer.three_views (allocations included);
  (2) "aten":      clamp_min(0), three amax calls, three maxima, the divisions and the two rotations in ATen on the device;
  (3) "reference": the reference's route: the device-to-host copy of the plane, then the NumPy clamp, reductions and divisions.
(1) and (2) are timed in alternating rounds, the median of `--calls` event-timed calls per round; (3) is a host clock around
`--host-calls` calls.  For (1) the algorithmic bytes (one read of the plane, the slabs written and read once, the views) over
the time of its kernels (the library's per-kernel event times) is set against the read rate of this device, measured as
tools/hbm_bw_probe.py measures it (`sum` over 4 GiB).  The images of (1) are checked against (2) before anything is timed.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hiddenpose_amd import _lib  # noqa: E402
from hiddenpose_amd import visualizer as V  # noqa: E402


def event_median(fn, calls):
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def kernel_profile(fn):
    """The library's per-kernel event timing of one call: {kernel: [launches, ms]}."""
    fn()
    _lib.profile_enable(True)
    _lib.profile_reset()
    fn()
    torch.cuda.synchronize()
    prof = _lib.profile_read()
    _lib.profile_enable(False)
    return {k: [cnt, round(ms, 4)] for k, (cnt, ms) in sorted(prof.items())}


def read_rate():
    """tools/hbm_bw_probe.py's `sum` line: bytes per second of a streaming read of 4 GiB."""
    x = torch.empty(1 << 30, device="cuda")
    x.fill_(1.0)
    x.sum()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        x.sum()
    torch.cuda.synchronize()
    return x.numel() * 4 / ((time.perf_counter() - t0) / 10)


def one_shape(T, H, W, a, rate):
    L = _lib.lib()
    g = torch.Generator().manual_seed(T + H + W)
    x = (torch.randn(1, 1, T, H, W, generator=g) * 1.5 - 0.3).cuda()
    plane = x[0, 0]
    kw = dict(dtype=torch.float32, device="cuda")
    need = L.hp_volume_views_workspace_bytes(1, T, H, W, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    front, top, left, vmax = torch.empty(1, H, W, **kw), torch.empty(1, T, W, **kw), torch.empty(1, T, H, **kw), torch.empty(1, 3, **kw)
    of, ot, ol = torch.empty(1, H, W, **kw), torch.empty(1, T, W, **kw), torch.empty(1, H, T, **kw)
    st = _lib.current_stream_handle(x.device)

    def hip():
        _lib.check(L.hp_volume_views(plane.data_ptr(), front.data_ptr(), top.data_ptr(), left.data_ptr(), vmax.data_ptr(), 1, T, H, W, 0,
                                     ws.data_ptr(), need, st), "hp_volume_views")
        _lib.check(L.hp_views_orient(front.data_ptr(), top.data_ptr(), left.data_ptr(), vmax.data_ptr(), of.data_ptr(), ot.data_ptr(),
                                     ol.data_ptr(), 1, T, H, W, st), "hp_views_orient")

    def hip_module():
        return V.three_views(x, (0, 0))

    def aten():
        v = plane.clamp_min(0)
        f, t, l = v.amax(0), v.amax(1), v.amax(2)
        return f / f.max(), torch.rot90(t / t.max(), 2), torch.rot90(l / l.max(), 3)

    def reference():
        v = plane.cpu().numpy()
        v[v < 0] = 0
        f, t, l = np.max(v, axis=0), np.max(v, axis=1), np.max(v, axis=2)
        return f / np.max(f), np.rot90(t / np.max(t), 2), np.rot90(l / np.max(l), 3)

    hip()
    agree = all(torch.equal(p[0], q.contiguous()) for p, q in zip((of, ot, ol), aten()))
    agree = agree and all(torch.equal(p, q[0]) for p, q in zip(hip_module(), (of, ot, ol)))
    for _ in range(3):
        hip(), hip_module(), aten()
    r_hip, r_mod, r_aten = [], [], []
    for _ in range(a.rounds):
        r_hip.append(event_median(hip, a.calls))
        r_aten.append(event_median(aten, a.calls))
        r_mod.append(event_median(hip_module, a.calls))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.host_calls):
        reference()
    ref_ms = (time.perf_counter() - t0) * 1e3 / a.host_calls
    t0 = time.perf_counter()
    for _ in range(a.host_calls):
        plane.cpu()
    copy_ms = (time.perf_counter() - t0) * 1e3 / a.host_calls
    prof = kernel_profile(hip)
    kernels_ms = sum(ms for _, ms in prof.values())
    vol, views = 4 * T * H * W, 4 * (H * W + T * W + T * H)
    slabs = need - 0     # every slab float is written once and read once (the few per-workgroup maxima included)
    moved = vol + 2 * slabs + 3 * views      # views: written by the combine, read and written by the orientation
    med = statistics.median
    return {"shape": [T, H, W], "images_equal_aten": bool(agree),
            "hip_ms": [round(t, 4) for t in r_hip], "aten_ms": [round(t, 4) for t in r_aten], "hip_module_ms": [round(t, 4) for t in r_mod],
            "median_hip_ms": round(med(r_hip), 4), "median_aten_ms": round(med(r_aten), 4), "median_hip_module_ms": round(med(r_mod), 4),
            "reference_ms": round(ref_ms, 2), "reference_copy_ms": round(copy_ms, 2),
            "hip_kernels_ms": prof, "hip_kernels_total_ms": round(kernels_ms, 4),
            "plane_bytes": vol, "slab_bytes": slabs, "view_bytes": views, "bytes_moved": moved,
            "aten_bytes_moved": 5 * vol + 9 * views,   # clamp reads and writes the plane, each amax reads it again
            "achieved_bytes_per_s": round(moved / (kernels_ms * 1e-3)), "read_rate_bytes_per_s": round(rate),
            "share_of_read_rate": round(moved / (kernels_ms * 1e-3) / rate, 4), "host_bytes_copied": views}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--shapes", type=str, default="512x128x128,1024x256x256")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_views.py measures on a GPU; none is visible")
    rate = read_rate()
    torch.cuda.empty_cache()
    shapes = [tuple(int(v) for v in s.split("x")) for s in a.shapes.split(",")]
    print(json.dumps({"views": [one_shape(T, H, W, a, rate) for T, H, W in shapes]}))


if __name__ == "__main__":
    main()
