"""Three-view projections without a GPU: the NumPy restatement (tests/views_ref.py) against the arrays the reference's own
utils/visualizer.py handed to imshow (tests/golden/views.npz, make_views_goldens.py), and the host side of the C ABI: the
symbols, the workspace query, and every argument check, which comes before any device call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import views_ref as R  # noqa: E402

from hiddenpose_amd import _lib  # noqa: E402

BAD_ARG, WORKSPACE = -1, -4
P0 = 0x1000        # a pointer a refused call never touches


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_restatement_reproduces_threeviews_log_bit_for_bit(golden):
    g = golden("views.npz")
    x = g["x"]
    assert x.shape == (2, 2, 12, 10, 14) and (x < 0).mean() > 0.3
    f, t, l, m = R.project(x[0, -1][None], R.MAX)
    assert (m > 0).all()                                 # the reference never divided by zero on this input
    of, ot, ol = R.orient(f, t, l, m)
    for got, key in ((of[0], "tv_front"), (ot[0], "tv_top"), (ol[0], "tv_left")):
        assert got.shape == g[key].shape and got.dtype == g[key].dtype == np.float32
        assert np.array_equal(bits(got), bits(g[key])), key
    # the orientation's index formulas of the header, spelled out
    T, H, W = x.shape[2:]
    n_top, n_left = t[0] / m[0, 1], l[0] / m[0, 2]
    i, j = np.meshgrid(np.arange(T), np.arange(W), indexing="ij")
    assert np.array_equal(g["tv_top"], n_top[T - 1 - i, W - 1 - j])
    i, j = np.meshgrid(np.arange(H), np.arange(T), indexing="ij")
    assert np.array_equal(g["tv_left"], n_left[T - 1 - j, i])


def test_restatement_reproduces_volume_log_exactly(golden):
    """volume_log sums with torch on the CPU (`volume[0, 0].sum(axis).numpy()`); the restatement makes the same calls, and the
    marks are the reference's NumPy lines, so the arrays are equal bit for bit."""
    g = golden("views.npz")
    f, t, l, _ = R.project(g["x"][0, 0][None], R.SUM)
    j = g["joints"]
    assert j.shape == (24, 3)
    for im, a, b, key in ((f[0], 1, 2, "vl_front"), (t[0], 0, 2, "vl_top"), (l[0], 0, 1, "vl_left")):
        got = R.mark(im.copy(), j, a, b)
        assert got.shape == g[key].shape and got.dtype == g[key].dtype
        assert np.array_equal(bits(got), bits(g[key])), key
        assert not np.array_equal(got, im)               # the marks are there


def test_restatement_rules():
    """The NaN rule, the clamp and the zero-maximum rule of the model itself."""
    x = np.full((2, 3, 4, 5), -1.0, np.float32)
    x[0, 1, 2, 3] = np.nan
    f, t, l, m = R.project(x, R.MAX)
    assert np.isnan(m[0]).all() and (m[1] == 0).all()
    assert np.isnan(f[0]).sum() == np.isnan(t[0]).sum() == np.isnan(l[0]).sum() == 1
    assert np.isnan(f[0, 2, 3]) and np.isnan(t[0, 1, 3]) and np.isnan(l[0, 1, 2])
    of, ot, ol = R.orient(f, t, l, m)
    assert (of[1] == 0).all() and (ot[1] == 0).all() and (ol[1] == 0).all()      # zero maximum: zeros, no NaN
    assert np.isnan(of[0]).all() and ol.shape == (2, 4, 3)                        # NaN maximum: a NaN view
    assert R.same(np.array([0.0, np.nan], np.float32), np.array([-0.0, np.nan], np.float32))
    assert not R.same(np.array([0.0, 1.0], np.float32), np.array([0.0, np.nan], np.float32))


def test_symbols_and_signatures(hip_lib):
    for name in ("hp_volume_views_workspace_bytes", "hp_volume_views", "hp_views_orient"):
        assert hasattr(hip_lib, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["hp_volume_views_workspace_bytes"][0] is C.c_size_t
    assert len(_lib.SIGNATURES["hp_volume_views"][1]) == 13 and len(_lib.SIGNATURES["hp_views_orient"][1]) == 12
    from hiddenpose_amd import visualizer as V

    assert V.MODES == {"max": R.MAX, "sum": R.SUM}


@pytest.mark.parametrize("mode", [R.MAX, R.SUM])
def test_workspace_query(hip_lib, mode):
    q = hip_lib.hp_volume_views_workspace_bytes
    for T, H, W in ((1, 1, 1), (3, 5, 7), (17, 33, 65), (130, 9, 70), (512, 128, 128), (1024, 256, 256)):
        prev = 0
        for P in (1, 2, 3, 7):
            n = q(P, T, H, W, mode)
            assert n > 0 and n % 4 == 0 and n > prev, (P, T, H, W, n)
            prev = n
    # one read of the plane plus slabs that are a fraction of it at the shapes people run
    assert q(1, 512, 128, 128, mode) < 0.25 * 4 * 512 * 128 * 128
    # what the call would refuse
    assert q(0, 4, 4, 4, mode) == 0 and q(1, 0, 4, 4, mode) == 0 and q(1, 4, -1, 4, mode) == 0 and q(1, 4, 4, 0, mode) == 0
    assert q(1, 2048, 1024, 1024, mode) == 0            # a plane of 2^31 voxels
    assert q(1, 2047, 1024, 1024, mode) > 0
    assert q(1, 4, 4, 4, 2) == 0 and q(1, 4, 4, 4, -1) == 0


def test_volume_views_refuses_bad_arguments_before_any_launch(hip_lib):
    call = hip_lib.hp_volume_views
    ok = dict(x=P0, front=P0, top=P0, left=P0, vmax=P0, P=2, T=4, H=5, W=6, mode=R.MAX, ws=P0, nbytes=None)

    def run(**kw):
        a = dict(ok, **kw)
        if a["nbytes"] is None:
            a["nbytes"] = max(hip_lib.hp_volume_views_workspace_bytes(a["P"], a["T"], a["H"], a["W"], a["mode"]), 4)
        return call(a["x"], a["front"], a["top"], a["left"], a["vmax"], a["P"], a["T"], a["H"], a["W"], a["mode"], a["ws"],
                    a["nbytes"], None)

    for name in ("x", "front", "top", "left", "vmax", "ws"):
        assert run(**{name: None}) == BAD_ARG, name
        assert b"null" in hip_lib.hp_last_error_string()
    for name in ("P", "T", "H", "W"):
        for v in (0, -3):
            assert run(**{name: v}) == BAD_ARG, (name, v)
            assert b"at least 1" in hip_lib.hp_last_error_string()
    for mode in (2, -1, 7):
        assert run(mode=mode) == BAD_ARG
        assert b"mode" in hip_lib.hp_last_error_string()
    assert run(T=2048, H=1024, W=1024) == BAD_ARG
    assert b"2^31" in hip_lib.hp_last_error_string()
    need = hip_lib.hp_volume_views_workspace_bytes(2, 4, 5, 6, R.SUM)
    assert run(mode=R.SUM, nbytes=need - 1) == WORKSPACE
    assert b"workspace too small" in hip_lib.hp_last_error_string()
    assert run(nbytes=0) == WORKSPACE


def test_views_orient_refuses_bad_arguments_before_any_launch(hip_lib):
    call = hip_lib.hp_views_orient
    ptrs = [P0] * 7
    for k in range(7):
        a = list(ptrs)
        a[k] = None
        assert call(*a, 1, 4, 5, 6, None) == BAD_ARG, k
        assert b"null" in hip_lib.hp_last_error_string()
    for dims in ((0, 4, 5, 6), (1, 0, 5, 6), (1, 4, -1, 6), (1, 4, 5, 0)):
        assert call(*ptrs, *dims, None) == BAD_ARG, dims
    assert call(*ptrs, 1, 2048, 1024, 1024, None) == BAD_ARG
    assert b"2^31" in hip_lib.hp_last_error_string()


def test_module_refuses_cpu_tensors():
    import torch

    from hiddenpose_amd import visualizer as V

    with pytest.raises(_lib.HiddenPoseHipError):
        V.project_views(torch.zeros(1, 1, 2, 3, 4))
    with pytest.raises(_lib.HiddenPoseHipError):
        V.three_views(torch.zeros(1, 1, 2, 3, 4))
