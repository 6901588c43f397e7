"""Three-view projections on the GPU: hp_volume_views / hp_views_orient through the C ABI and hiddenpose_amd.visualizer
against the reference's recorded arrays (tests/golden/views.npz) and the NumPy model (tests/views_ref.py).

Max mode and the oriented images are compared bit for bit (`views_ref.same`: equal values, NaNs in the same places).  Sum mode
is compared with a float64 sum per pixel under |got - s64| <= (n + 1) 2^-24 sum|x| over the n reduced terms, the bound of
fp32 accumulation in any order.  The tile of k_views_tile is (16 frames, 16 rows, 64 columns), a wave takes 4 rows, the
combine kernels work on 256 pixels: the shapes cross each of those edges."""
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import views_ref as R  # noqa: E402

from hiddenpose_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(1, 1, 1), (1, 7, 1), (3, 5, 7), (17, 33, 65), (64, 64, 64), (130, 9, 70)]
POISON_NAN, POISON_BIG = 0x7FC00001, 0x7F7FFFF0      # a NaN payload and a float near FLT_MAX


def filled(shape, pattern, dev="cuda"):
    n = int(np.prod(shape))
    t = torch.full((n,), pattern if pattern < 2 ** 31 else pattern - 2 ** 32, dtype=torch.int32, device=dev) if pattern is not None \
        else torch.empty(n, dtype=torch.int32, device=dev)
    return t.view(torch.float32).reshape(shape)


def abi_views(x, mode, pattern=None, ws_extra=0):
    """x: (P, T, H, W) float32 CUDA tensor -> dict of NumPy results of hp_volume_views + hp_views_orient, with outputs and
    workspace pre-filled with `pattern` and a workspace of exactly the queried size (+ ws_extra bytes)."""
    L = _lib.lib()
    P, T, H, W = x.shape
    need = L.hp_volume_views_workspace_bytes(P, T, H, W, mode)
    assert need > 0 and need % 4 == 0
    ws = filled((need // 4,), pattern)
    front, top, left = filled((P, H, W), pattern), filled((P, T, W), pattern), filled((P, T, H), pattern)
    vmax = filled((P, 3), pattern)
    st = _lib.current_stream_handle(x.device)
    rc = L.hp_volume_views(x.data_ptr(), front.data_ptr(), top.data_ptr(), left.data_ptr(), vmax.data_ptr(), P, T, H, W, mode,
                           ws.data_ptr(), need + ws_extra, st)
    assert rc == 0, L.hp_last_error_string()
    of, ot, ol = filled((P, H, W), pattern), filled((P, T, W), pattern), filled((P, H, T), pattern)
    rc = L.hp_views_orient(front.data_ptr(), top.data_ptr(), left.data_ptr(), vmax.data_ptr(), of.data_ptr(), ot.data_ptr(),
                           ol.data_ptr(), P, T, H, W, st)
    assert rc == 0, L.hp_last_error_string()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(front=front, top=top, left=left, vmax=vmax, of=of, ot=ot, ol=ol).items()}


def ref_views(x_np, mode=R.MAX):
    f, t, l, m = R.project(x_np, mode)
    of, ot, ol = R.orient(f, t, l, m)
    return dict(front=f, top=t, left=l, vmax=m, of=of, ot=ot, ol=ol)


def assert_same(got, want, what=""):
    for k in want:
        assert R.same(got[k], want[k]), (what, k)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def volume(P, T, H, W, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    return (g.standard_normal((P, T, H, W)) * 1.5 - 0.3).astype(np.float32)


# ---------------------------------------------------------------- the golden
def test_golden_three_views_bit_equal(golden):
    from hiddenpose_amd import visualizer as V

    g = golden("views.npz")
    x = torch.from_numpy(g["x"]).cuda()
    keep = x.clone()
    of, ot, ol = V.three_views(x)
    for got, key in ((of, "tv_front"), (ot, "tv_top"), (ol, "tv_left")):
        assert got.shape == g[key].shape
        assert np.array_equal(bits(got.cpu().numpy()), bits(g[key])), key
    assert torch.equal(x.view(torch.int32), keep.view(torch.int32))          # the call never modifies x
    got = abi_views(x[0, -1][None].contiguous(), R.MAX)
    for k, key in (("of", "tv_front"), ("ot", "tv_top"), ("ol", "tv_left")):
        assert np.array_equal(bits(got[k][0]), bits(g[key])), key
    # volume_log's plane: the device sums against float64 and, through it, against what the reference summed (its marks
    # are host work on the finished views: test_loggers_write_the_reference_file_stems)
    f, t, l, _ = V.project_views(x, [(0, 0)], "sum")
    for view, (s64, a64, n) in zip((f, t, l), R.sums64(g["x"][0, 0][None])):
        assert (np.abs(view[0].cpu().numpy() - s64[0]) <= R.sum_bound(a64[0], n)).all()


# ---------------------------------------------------------------- small shapes
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("T,H,W", SHAPES)
def test_shapes_against_the_model(T, H, W, P):
    x_np = volume(P, T, H, W, seed=T * 1000 + H * 10 + W + P)
    x = torch.from_numpy(x_np).cuda()
    assert_same(abi_views(x, R.MAX), ref_views(x_np), (T, H, W, P))
    got = abi_views(x, R.SUM)
    for k, (s64, a64, n) in zip(("front", "top", "left"), R.sums64(x_np)):
        assert got[k].shape == s64.shape
        err, bound = np.abs(got[k].astype(np.float64) - s64), R.sum_bound(a64, n)
        assert (err <= bound).all(), (k, float((err - bound).max()))
    # vmax and the oriented images follow from the finished views exactly, whatever the summation order
    f, t, l = got["front"], got["top"], got["left"]
    m = np.stack([v.reshape(P, -1).max(axis=1) for v in (f, t, l)], axis=1)
    assert R.same(got["vmax"], m)
    of, ot, ol = R.orient(f, t, l, m)
    assert R.same(got["of"], of) and R.same(got["ot"], ot) and R.same(got["ol"], ol)


# ---------------------------------------------------------------- edges of every axis
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_first_and_last_index_of_an_axis(axis):
    T, H, W = 33, 17, 65                                  # several tiles along every axis, the last one a single index wide
    x_np = np.full((1, T, H, W), -2.0, np.float32)
    first, last = [5, 3, 7], [20, 11, 40]
    first[axis], last[axis] = 0, (T, H, W)[axis] - 1
    x_np[0][tuple(first)], x_np[0][tuple(last)] = 3.0, 5.0
    got = abi_views(torch.from_numpy(x_np).cuda(), R.MAX)
    assert_same(got, ref_views(x_np), axis)
    for k, drop in (("front", 0), ("top", 1), ("left", 2)):
        want = np.zeros(got[k].shape[1:], np.float32)
        want[tuple(v for i, v in enumerate(first) if i != drop)] = 3.0
        want[tuple(v for i, v in enumerate(last) if i != drop)] = 5.0
        assert np.array_equal(got[k][0], want), (axis, k)
    assert np.array_equal(got["vmax"], np.full((1, 3), 5.0, np.float32))


# ---------------------------------------------------------------- clamp
def test_all_negative_plane_gives_zero_views_and_no_nan():
    x_np = -np.abs(volume(2, 17, 33, 65, seed=5)) - 0.5
    x_np[1] = volume(1, 17, 33, 65, seed=6)[0]
    got = abi_views(torch.from_numpy(x_np).cuda(), R.MAX, POISON_NAN)
    for k in ("front", "top", "left", "of", "ot", "ol"):
        assert np.array_equal(bits(got[k][0]), np.zeros_like(bits(got[k][0]))), k     # +0.0, not -0.0, not NaN
    assert np.array_equal(bits(got["vmax"][0]), np.zeros(3, np.uint32))
    assert_same(got, ref_views(x_np))
    neg_zero = np.full((1, 3, 5, 7), -0.0, np.float32)
    got = abi_views(torch.from_numpy(neg_zero).cuda(), R.MAX)
    assert not np.isnan(got["of"]).any() and (got["vmax"] == 0).all() and (got["of"] == 0).all()


# ---------------------------------------------------------------- NaN and inf
@pytest.mark.parametrize("pattern", [0x7FC00000, 0xFFC00001, 0x7F800000], ids=["nan", "negative-nan", "inf"])
@pytest.mark.parametrize("mode", [R.MAX, R.SUM], ids=["max", "sum"])
def test_a_single_non_finite_value(pattern, mode):
    P, T, H, W = 3, 40, 20, 70
    base = volume(P, T, H, W, seed=11)
    x_np = base.copy()
    t, h, w = 33, 17, 66                                  # in the last tile of every axis
    x_np.view(np.uint32)[1, t, h, w] = pattern
    got = abi_views(torch.from_numpy(x_np).cuda(), mode)
    clean = abi_views(torch.from_numpy(base).cuda(), mode)
    for k in got:                                         # the other planes are untouched
        assert np.array_equal(bits(got[k][[0, 2]]), bits(clean[k][[0, 2]])), k
    hit = {"front": (h, w), "top": (t, w), "left": (t, h)}
    if pattern == 0x7F800000:
        for k, at in hit.items():
            assert np.isinf(got[k][1]).sum() == 1 and got[k][1][at] == np.inf, k
        assert (got["vmax"][1] == np.inf).all()           # +inf propagates as a value, here as the maximum
        if mode == R.MAX:
            assert_same(got, ref_views(x_np))
        return
    for k, at in hit.items():
        nan = np.isnan(got[k][1])
        assert nan.sum() == 1 and nan[at], k              # exactly the three pixels of its lines
        rest = ~nan
        assert np.array_equal(bits(got[k][1][rest]), bits(clean[k][1][rest])), k
    assert np.isnan(got["vmax"][1]).all()
    assert np.isnan(got["of"][1]).all() and np.isnan(got["ot"][1]).all() and np.isnan(got["ol"][1]).all()
    if mode == R.MAX:
        assert_same(got, ref_views(x_np))
        assert (bits(got["vmax"][1]) == 0x7FC00000).all() and bits(got["front"][1])[h, w] == 0x7FC00000


# ---------------------------------------------------------------- poison, exact workspace, determinism
@pytest.mark.parametrize("mode", [R.MAX, R.SUM], ids=["max", "sum"])
def test_poisoned_outputs_and_exact_workspace(mode):
    L = _lib.lib()
    P, T, H, W = 2, 70, 35, 130
    x_np = volume(P, T, H, W, seed=21)
    x = torch.from_numpy(x_np).cuda()
    runs = [abi_views(x, mode, pat) for pat in (None, POISON_NAN, POISON_BIG, POISON_NAN)]
    for r in runs[1:]:                                    # poison changes nothing; two calls give equal bits
        for k in r:
            assert np.array_equal(bits(r[k]), bits(runs[0][k])), k
    assert np.array_equal(bits(x.cpu().numpy()), bits(x_np))                  # x is bit-identical after the calls
    if mode == R.MAX:
        assert_same(runs[0], ref_views(x_np))
    # one byte less than the query: refused before any launch, nothing written
    need = L.hp_volume_views_workspace_bytes(P, T, H, W, mode)
    ws = filled((need // 4,), POISON_NAN)
    outs = [filled(s, POISON_NAN) for s in ((P, H, W), (P, T, W), (P, T, H), (P, 3))]
    rc = L.hp_volume_views(x.data_ptr(), *[o.data_ptr() for o in outs], P, T, H, W, mode, ws.data_ptr(), need - 1,
                           _lib.current_stream_handle(x.device))
    assert rc == -4 and b"workspace too small" in L.hp_last_error_string()
    torch.cuda.synchronize()
    for o in outs + [ws]:
        assert (o.view(torch.int32) == POISON_NAN).all()


# ---------------------------------------------------------------- the module: plane selection and layout
def test_plane_selection_and_layout():
    from hiddenpose_amd import visualizer as V

    B, C, T, H, W = 2, 3, 17, 9, 70
    x_np = volume(B * C, T, H, W, seed=31).reshape(B, C, T, H, W)
    x = torch.from_numpy(x_np).cuda()
    want = ref_views(x_np[0, -1][None])
    of, ot, ol = V.three_views(x)
    assert R.same(of.cpu().numpy(), want["of"][0]) and R.same(ot.cpu().numpy(), want["ot"][0])
    assert R.same(ol.cpu().numpy(), want["ol"][0]) and ol.shape == (H, T)
    other = V.three_views(x, plane=(1, 0))
    assert R.same(other[0].cpu().numpy(), ref_views(x_np[1, 0][None])["of"][0])
    # every plane in (b, c) order
    f, t, l, m = V.project_views(x)
    allp = ref_views(x_np.reshape(B * C, T, H, W))
    assert R.same(f.cpu().numpy(), allp["front"]) and R.same(t.cpu().numpy(), allp["top"])
    assert R.same(l.cpu().numpy(), allp["left"]) and R.same(m.cpu().numpy(), allp["vmax"])
    # a permuted (non-contiguous) view gives what its contiguous copy gives; so does a float64 tensor of the same values
    y = torch.from_numpy(np.ascontiguousarray(x_np.transpose(0, 1, 4, 3, 2))).cuda().permute(0, 1, 4, 3, 2)
    assert not y.is_contiguous() and torch.equal(y, x)
    for z in (y, x.double()):
        for a, b in zip(V.three_views(z), (of, ot, ol)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        for a, b in zip(V.project_views(z, mode="sum"), V.project_views(x, mode="sum")):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(_lib.HiddenPoseHipError):
        V.project_views(x.cpu())


# ---------------------------------------------------------------- the loggers
def test_loggers_write_the_reference_file_stems(tmp_path):
    from hiddenpose_amd import visualizer as V

    x_np = volume(4, 12, 10, 14, seed=41).reshape(2, 2, 12, 10, 14)
    x = torch.from_numpy(x_np).cuda()
    d = str(tmp_path / "tv")
    imgs = V.threeviews_log(x, d, "feature_7", 7)
    want = ref_views(x_np[0, -1][None])
    assert R.same(imgs["front"], want["of"][0]) and R.same(imgs["top"], want["ot"][0]) and R.same(imgs["left"], want["ol"][0])
    for view in ("front", "top", "left"):
        assert os.path.getsize(os.path.join(d, f"feature_7_{view}_view_7.jpg")) > 0
    joints = np.array([[3.2, 4.9, 6.1], [10.0, 8.0, 12.0], [0.0, 0.0, 0.0]])
    v = str(tmp_path / "vol")
    got = V.volume_log(x, v, "volume_7", 7, joints=joints)
    plain = V.volume_log(x, v, "plain_7", 7)
    assert os.path.getsize(os.path.join(v, "projection_of_vol", "volume_7_7_front_joints.jpg")) > 0
    for view in ("top", "left"):
        assert os.path.getsize(os.path.join(v, "figure", "projection_of_vol", f"volume_7_7_{view}_joints.jpg")) > 0
    for (k, (a, b)), (s64, a64, n) in zip((("front", (1, 2)), ("top", (0, 2)), ("left", (0, 1))), R.sums64(x_np[0, 0][None])):
        assert (np.abs(plain[k] - s64[0]) <= R.sum_bound(a64[0], n)).all(), k
        assert np.array_equal(got[k], R.mark(plain[k].copy(), joints, a, b)) and not np.array_equal(got[k], plain[k]), k
    j = np.arange(72, dtype=np.float64).reshape(24, 3) % 60
    jd = str(tmp_path / "joints")
    back = V.joints_log(torch.from_numpy(j).cuda(), jd, "pred_joints_7", 7)
    assert np.array_equal(back, j)
    assert np.array_equal(np.loadtxt(os.path.join(jd, "txt", "pred_joints_77.txt")), j)
    assert os.path.getsize(os.path.join(jd, "pred_joints_77.png")) > 0


def test_train_epoch_writes_the_eight_items_only_when_asked(tmp_path):
    from hiddenpose_amd import testing as hpt
    from hiddenpose_amd.config import make_cfg
    from hiddenpose_amd.NlosPose import NlosPose
    from hiddenpose_amd.nlos_pose_dataloader import NlosPoseDataset
    from hiddenpose_amd.train_epoch import build_training, train_epoch
    from train import _collate

    spec = importlib.util.spec_from_file_location("make_synthetic_dataset", os.path.join(ROOT, "tools", "make_synthetic_dataset.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    data = tmp_path / "ds"
    argv = sys.argv
    try:
        sys.argv = ["make_synthetic_dataset.py", str(data), "2", "64"]
        tool.main()
    finally:
        sys.argv = argv
    cfg = make_cfg(128, 32)            # 600 x 64 x 64 pixels -> (128, 32, 32) after the ingest pyramid
    cfg.TRAIN.END_EPOCH = 1
    ds = NlosPoseDataset(cfg, str(data))
    loader = torch.utils.data.DataLoader(ds, batch_size=2, shuffle=False, collate_fn=_collate)
    model = NlosPose(cfg)
    hpt.fill_module(model)
    model = model.cuda()
    criterion, voxel_criterion, optimizer, sched = build_training(cfg, model)
    sched.step()

    def epoch(views_every, views_dir):
        return train_epoch(cfg, loader, model, criterion, voxel_criterion, optimizer, 0, str(tmp_path), None, 0.0,
                           str(tmp_path / "ck"), sched, max_steps=1, views_every=views_every, views_dir=str(views_dir))

    off = tmp_path / "off"
    assert np.isfinite(epoch(None, off)) and not off.exists()
    on = tmp_path / "on"
    assert np.isfinite(epoch(1, on))
    it = 1
    want = [f"volume/projection_of_vol/{n}_{it}_{it}_front_joints.jpg" for n in ("volume", "output", "feature")]
    want += [f"volume/figure/projection_of_vol/{n}_{it}_{it}_{v}_joints.jpg" for n in ("volume", "output", "feature") for v in ("top", "left")]
    want += [f"figure/joints/{n}_joints_{it}{it}.png" for n in ("pred", "gt")]
    want += [f"figure/joints/txt/{n}_joints_{it}{it}.txt" for n in ("pred", "gt")]
    want += [f"figure/threeviews/{n}_{it}_{v}_view_{it}.jpg" for n in ("feature", "output", "volume") for v in ("front", "top", "left")]
    for rel in want:
        assert os.path.getsize(os.path.join(str(on), rel)) > 0, rel
    assert np.loadtxt(os.path.join(str(on), f"figure/joints/txt/gt_joints_{it}{it}.txt")).shape == (24, 3)
