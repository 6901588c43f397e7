"""CPU-side checks of the transformer heads' losses (hp_joint_heatmaps, hp_joints_mse_*, hp_simdr_loss_*; criterion.JointsMSELoss /
JointTarget / NMTNORMCritierion): the float64 and float32 models of tests/head_loss_ref.py reproduce the goldens captured from
the reference, every refusal of the C entries returns a status and a message with no device present, `get_criterion`
selects by LOSS.TYPE, and the workspace queries are monotone multiples of 16 bytes."""
import numpy as np
import pytest
import torch

import head_loss_ref as R

FAKE = 0x1000      # a non-null address that is never dereferenced: every check below comes before any device call
WS = 1 << 16


def refused(L, rc, *words, status=-1):
    msg = L.hp_last_error_string()
    assert rc == status, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


# ---------------------------------------------------------------- the models against the reference's outputs
@pytest.mark.parametrize("u", [0, 1])
def test_heatmap_models_reproduce_the_reference(golden, u):
    g = golden("head_losses.npz")
    expect = np.array([[1, 1, 1, 1, 0], [1, 0, 1, 1, 0], [1, 1, 1, 1, 0]], np.float32)
    for dtype, tol in ((torch.float64, 2e-6), (torch.float32, 2e-6)):    # the reference itself computes in float32
        loss, grad, flags = R.joints_mse(g["hm_pred"], g["hm_joints"], float(g["hm_sigma"]), bool(u), dtype)
        assert np.array_equal(flags, expect) and np.array_equal(flags, g[f"hm_flags_{u}"])
        assert abs(loss / float(g[f"hm_loss_{u}"]) - 1) < tol, (dtype, loss)
        assert R.rel_l2(grad, g[f"hm_grad_{u}"]) < tol
    # truncation, not floor: (-3.2, 1.0) at sigma 2 has br.x = trunc(-0.2) = 0 and is in range; floor would put it out
    assert R.range_flags([[-3.2, 1.0]], 8, 12, 2.0)[0] == 1.0 and np.floor(np.float32(-3.2) + 2 + 1) < 0


def test_joint_target_model_reproduces_the_reference(golden):
    g = golden("head_losses.npz")
    W, H = (int(v) for v in g["jt_heatmap_size"])
    sigma = int(g["jt_sigma"]) * W // int(g["jt_image_size"][0])
    for dt, tol in ((np.float64, 2e-6), (np.float32, 2e-6)):
        t, w = R.heatmaps(g["jt_joints"], H, W, sigma, 3 * sigma, dt, vis=g["jt_vis"][:, 0])
        assert np.array_equal(w, g["jt_weight"][:, 0])
        assert R.rel_l2(t, g["jt_target"]) < tol
        assert all(not t[i].any() for i in range(len(w)) if w[i] <= 0.5) and t[0].any() and t[1].any()


def test_simdr_models_reproduce_the_reference(golden):
    g = golden("head_losses.npz")
    for dtype in (torch.float64, torch.float32):
        loss, grads = R.simdr([g["sd_x"], g["sd_y"], g["sd_z"]], g["sd_target"], g["sd_weight"], float(g["sd_ls"]), dtype)
        assert abs(loss / float(g["sd_loss"]) - 1) < 2e-6, (dtype, loss)
        for got, key in zip(grads, ("sd_gx", "sd_gy", "sd_gz")):
            assert R.rel_l2(got, g[key]) < 2e-6, key


def test_simdr_model_limits():
    """ls = 0 is the formula's limit -s_label / n; a label outside [0, n) leaves every bin at ls / (n - 1)."""
    g = torch.Generator().manual_seed(3)
    x = [torch.randn(2, 3, n, generator=g).numpy() for n in (5, 6, 7)]
    tgt = torch.tensor([[[1.2, 0.0, 6.9]] * 3] * 2)
    loss, _ = R.simdr(x, tgt, None, 0.0)
    want = sum(float(-(torch.log_softmax(torch.tensor(x[a]).double(), -1)[:, :, int(tgt[0, 0, a])]).sum()) / x[a].shape[-1]
               for a in range(3)) / 6
    assert abs(loss - want) < 1e-12
    out, _ = R.simdr(x, torch.full((2, 3, 3), 99.0), None, 0.2)
    want = 0.0
    for a in range(3):
        n = x[a].shape[-1]
        s = torch.log_softmax(torch.tensor(x[a]).double(), -1)
        u = 0.2 / (n - 1)
        want += float((u * (np.log(u) - s)).sum()) / n / 6
    assert abs(out - want) < 1e-12 and np.isfinite(out)


# ---------------------------------------------------------------- refusals: status -1 and a message, before any launch
def test_heatmap_argument_checks_come_before_any_device_call(hip_lib):
    L = hip_lib

    def fwd(pred=FAKE, joints=FAKE, B=2, J=3, H=8, W=12, sigma=2.0, utw=0, flags=FAKE, loss=FAKE, ws=FAKE, ws_bytes=WS):
        return L.hp_joints_mse_forward(pred, joints, B, J, H, W, sigma, utw, flags, loss, ws, ws_bytes, None)

    def bwd(pred=FAKE, joints=FAKE, flags=FAKE, gloss=FAKE, B=2, J=3, H=8, W=12, sigma=2.0, utw=0, d=FAKE):
        return L.hp_joints_mse_backward(pred, joints, flags, gloss, B, J, H, W, sigma, utw, d, None)

    def render(joints=FAKE, vis=None, R_=6, H=8, W=12, sigma=2.0, tmp=6.0, target=FAKE, flags=FAKE):
        return L.hp_joint_heatmaps(joints, vis, R_, H, W, sigma, tmp, target, flags, None)

    for name in ("pred", "joints", "flags", "loss"):
        refused(L, fwd(**{name: None}), "null pointer")
    for name in ("pred", "joints", "flags", "gloss", "d"):
        refused(L, bwd(**{name: None}), "null pointer")
    for name in ("joints", "target", "flags"):
        refused(L, render(**{name: None}), "null pointer")
    for call in (fwd, bwd):
        for name in ("B", "J", "H", "W"):
            refused(L, call(**{name: 0}), "at least 1")
            refused(L, call(**{name: -2}), "at least 1")
        for s in (0.0, -1.0, float("nan"), float("inf")):
            refused(L, call(sigma=s), "sigma")
        refused(L, call(B=65536, J=65536), "maps exceed")
        refused(L, call(H=65536, W=65536), "32-bit index")
        refused(L, call(utw=2), "use_target_weight")
    for name in ("R_", "H", "W"):
        refused(L, render(**{name: 0}), "at least 1")
    refused(L, render(sigma=0.0), "sigma")
    refused(L, render(tmp=float("nan")), "tmp_size")
    refused(L, render(H=65536, W=65536), "32-bit index")
    refused(L, fwd(ws=None), "null workspace")
    refused(L, fwd(ws_bytes=L.hp_joints_mse_workspace_bytes(2, 3) - 1), "workspace too small")
    refused(L, fwd(H=9000, W=9000), "not built", status=-2)      # the tables of a map live in LDS


def test_simdr_argument_checks_come_before_any_device_call(hip_lib):
    L = hip_lib

    def args(px=FAKE, nx=16, sx=16, py=FAKE, ny=24, sy=24, pz=FAKE, nz=7, sz=7, target=FAKE, weight=None, B=2, J=3, ls=0.2):
        return [px, nx, sx, py, ny, sy, pz, nz, sz, target, weight, B, J, ls]

    def fwd(stat=FAKE, loss=FAKE, ws=FAKE, ws_bytes=WS, **kw):
        return L.hp_simdr_loss_forward(*args(**kw), stat, loss, ws, ws_bytes, None)

    def bwd(stat=FAKE, gloss=FAKE, dx=FAKE, dy=FAKE, dz=FAKE, **kw):
        return L.hp_simdr_loss_backward(*args(**kw), stat, gloss, dx, dy, dz, None)

    for call in (fwd, bwd):
        for name in ("px", "py", "pz", "target", "stat"):
            refused(L, call(**{name: None}), "null pointer")
        for name in ("B", "J"):
            refused(L, call(**{name: 0}), "at least 1")
        for name in ("nx", "ny", "nz"):
            refused(L, call(**{name: 1}), "at least 2 bins")
        refused(L, call(sx=15), "stride")
        for ls in (-0.1, 1.0, float("nan"), float("inf")):
            refused(L, call(ls=ls), "label_smoothing")
        refused(L, call(B=65536, J=65536), "rows exceed")
    refused(L, fwd(loss=None), "null pointer")
    for name in ("gloss", "dx", "dy", "dz"):
        refused(L, bwd(**{name: None}), "null pointer")
    refused(L, fwd(ws=None), "null workspace")
    refused(L, fwd(ws_bytes=L.hp_simdr_loss_workspace_bytes(2, 3) - 1), "workspace too small")


def test_workspace_queries(hip_lib):
    for q, per in ((hip_lib.hp_joints_mse_workspace_bytes, 8), (hip_lib.hp_simdr_loss_workspace_bytes, 24)):
        assert q(0, 3) == 0 and q(3, 0) == 0 and q(-1, 3) == 0
        last = 0
        for B, J in ((1, 1), (1, 3), (2, 3), (3, 5), (8, 16), (8, 17), (64, 24), (1000, 33)):
            v = q(B, J)
            assert v % 16 == 0 and v >= B * J * per and v >= last, (B, J, v)
            last = v


# ---------------------------------------------------------------- Python layer
def test_get_criterion_selects_by_loss_type():
    from hiddenpose_amd import criterion as Cr
    from hiddenpose_amd.config import get_cfg_defaults

    cfg = get_cfg_defaults()
    assert cfg.DATASET.TARGET_TYPE == "gaussian" and cfg.DATASET.SIGMA == 2 and cfg.DATASET.USE_DIFFERENT_JOINTS_WEIGHT is True
    assert cfg.LOSS.LABEL_SMOOTHING == 0.2 and cfg.LOSS.USE_TARGET_WEIGHT is False
    assert type(Cr.get_criterion(cfg)) is Cr.L2JointLocationLoss
    cfg.LOSS.TYPE = "JointsMSELoss"
    c = Cr.get_criterion(cfg)
    assert type(c) is Cr.JointsMSELoss and c.sigma == 2 and c.use_target_weight is False
    cfg.LOSS.USE_TARGET_WEIGHT = True
    assert Cr.get_criterion(cfg).use_target_weight is True
    cfg.LOSS.TYPE = "NMTNORMCritierion"
    c = Cr.get_criterion(cfg)
    assert type(c) is Cr.NMTNORMCritierion and c.label_smoothing == 0.2
    cfg.LOSS.TYPE = "nope"
    with pytest.raises(ValueError, match="LOSS.TYPE"):
        Cr.get_criterion(cfg)


def test_python_refusals():
    from hiddenpose_amd import _lib
    from hiddenpose_amd import criterion as Cr
    from hiddenpose_amd.config import get_cfg_defaults

    cfg = get_cfg_defaults()
    cfg.DATASET.HEATMAP_SIZE = [12, 8]
    cfg.DATASET.TARGET_TYPE = "offset"
    with pytest.raises(AssertionError, match="gaussian"):
        Cr.JointsMSELoss(cfg, False)(torch.zeros(1, 2, 8, 12), torch.zeros(1, 2, 2), None)
    cfg.DATASET.IMAGE_SIZE = [12, 8]
    with pytest.raises(AssertionError, match="gaussian"):
        Cr.JointTarget(cfg).generate_target(torch.zeros(2, 2), torch.ones(2, 2))
    cfg.DATASET.TARGET_TYPE = "gaussian"
    with pytest.raises(AssertionError, match="HEATMAP_SIZE"):
        Cr.JointsMSELoss(cfg, False)(torch.zeros(1, 2, 12, 8), torch.zeros(1, 2, 2), None)
    with pytest.raises(_lib.HiddenPoseHipError, match="no CPU path"):     # no quiet fall-back to ATen
        Cr.JointsMSELoss(cfg, False)(torch.zeros(1, 2, 8, 12), torch.zeros(1, 2, 2), None)
    with pytest.raises(_lib.HiddenPoseHipError, match="no CPU path"):
        Cr.NMTNORMCritierion(0.2)(torch.zeros(1, 2, 4), torch.zeros(1, 2, 4), torch.zeros(1, 2, 4), torch.zeros(1, 2, 3), None)
    for ls in (-0.1, 1.0):
        with pytest.raises(ValueError, match="label_smoothing"):
            Cr.NMTNORMCritierion(ls)
