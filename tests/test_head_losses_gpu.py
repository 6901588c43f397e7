"""GPU tests of the transformer heads' losses (headloss_kernels.hip behind hip_ops.joints_mse / joint_heatmaps / simdr_loss,
criterion.JointsMSELoss / JointTarget / NMTNORMCritierion, train_heads): parity with the float64 model of head_loss_ref inside a
bar set by the float32 CPU model's own error, packed views, guard regions and alignment, reproducibility, autograd scaling, and
heads trained end to end.

Bar of every parity check: relative L2 <= max(4 x e_ref, 8 x 2^-24), e_ref = the float32 CPU model's error against float64 on
the same inputs.  The HIP / float32-model ratio is printed per case (DESIGN 4.5.1 records the measured ones)."""
import numpy as np
import pytest
import torch

import head_loss_ref as R
from hiddenpose_amd import _lib
from hiddenpose_amd import criterion as Cr
from hiddenpose_amd import hip_ops as ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -12345.0


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def check(what, got, want64, ref32):
    """got (HIP) and ref32 (float32 CPU model) against want64; scalars or tensors."""
    if np.ndim(want64) == 0 and not torch.is_tensor(want64):
        e = abs(float(got) - want64) / max(abs(want64), 1e-300)
        e_ref = abs(float(ref32) - want64) / max(abs(want64), 1e-300)
    else:
        e, e_ref = R.rel_l2(got, want64), R.rel_l2(ref32, want64)
    print(f"head-loss parity {what}: hip {e:.3e} fp32-model {e_ref:.3e} ratio {e / max(e_ref, 1e-300):.2f} bar {R.bar(e_ref):.3e}")
    assert e <= R.bar(e_ref), (what, e, e_ref)


# ---------------------------------------------------------------- 1. parity: heat-map
def hm_inputs(B, J, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(B, J, H, W, generator=g) * 1.2 - 0.1
    joints = torch.stack((torch.rand(B, J, generator=g) * (W + 8) - 4, torch.rand(B, J, generator=g) * (H + 8) - 4), dim=-1)
    return pred, joints


HM_CASES = [("golden", 0, 0, 0, 0, 2.0), ("7x5", 2, 3, 7, 5, 2.0), ("1x1", 2, 3, 1, 1, 2.0), ("tokenpose-64x48", 2, 16, 64, 48, 2.0),
            ("B1", 1, 4, 8, 12, 2.0), ("J1", 3, 1, 8, 12, 2.0), ("sigma0.5", 2, 3, 16, 20, 0.5), ("sigma7.5", 2, 3, 16, 20, 7.5)]


@pytest.mark.parametrize("utw", [False, True])
@pytest.mark.parametrize("name,B,J,H,W,sigma", HM_CASES, ids=[c[0] for c in HM_CASES])
def test_heatmap_parity_with_the_float64_model(golden, name, B, J, H, W, sigma, utw):
    if name == "golden":
        g = golden("head_losses.npz")
        pred, joints = torch.from_numpy(g["hm_pred"]), torch.from_numpy(g["hm_joints"])
        B, J, H, W = pred.shape
    else:
        pred, joints = hm_inputs(B, J, H, W, seed=11 + H * W)
    l64, g64, f64 = R.joints_mse(pred, joints, sigma, utw, torch.float64)
    l32, g32, _ = R.joints_mse(pred, joints, sigma, utw, torch.float32)
    p = pred.to(DEV).requires_grad_(True)
    loss, flags = ops.joints_mse(p, joints.to(DEV), sigma, utw)
    loss.backward()
    assert np.array_equal(flags.cpu().numpy(), f64), "flags must be exact"
    tag = f"heat-map {name} utw={int(utw)}"
    check(tag + " loss", loss.item(), l64, l32)
    check(tag + " grad", p.grad, g64, g32)
    if name == "golden":
        u = int(utw)
        assert np.array_equal(flags.cpu().numpy(), g[f"hm_flags_{u}"])
        assert abs(loss.item() / float(g[f"hm_loss_{u}"]) - 1) < 2e-6 and R.rel_l2(p.grad, g[f"hm_grad_{u}"]) < 2e-6
    if not utw:     # the rendered maps: JointsMSELoss's range (t = sigma) and JointTarget's (t = 3 sigma, with visibilities)
        vis = (torch.arange(B * J) % 4).float() / 3.0
        for t, v in ((sigma, None), (3 * sigma, vis)):
            m64, w64 = R.heatmaps(joints.reshape(-1, 2), H, W, sigma, t, np.float64, None if v is None else v.numpy())
            m32, _ = R.heatmaps(joints.reshape(-1, 2), H, W, sigma, t, np.float32, None if v is None else v.numpy())
            maps, w = ops.joint_heatmaps(joints.to(DEV), H, W, sigma, t, v)
            assert np.array_equal(w.cpu().numpy(), w64)
            zero = w64 <= 0.5
            assert not maps[torch.from_numpy(zero).to(DEV)].any()
            if (~zero).any():
                check(tag + f" maps t={t}", maps, m64, m32)


def test_joint_target_matches_the_reference_golden(golden):
    from hiddenpose_amd.config import get_cfg_defaults

    g = golden("head_losses.npz")
    cfg = get_cfg_defaults()
    cfg.DATASET.NUM_JOINTS = 5
    cfg.DATASET.HEATMAP_SIZE = [int(v) for v in g["jt_heatmap_size"]]
    cfg.DATASET.IMAGE_SIZE = [int(v) for v in g["jt_image_size"]]
    cfg.DATASET.SIGMA = int(g["jt_sigma"])
    for joints, vis in ((torch.from_numpy(g["jt_joints"]), g["jt_vis"]), (torch.from_numpy(g["jt_joints"]).to(DEV), torch.from_numpy(g["jt_vis"]).to(DEV))):
        target, weight = Cr.JointTarget(cfg).generate_target(joints, vis)
        assert target.shape == g["jt_target"].shape and weight.shape == (5, 1)
        assert np.array_equal(weight.cpu().numpy(), g["jt_weight"])
        assert R.rel_l2(target, g["jt_target"]) < 2e-6


# ---------------------------------------------------------------- 1. parity: SimDR
def sd_inputs(bins, B=2, J=3, seed=5, scale=2.0):
    g = torch.Generator().manual_seed(seed + sum(bins))
    xs = [torch.randn(B, J, n, generator=g) * scale for n in bins]
    target = torch.stack([torch.randint(0, n, (B, J), generator=g).float() + 0.6 for n in bins], dim=-1)
    weight = torch.rand(B, J, 1, generator=g)
    return xs, target, weight


def sd_run(xs, target, weight, ls):
    leaves = [x.to(DEV).requires_grad_(True) for x in xs]
    loss = ops.simdr_loss(*leaves, target.to(DEV), None if weight is None else weight.to(DEV), ls)
    loss.backward()
    return loss, [p.grad for p in leaves]


def sd_check(tag, xs, target, weight, ls):
    l64, g64 = R.simdr(xs, target, weight, ls, torch.float64)
    l32, g32 = R.simdr(xs, target, weight, ls, torch.float32)
    loss, grads = sd_run(xs, target, weight, ls)
    assert torch.isfinite(loss).item()
    check(tag + " loss", loss.item(), l64, l32)
    for a in range(3):
        check(tag + f" grad{a}", grads[a], g64[a], g32[a])
    return loss, grads


@pytest.mark.parametrize("n", [2, 7, 63, 64, 65, 257, 512, 513, 1000])
def test_simdr_parity_per_bin_count(n):
    """2: the minimum; 63 / 64 / 65: the wave's edges; 512 / 513: rows in registers against the online loop; 1000: a ragged loop."""
    xs, target, weight = sd_inputs((n, n, n))
    sd_check(f"simdr n={n}", xs, target, weight, 0.2)


def test_simdr_parity_golden(golden):
    g = golden("head_losses.npz")
    xs = [torch.from_numpy(g[k]) for k in ("sd_x", "sd_y", "sd_z")]
    loss, grads = sd_check("simdr golden", xs, torch.from_numpy(g["sd_target"]), torch.from_numpy(g["sd_weight"]), float(g["sd_ls"]))
    assert abs(loss.item() / float(g["sd_loss"]) - 1) < 2e-6
    for got, key in zip(grads, ("sd_gx", "sd_gy", "sd_gz")):
        assert R.rel_l2(got, g[key]) < 2e-6


@pytest.mark.parametrize("ls", [0.0, 0.2, 0.9])
def test_simdr_parity_edge_cases(ls):
    """Three different counts (one of them on the loop path) in one call; labels 0 and n - 1; a target of 5.99 (label 5); logits of
    +-80 in one row; a row with weight 0; labels outside the range on every side (no confidence bin, finite loss); weight=None."""
    bins = (16, 600, 7)
    xs, target, weight = sd_inputs(bins, B=2, J=4, seed=9)
    target[0, 0] = torch.tensor([0.0, 0.3, 0.9])            # label 0 on every axis
    target[0, 1] = torch.tensor([15.2, 599.9, 6.0])         # label n - 1
    target[0, 2] = torch.tensor([5.99, 5.99, 5.99])
    target[0, 3] = torch.tensor([16.0, -1.0, 1.0e12])       # outside: n, negative, far beyond int32
    target[1, 0] = torch.tensor([-0.5, 600.0, -3.7])        # trunc(-0.5) = 0 is a bin; the other two are outside
    xs[0][1, 1, ::2], xs[0][1, 1, 1::2] = 80.0, -80.0
    xs[1][1, 1, :300], xs[1][1, 1, 300:] = -80.0, 80.0
    weight[1, 2] = 0.0
    _, grads = sd_check(f"simdr edges ls={ls}", xs, target, weight, ls)
    assert not grads[0][1, 2].any() and not grads[1][1, 2].any()       # the weight-0 row
    sd_check(f"simdr edges ls={ls} weight=None", xs, target, None, ls)


# ---------------------------------------------------------------- 2. packed views
def test_simdr_packed_views_equal_contiguous_copies():
    g = torch.Generator().manual_seed(21)
    B, J, n = 3, 5, 24
    packed = (torch.randn(B, J, 3, n, generator=g) * 2).to(DEV).requires_grad_(True)
    target = (torch.randint(0, n, (B, J, 3), generator=g).float() + 0.6).to(DEV)
    weight = torch.rand(B, J, generator=g).to(DEV)
    loss_p = ops.simdr_loss(packed[:, :, 0], packed[:, :, 1], packed[:, :, 2], target, weight, 0.2)
    loss_p.backward()
    copies = [packed.detach()[:, :, a].contiguous().requires_grad_(True) for a in range(3)]
    loss_c = ops.simdr_loss(*copies, target, weight, 0.2)
    loss_c.backward()
    assert same_bits(loss_p, loss_c)
    assert packed.grad is not None and packed.grad.shape == packed.shape
    for a in range(3):
        assert same_bits(packed.grad[:, :, a], copies[a].grad)


# ---------------------------------------------------------------- 3. guard regions and alignment (straight through the C ABI)
def guarded(n, off):
    buf = torch.full((n + 8,), SENT, dtype=torch.float32, device=DEV)
    return buf, buf[off:off + n]


def untouched(buf, off, n):
    return bool((buf[:off] == SENT).all().item() and (buf[off + n:] == SENT).all().item())


@pytest.mark.parametrize("B,J,H,W", [(2, 3, 8, 12), (2, 3, 7, 5), (1, 2, 64, 48), (3, 7, 1, 1)])
def test_heatmap_outputs_stay_inside_their_buffers_at_every_alignment(B, J, H, W):
    L = _lib.lib()
    st = _lib.current_stream_handle()
    pred, joints = hm_inputs(B, J, H, W, seed=31)
    pred, joints = pred.to(DEV), joints.reshape(-1, 2).contiguous().to(DEV)
    gloss = torch.tensor([1.7], device=DEV)
    Rn, N = B * J, B * J * H * W
    nbytes = L.hp_joints_mse_workspace_bytes(B, J)
    first = None
    for off in range(4):
        fb, flags = guarded(Rn, off)
        lb, loss = guarded(1, off)
        db, dpred = guarded(N, off)
        tb, target = guarded(N, off)
        rb, rflags = guarded(Rn, off)
        wb = torch.full((nbytes // 4 + 8,), SENT, dtype=torch.float32, device=DEV)      # an exact-size workspace, guarded behind
        _lib.check(L.hp_joints_mse_forward(pred.data_ptr(), joints.data_ptr(), B, J, H, W, 2.0, 1, flags.data_ptr(), loss.data_ptr(),
                                           wb.data_ptr(), nbytes, st), "forward")
        _lib.check(L.hp_joints_mse_backward(pred.data_ptr(), joints.data_ptr(), flags.data_ptr(), gloss.data_ptr(), B, J, H, W, 2.0, 1,
                                            dpred.data_ptr(), st), "backward")
        _lib.check(L.hp_joint_heatmaps(joints.data_ptr(), None, Rn, H, W, 2.0, 6.0, target.data_ptr(), rflags.data_ptr(), st), "render")
        torch.cuda.synchronize()
        assert untouched(fb, off, Rn) and untouched(lb, off, 1) and untouched(db, off, N) and untouched(tb, off, N) and untouched(rb, off, Rn)
        assert bool((wb[nbytes // 4:] == SENT).all().item())
        assert not (dpred == SENT).any() and not (target == SENT).any() and not (flags == SENT).any() and loss.item() != SENT
        got = [flags.clone(), loss.clone(), dpred.clone(), target.clone(), rflags.clone()]
        if first is None:
            first = got
        for a, b in zip(got, first):
            assert same_bits(a, b), off
    # the prediction's own alignment does not change a bit either (the element -> thread assignment ignores it)
    pb, p1 = guarded(N, 1)
    p1.copy_(pred.reshape(-1))
    flags, loss, dpred = (torch.empty(k, device=DEV) for k in (Rn, 1, N))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(L.hp_joints_mse_forward(p1.data_ptr(), joints.data_ptr(), B, J, H, W, 2.0, 1, flags.data_ptr(), loss.data_ptr(),
                                       ws.data_ptr(), nbytes, st), "forward")
    _lib.check(L.hp_joints_mse_backward(p1.data_ptr(), joints.data_ptr(), flags.data_ptr(), gloss.data_ptr(), B, J, H, W, 2.0, 1,
                                        dpred.data_ptr(), st), "backward")
    assert same_bits(loss, first[1]) and same_bits(dpred, first[2])


@pytest.mark.parametrize("bins", [(16, 24, 7), (513, 64, 2)])
def test_simdr_outputs_stay_inside_their_buffers_at_every_alignment(bins):
    L = _lib.lib()
    st = _lib.current_stream_handle()
    B, J = 2, 3
    xs, target, weight = sd_inputs(bins, B, J, seed=41)
    xs = [x.to(DEV) for x in xs]
    target, weight = target.reshape(-1, 3).contiguous().to(DEV), weight.reshape(-1).contiguous().to(DEV)
    gloss = torch.tensor([0.6], device=DEV)
    Rn = B * J
    nbytes = L.hp_simdr_loss_workspace_bytes(B, J)
    first = None
    for off in range(4):
        sb, stat = guarded(Rn * 6, off)
        lb, loss = guarded(1, off)
        gb = [guarded(Rn * n, off) for n in bins]
        wb = torch.full((nbytes // 4 + 8,), SENT, dtype=torch.float32, device=DEV)
        pre = [xs[0].data_ptr(), bins[0], bins[0], xs[1].data_ptr(), bins[1], bins[1], xs[2].data_ptr(), bins[2], bins[2],
               target.data_ptr(), weight.data_ptr(), B, J, 0.2]
        _lib.check(L.hp_simdr_loss_forward(*pre, stat.data_ptr(), loss.data_ptr(), wb.data_ptr(), nbytes, st), "forward")
        _lib.check(L.hp_simdr_loss_backward(*pre, stat.data_ptr(), gloss.data_ptr(), *(v.data_ptr() for _, v in gb), st), "backward")
        torch.cuda.synchronize()
        assert untouched(sb, off, Rn * 6) and untouched(lb, off, 1) and bool((wb[nbytes // 4:] == SENT).all().item())
        for (buf, v), n in zip(gb, bins):
            assert untouched(buf, off, Rn * n) and not (v == SENT).any()
        assert not (stat == SENT).any() and loss.item() != SENT
        got = [stat.clone(), loss.clone()] + [v.clone() for _, v in gb]
        if first is None:
            first = got
        for a, b in zip(got, first):
            assert same_bits(a, b), off


# ---------------------------------------------------------------- 4. reproducibility
def test_two_calls_give_the_same_bits():
    pred, joints = hm_inputs(2, 16, 64, 48, seed=51)
    runs = []
    for _ in range(2):
        p = pred.to(DEV).requires_grad_(True)
        loss, _ = ops.joints_mse(p, joints.to(DEV), 2.0, False)
        loss.backward()
        runs.append((loss.detach(), p.grad))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])
    xs, target, weight = sd_inputs((1000, 64, 7), B=4, J=16, seed=52)
    a, b = sd_run(xs, target, weight, 0.2), sd_run(xs, target, weight, 0.2)
    assert same_bits(a[0], b[0]) and all(same_bits(u, v) for u, v in zip(a[1], b[1]))


# ---------------------------------------------------------------- 5. autograd
def within_one_ulp(a, b):
    a, b = bits(a).long(), bits(b).long()
    return bool(((a - b).abs() <= 1).all().item())


def test_a_scaled_loss_scales_the_gradient_and_a_host_target_equals_a_device_target():
    pred, joints = hm_inputs(2, 3, 7, 5, seed=61)
    grads = []
    for scale, tgt in ((1.0, joints.to(DEV)), (3.0, joints.to(DEV)), (1.0, joints)):      # the last: target on the host
        p = pred.to(DEV).requires_grad_(True)
        loss, flags = ops.joints_mse(p, tgt, 2.0, True)
        assert not flags.requires_grad
        (loss * scale).backward()
        grads.append((loss.detach(), p.grad))
    assert within_one_ulp(grads[1][1], 3.0 * grads[0][1])
    assert same_bits(grads[2][0], grads[0][0]) and same_bits(grads[2][1], grads[0][1])
    xs, target, weight = sd_inputs((16, 600, 7), seed=62)
    plain = sd_run(xs, target, weight, 0.2)[1]
    leaves = [x.to(DEV).requires_grad_(True) for x in xs]
    (3.0 * ops.simdr_loss(*leaves, target, weight, 0.2)).backward()           # target and weight on the host
    for a in range(3):
        assert within_one_ulp(leaves[a].grad, 3.0 * plain[a])


def test_joints_mse_loss_module_keeps_the_flags_and_leaves_the_callers_weights_alone(golden):
    from hiddenpose_amd.config import get_cfg_defaults

    g = golden("head_losses.npz")
    cfg = get_cfg_defaults()
    cfg.DATASET.NUM_JOINTS, cfg.DATASET.HEATMAP_SIZE = 5, [12, 8]
    cfg.LOSS.TYPE = "JointsMSELoss"
    crit = Cr.get_criterion(cfg)
    tw = torch.full((3, 5, 1), 0.25)
    loss = crit(torch.from_numpy(g["hm_pred"]).to(DEV), torch.from_numpy(g["hm_joints"]), tw)
    assert abs(loss.item() / float(g["hm_loss_0"]) - 1) < 2e-6
    assert crit.last_target_weight.shape == (3, 5, 1) and crit.last_target_weight.is_cuda
    assert np.array_equal(crit.last_target_weight.cpu().numpy()[:, :, 0], g["hm_flags_0"]) and bool((tw == 0.25).all())


# ---------------------------------------------------------------- 6. heads trained end to end
def grads_of(model):
    return torch.cat([p.grad.reshape(-1) for p in model.parameters() if p.grad is not None])


def test_tokenpose_trains_on_the_heatmap_loss():
    """TokenPose at tests/test_xformers.py's small learnable-embedding config (8 x 6 heat-maps, 5 keypoints): the first step's
    parameter gradients against those of the float64 model's d loss / d output fed through the same head backward, then three
    steps of train_2d_heatmap with HipAdam on one batch: the loss falls."""
    from hiddenpose_amd.config import get_cfg_defaults
    from hiddenpose_amd.optimizer import HipAdam
    from hiddenpose_amd.train_heads import train_2d_heatmap
    from test_xformers import _tp

    cfg = get_cfg_defaults()
    cfg.DATASET.NUM_JOINTS, cfg.DATASET.HEATMAP_SIZE, cfg.DATASET.SIGMA = 5, [6, 8], 1
    cfg.LOSS.TYPE = "JointsMSELoss"
    crit = Cr.get_criterion(cfg)
    m, feat = _tp("learnable")
    m = m.to(DEV).train()
    target = torch.tensor([[1.5, 2.2, 1.0], [4.9, 7.0, 1.0], [-3.0, 3.0, 1.0], [2.0, 5.5, 1.0], [3.3, 0.4, 1.0]])[None].repeat(2, 1, 1)
    target[1, :, 0] += 0.7
    # step 1 by hand: the criterion's gradients against the float64 model's through the same backward
    y = m(feat.to(DEV))
    assert y.shape == (2, 5, 8, 6)
    m.zero_grad(set_to_none=True)
    crit(y, target[:, :, :2], None).backward()
    got = grads_of(m).clone()
    l64, d64, _ = R.joints_mse(y.detach().cpu(), target[:, :, :2], 1, False, torch.float64)
    _, d32, _ = R.joints_mse(y.detach().cpu(), target[:, :, :2], 1, False, torch.float32)
    m.zero_grad(set_to_none=True)
    m(feat.to(DEV)).backward(d64.float().to(DEV))
    want = grads_of(m).clone()
    e, e_ref = R.rel_l2(got, want), R.rel_l2(d32, d64)
    print(f"head-loss e2e tokenpose parameter gradients: hip {e:.3e} fp32-model d loss / d output {e_ref:.3e} bar {R.bar(e_ref):.3e}")
    assert e <= R.bar(e_ref)
    m.zero_grad(set_to_none=True)
    opt = HipAdam(m.parameters(), lr=1e-3)
    losses = train_2d_heatmap(cfg, [(feat, target)] * 3, m, crit, opt, 0, None, None).cpu()
    assert abs(losses[0].item() / l64 - 1) < 1e-5
    assert losses[2] < losses[1] < losses[0], losses


class _SimdrStandIn(torch.nn.Module):
    def __init__(self, J=5, bins=16):
        super().__init__()
        self.J, self.bins = J, bins
        self.fc = torch.nn.Linear(8, J * 3 * bins)

    def forward(self, x):
        return self.fc(x).reshape(x.shape[0], self.J, 3, self.bins)


def test_a_simdr_head_trains_through_train_simdr():
    from hiddenpose_amd.optimizer import HipAdam
    from hiddenpose_amd.train_heads import train_simdr

    torch.manual_seed(71)
    m = _SimdrStandIn().to(DEV)
    g = torch.Generator().manual_seed(72)
    x = torch.randn(4, 8, generator=g)
    target = torch.randint(0, 16, (4, 5, 3), generator=g).float() + 0.6
    crit = Cr.NMTNORMCritierion(0.2)
    y = m(x.to(DEV))
    crit(y[:, :, 0], y[:, :, 1], y[:, :, 2], target.to(DEV), None).backward()
    got = grads_of(m).clone()
    yc = y.detach().cpu()
    l64, d64 = R.simdr([yc[:, :, a] for a in range(3)], target, None, 0.2, torch.float64)
    _, d32 = R.simdr([yc[:, :, a] for a in range(3)], target, None, 0.2, torch.float32)
    m.zero_grad(set_to_none=True)
    m(x.to(DEV)).backward(torch.stack(d64, dim=2).float().to(DEV))
    want = grads_of(m).clone()
    e, e_ref = R.rel_l2(got, want), R.rel_l2(torch.stack(d32, dim=2), torch.stack(d64, dim=2))
    print(f"head-loss e2e simdr parameter gradients: hip {e:.3e} fp32-model d loss / d output {e_ref:.3e} bar {R.bar(e_ref):.3e}")
    assert e <= R.bar(e_ref)
    m.zero_grad(set_to_none=True)
    losses = train_simdr(None, [(x, target)] * 3, m, crit, HipAdam(m.parameters(), lr=1e-2), 0, None, None).cpu()
    assert abs(losses[0].item() / l64 - 1) < 1e-5
    assert losses[2] < losses[1] < losses[0], losses


class _Heat3dStandIn(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(4, 3 * 64)

    def forward(self, x):
        return self.fc(x).reshape(x.shape[0], 3, 4, 4, 4)


def test_train_3d_heatmap_runs_a_step_on_the_soft_argmax_loss():
    from hiddenpose_amd.config import get_cfg_defaults
    from hiddenpose_amd.optimizer import HipAdam
    from hiddenpose_amd.train_heads import train_3d_heatmap

    torch.manual_seed(81)
    m = _Heat3dStandIn().to(DEV)
    before = m.fc.weight.detach().clone()
    crit = Cr.get_criterion(get_cfg_defaults())
    assert type(crit) is Cr.L2JointLocationLoss
    g = torch.Generator().manual_seed(82)
    losses = train_3d_heatmap(None, [(torch.randn(2, 4, generator=g), torch.rand(2, 3, 3, generator=g) * 3)], m, crit,
                              HipAdam(m.parameters(), lr=1e-2), 0, None, None)
    assert losses.shape == (1,) and torch.isfinite(losses).all() and losses[0] > 0
    assert not torch.equal(before, m.fc.weight.detach())
