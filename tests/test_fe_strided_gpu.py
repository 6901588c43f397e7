"""GPU parity of FeatureExtraction at stride 2 and basedim > 1 (csrc/fe_entry_kernels.hip, hp_fe_entry_* / hp_bcast_add_forward /
hp_channel_sum): the entry kernels and the broadcast join against float64 CPU evaluations of the reference operators
(ReplicationPad3d(1) + Conv3d(stride), feature_extraction.py:147-155; conv3d(stride, padding 1), :167; the broadcast add,
:170), the module and the network against goldens captured from the reference
(tests/golden/make_feature_extraction_goldens.py).

Bars: the entry kernels are the same 27-tap fp32 arithmetic as test_dconv_gpu.py::test_dconv3 and carry its bars (2e-6 on
outputs and the input gradient, 1e-5 on weight / bias gradients); the module cases carry the bars of
test_stages_gpu.py::test_feature_extraction_and_unet_vs_golden (1e-5 / 1e-4), the network case the 1e-3 of
test_nlospose_gpu.py::test_eval_forward_T32_vs_reference_golden."""
import pytest
import torch
import torch.nn.functional as F

from hiddenpose_amd import hip_ops as ops
from hiddenpose_amd import testing as hpt
from util import rel_l2

pytestmark = pytest.mark.gpu

# (B, C, D, H, W)
S2_CASES = [
    (2, 2, 5, 6, 7),      # mixed parities
    (1, 1, 8, 8, 8),      # all even: the right pad is never read
    (1, 3, 9, 5, 70),     # odd C, x past one wave's tile of the input gradient
    (1, 5, 1, 3, 2), (1, 2, 2, 2, 2),   # extents of 1 and 2: every tap clamps
    (1, 1, 1, 1, 1),
    (2, 9, 4, 7, 33),     # C past one register group (three groups of 4), W % 4 != 0
    (1, 4, 37, 4, 16),    # z walk split over several workgroups, 16-byte path
    (1, 1, 136, 9, 8),    # more partial records (18) than the reduction has slices (16)
    # x tile of the forward / weight gradient: 128 outputs (Wo = 127, 128, 128 on the 16-byte path, 129)
    (1, 2, 2, 3, 253), (1, 2, 2, 3, 255), (1, 1, 2, 3, 256), (1, 2, 2, 3, 257),
    # y tile: 4 output rows (Ho = 3, 4, 5)
    (1, 2, 3, 5, 6), (1, 2, 3, 7, 8), (1, 2, 3, 9, 6),
    # z: at most ceil(Do / 8) chunks per column (Do = 7, 8: one chunk; 9: two, of 5 and 4 planes)
    (1, 2, 13, 3, 4), (1, 2, 15, 3, 4), (1, 2, 17, 3, 4),
    # tile of the input gradient: 64 x 4 input voxels
    (1, 2, 2, 3, 63), (1, 2, 2, 4, 64), (1, 2, 2, 5, 65),
]
S1_CASES = [
    (1, 3, 5, 6, 7), (2, 4, 3, 9, 66),
    (1, 1, 5, 6, 8), (2, 1, 3, 5, 7),                          # C = 1: reachable through the ABI only (the module keeps its fused path)
    (1, 2, 2, 3, 255), (1, 2, 2, 3, 256), (1, 2, 2, 3, 257),   # x tile: 256 outputs
    (1, 2, 3, 3, 5), (1, 2, 3, 4, 8), (1, 2, 3, 5, 5),         # y tile: 4 rows
    (1, 2, 7, 3, 4), (1, 2, 8, 3, 4), (1, 2, 9, 3, 4),         # z chunk: 8 planes
    (1, 5, 4, 5, 12),                                          # three channel groups of 2
]
CASES = [(2,) + c for c in S2_CASES] + [(1,) + c for c in S1_CASES]


def entry_reference(x, w, b, wb, s, ga, gb):
    """float64 (a, box) and the gradients of sum(a * ga) + sum(box * gb) wrt (x, w, b, wb)."""
    xd, wd, bd, wbd = (t.double().requires_grad_(True) for t in (x, w, b, wb))
    a = F.conv3d(F.pad(xd, (1,) * 6, mode="replicate"), wd, bd, stride=s)
    box = F.conv3d(xd, wbd, stride=s, padding=1)
    if ga is None:
        return a, box
    ((a * ga.double()).sum() + (box * gb.double()).sum()).backward()
    return a.detach(), box.detach(), xd.grad, wd.grad, bd.grad, wbd.grad


def entry_inputs(s, dims):
    B, C, D, H, W = dims
    g = torch.Generator().manual_seed(1000 * s + 100 * C + D + H + W)
    x = torch.randn(B, 1, D, H, W, generator=g)
    w = torch.randn(C, 1, 3, 3, 3, generator=g) * 0.2
    b = torch.randn(C, generator=g)
    wb = torch.randn(1, 1, 3, 3, 3, generator=g) * 0.2
    do, ho, wo = ((n - 1) // s + 1 for n in (D, H, W))
    ga = torch.randn(B, C, do, ho, wo, generator=g)
    gb = torch.randn(B, 1, do, ho, wo, generator=g)
    return x, w, b, wb, ga, gb


@pytest.mark.parametrize("s,B,C,D,H,W", CASES)
def test_fe_entry_vs_float64(s, B, C, D, H, W):
    x, w, b, wb, ga, gb = entry_inputs(s, (B, C, D, H, W))
    ra, rbox, rgx, rgw, rgb, rgwb = entry_reference(x, w, b, wb, s, ga, gb)
    xg, wg, bg, wbg = (t.cuda().requires_grad_(True) for t in (x, w, b, wb))
    a, box = ops.fe_entry(xg, wg, bg, wbg, s)
    assert a.shape == ra.shape and box.shape == rbox.shape
    ((a * ga.cuda()).sum() + (box * gb.cuda()).sum()).backward()
    errs = {"a": rel_l2(a, ra), "box": rel_l2(box, rbox), "gx": rel_l2(xg.grad, rgx), "dw": rel_l2(wg.grad, rgw),
            "dbias": rel_l2(bg.grad, rgb), "dweights": rel_l2(wbg.grad, rgwb)}
    print(errs)
    assert errs["a"] < 2e-6 and errs["box"] < 2e-6 and errs["gx"] < 2e-6, errs
    assert errs["dw"] < 1e-5 and errs["dbias"] < 1e-5 and errs["dweights"] < 1e-5, errs


@pytest.mark.parametrize("s,dims", [(2, (2, 3, 5, 6, 7)), (1, (2, 3, 5, 6, 7))])
def test_fe_entry_parameter_gradients_without_input_gradient(s, dims):
    x, w, b, wb, ga, gb = entry_inputs(s, dims)
    _, _, _, rgw, rgb, rgwb = entry_reference(x, w, b, wb, s, ga, gb)
    xg = x.cuda()
    wg, bg, wbg = (t.cuda().requires_grad_(True) for t in (w, b, wb))
    a, box = ops.fe_entry(xg, wg, bg, wbg, s)
    ((a * ga.cuda()).sum() + (box * gb.cuda()).sum()).backward()
    assert xg.grad is None
    assert rel_l2(wg.grad, rgw) < 1e-5 and rel_l2(bg.grad, rgb) < 1e-5 and rel_l2(wbg.grad, rgwb) < 1e-5


def test_fe_entry_weight_gradients_are_bit_reproducible():
    x, w, b, wb, ga, gb = entry_inputs(2, (2, 3, 9, 5, 70))
    grads = []
    for _ in range(2):
        xg, wg, bg, wbg = (t.cuda().requires_grad_(True) for t in (x, w, b, wb))
        a, box = ops.fe_entry(xg, wg, bg, wbg, 2)
        ((a * ga.cuda()).sum() + (box * gb.cuda()).sum()).backward()
        grads.append((wg.grad, bg.grad, wbg.grad))
    for g0, g1 in zip(*grads):
        assert torch.equal(g0, g1)


# (B, C, D, H, W) of the output-sized tensors; the last three: one short of / equal to / past the 1024 elements of a workgroup
@pytest.mark.parametrize("dims", [(2, 3, 3, 5, 7), (1, 1, 2, 2, 2), (1, 2, 1, 3, 341), (2, 2, 1, 4, 256), (1, 3, 1, 5, 205)])
def test_broadcast_join_vs_float64(dims):
    B, C, D, H, W = dims
    g = torch.Generator().manual_seed(31 + C + W)
    t = torch.randn(B, C, D, H, W, generator=g)
    box = torch.randn(B, 1, D, H, W, generator=g)
    gy = torch.randn(B, C, D, H, W, generator=g)
    td, bd = t.double().requires_grad_(True), box.double().requires_grad_(True)
    ref = td + bd
    (ref * gy.double()).sum().backward()
    tg, bgp = t.cuda().requires_grad_(True), box.cuda().requires_grad_(True)
    y = ops.bcast_add(tg, bgp)
    (y * gy.cuda()).sum().backward()
    # one fp32 add per output; C - 1 fp32 adds per element of the box gradient
    assert rel_l2(y, ref) < 2e-7
    assert rel_l2(tg.grad, td.grad) < 2e-7
    assert rel_l2(bgp.grad, bd.grad) < 2e-7 * max(C, 1)


MODULE_CASES = {"c2_default": (2, None, (2, 8, 10, 12)), "c3_s1": (3, 1, (2, 5, 6, 7)), "c1_s2": (1, 2, (2, 7, 9, 11))}


@pytest.mark.parametrize("key", sorted(MODULE_CASES))
def test_module_vs_reference_golden(golden, key):
    from hiddenpose_amd.feature_extraction import FeatureExtraction

    g = golden("feature_extraction_strided.npz")
    basedim, stride, (B, T, H, W) = MODULE_CASES[key]
    fe = FeatureExtraction(basedim, 1) if stride is None else FeatureExtraction(basedim, 1, stride=stride)
    assert fe.stride == (2 if stride is None else stride)
    hpt.fill_module(fe, "feature_extraction.")
    fe = fe.cuda()
    x = hpt.synthetic_meas(B, T, max(H, W), "transient", seed=410)[:, :, :, :H, :W].contiguous().cuda().requires_grad_(True)
    y = fe(x)
    assert tuple(y.shape) == g[key + "_y"].shape
    _, C, To, Ho, Wo = y.shape
    gy = torch.cat([hpt.synthetic_meas(B, To, max(Ho, Wo), "uniform", seed=101 + 7 * c)[:, :, :, :Ho, :Wo] for c in range(C)], 1) - 0.5
    (y * gy.contiguous().cuda()).sum().backward()
    assert rel_l2(y, g[key + "_y"]) < 1e-5 and rel_l2(x.grad, g[key + "_gx"]) < 1e-5
    for k, p in fe.named_parameters():
        assert rel_l2(p.grad, g[key + "_g_" + k]) < 1e-4, k


def test_network_with_fe_stride_2_vs_reference_golden(golden):
    from hiddenpose_amd.config import make_cfg
    from hiddenpose_amd.NlosPose import NlosPose

    g = golden("feature_extraction_strided.npz")
    cfg = make_cfg(32, 32)
    assert NlosPose(cfg).feature_extraction.stride == 1   # the key is optional: absent = the reference's network
    cfg.MODEL.FE_STRIDE = 2
    model = NlosPose(cfg)
    assert model.feature_extraction.stride == 2
    hpt.fill_module(model)
    model = model.cuda().eval()
    with torch.no_grad():
        heat, refine = model(hpt.synthetic_meas(2, 64, 64).cuda())
    assert heat.shape == (2, 24, 16, 16, 16) and refine.shape == (2, 1, 32, 32, 32)
    assert rel_l2(heat, g["net_eval_heat"]) < 1e-3
    assert rel_l2(refine, g["net_eval_refine"]) < 1e-3


def test_stride_1_basedim_1_path_is_unchanged():
    from hiddenpose_amd.feature_extraction import FeatureExtraction

    fe = FeatureExtraction(1, 1, stride=1)
    hpt.fill_module(fe, "feature_extraction.")
    fe = fe.cuda()
    x = hpt.synthetic_meas(2, 9, 12).cuda()
    with torch.no_grad():
        assert torch.equal(fe(x), ops.feature_extraction_fused(x, fe))


def test_unsupported_stride_names_the_supported_set():
    from hiddenpose_amd.feature_extraction import FeatureExtraction

    fe = FeatureExtraction(1, 1, stride=3).cuda()
    with pytest.raises(NotImplementedError, match="stride 1 or 2"):
        fe(torch.zeros(1, 1, 4, 4, 4, device="cuda"))
