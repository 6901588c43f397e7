"""The memory-bound stages of csrc/unet_kernels.hip and the stage half of csrc/misc_kernels.hip at their launch edges: the
second trip of every grid-stride loop (grids are capped at 2048 workgroups of 256 threads: 524,288 items), the `+= 256` loops
that fill the per-workgroup interpolation tables, the scalar tails behind the 16-byte loops, the tie rules (first maximum of a
pool window, first occurrence of a volume's min / max, smaller depth index first), the entry points and the number ranges the
small shapes of test_stages_gpu.py / test_aux_gpu.py never reach.

Exact operations are compared exactly; the others by tests/stage_ref.py's bar rule against float64 on the CPU, evaluated once
more over only the elements the branch produces.  Every shape is the smallest that reaches its branch."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import stage_ref as R
from hiddenpose_amd import _lib
from hiddenpose_amd import hip_ops as ops
from oracle import nlospose_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def call(name, *args):
    """an entry point of the C ABI on the current stream, tensors passed as device pointers"""
    a = [t.data_ptr() if torch.is_tensor(t) else t for t in args]
    _lib.check(getattr(_lib.lib(), name)(*a, torch.cuda.current_stream().cuda_stream), name)


def leaf(t):
    return t.cuda().requires_grad_(True)


# ---------------------------------------------------------------- 1. GroupNorm + ReLU
def gn_chunks(V, planes):   # chunks_for of csrc/unet_kernels.hip
    return max(1, min(max(1, 2048 // max(planes, 1)), (V // 4 + R.WG - 1) // R.WG))


# (2,32,11,30,101): V = 33,330, V % 4 = 2 and V / 4 = 8,332 > 32 chunks x 256 -- second trip and a live tail;
# (2,6,3,5,7): V = 105 is odd, planes start on 4-byte boundaries; (1,4,1,1,3): V < 4, the tail alone
@pytest.mark.parametrize("offset", [0.25, 8.0])
@pytest.mark.parametrize("shape,G", [((2, 32, 11, 30, 101), 4), ((2, 6, 3, 5, 7), 1), ((2, 6, 3, 5, 7), 6), ((1, 4, 1, 1, 3), 4)])
def test_groupnorm_relu_second_trip_tail_and_offset_mean(shape, G, offset):
    """offset 8: |mean| / std = 8, where the variance E[x^2] - m^2 loses 2 * log2(8) + 1 bits of whatever precision the two
    sums were formed in.  The ReLU mask of the backward is a step function of z: the incoming gradient is zero within
    1e-4 max|a| of the kink (at most 1e-3 of the elements: a condition of the test)."""
    g = gen(11 + G)
    B, C = shape[:2]
    V = int(np.prod(shape[2:]))
    z = torch.randn(shape, generator=g) + offset
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)
    gy, share = R.mask_near_relu_kink(z, gamma, beta, torch.randn(shape, generator=g), G)
    print(f"[stage-edge] groupnorm {shape} G={G} +{offset}: gradient zeroed near the ReLU kink on {share:.2e} of the elements")
    assert share <= 1e-3
    ref = R.groupnorm_relu(z, gamma, beta, gy, G, torch.float64)
    r32 = R.groupnorm_relu(z, gamma, beta, gy, G, torch.float32)
    zg, gg, bg = leaf(z), leaf(gamma), leaf(beta)
    y = ops._GroupNormRelu.apply(zg, gg, bg, G, 1e-5)
    (y * gy.cuda()).sum().backward()
    chunks = gn_chunks(V, B * C)
    sub = {"tail": R.plane_tail(B * C, V), "second trip": R.plane_range(B * C, V, 4 * chunks * R.WG, 4 * (V // 4))}
    tag = f"groupnorm {shape} G={G} +{offset}"
    R.judge(tag + " y", y, ref[0], r32[0], 1e-6, sub)
    R.judge(tag + " dz", zg.grad, ref[1], r32[1], 1e-5, sub)
    R.judge(tag + " dgamma", gg.grad, ref[2], r32[2], 1e-5)
    R.judge(tag + " dbeta", bg.grad, ref[3], r32[3], 1e-5)


# ---------------------------------------------------------------- 2. MaxPool3d(2)
@pytest.fixture(scope="module")
def pool_case():
    """3 x 31 x 65 x 94 = 568,230 pooled voxels (> 524,288); values in {0, 1, 2}: every window has ties.  The CPU gives each
    window's gradient to exactly one element, the first maximum in d, h, w order."""
    g = gen(21)
    x = torch.randint(0, 3, (1, 3, 62, 130, 188), generator=g).float()
    xd = x.double().requires_grad_(True)
    ref = F.max_pool3d(xd, 2, 2)
    gy = torch.randn(ref.shape, generator=g)
    (ref * gy.double()).sum().backward()
    assert ref.numel() > R.TRIP and int((xd.grad != 0).sum()) <= ref.numel()
    return x, gy, ref.detach().float(), xd.grad.float(), torch.randn(x.shape, generator=g)


def test_maxpool2_ties_everywhere_beyond_one_grid(pool_case):
    x, gy, ref, gref, _ = pool_case
    xg = leaf(x)
    y = ops.max_pool3d_2(xg)
    (y * gy.cuda()).sum().backward()
    assert torch.equal(y.detach().cpu(), ref)
    assert R.same_bits(xg.grad, gref)


@pytest.mark.parametrize("use", ["both", "pool"])
def test_pool_and_skip_ties_everywhere_beyond_one_grid(pool_case, use):
    x, gy, ref, gref, wskip = pool_case
    xg = leaf(x)
    skip, pooled = ops.pool_and_skip(xg)
    assert torch.equal(skip.detach().cpu(), x) and torch.equal(pooled.detach().cpu(), ref)
    loss = (pooled * gy.cuda()).sum()
    if use == "both":
        loss = loss + (skip * wskip.cuda()).sum()
    loss.backward()
    # one routed value (or zero) plus the skip gradient: a single correctly rounded float32 add
    assert R.same_bits(xg.grad, gref + wskip if use == "both" else gref)


# ---------------------------------------------------------------- 3. trilinear x2 upsample + concat
def ups_subsets(shape, limit, trips):
    sub = {}
    for ax in (2, 3, 4):
        if shape[ax] > limit:
            sub[f"table wrap axis {ax}"] = R.axis_from(shape, ax, limit)
    n = int(np.prod(shape))
    for k in trips:
        if n > k * R.TRIP:
            sub[f"items beyond {k} x 524288"] = R.beyond_first_trip(n, 1, k * R.TRIP)
    return sub


# tables: (2,2,260), (2,258,4), (130,2,4) separable (an axis beyond 256 outputs / inputs); (2,2,259) fused, D+H+W = 263 entries
# second trips: (31,33,35) fused forward, 572,880 outputs; (66,64,63) fused adjoint, 532,224 inputs; (40,40,84) both separable
# templates, >= 524,288 items in a pass each way
@pytest.mark.parametrize("c1,dims", [(1, (2, 2, 260)), (1, (2, 258, 4)), (1, (130, 2, 4)), (1, (2, 2, 259)), (2, (31, 33, 35)),
                                     (2, (66, 64, 63)), (2, (40, 40, 84))])
def test_upsample_cat_table_loops_and_second_trips(c1, dims):
    g = gen(31)
    x1 = torch.randn(1, c1, *dims, generator=g)
    skip = torch.randn(1, 1, *(2 * d for d in dims), generator=g)
    gy = torch.randn(1, 1 + c1, *(2 * d for d in dims), generator=g)
    ref = R.upsample_cat(x1, skip, gy, torch.float64)
    r32 = R.upsample_cat(x1, skip, gy, torch.float32)
    ag, bg = leaf(x1), leaf(skip)
    y = ops.upsample_cat(ag, bg)
    (y * gy.cuda()).sum().backward()
    assert torch.equal(y[:, :1].detach().cpu(), skip) and torch.equal(bg.grad.cpu(), gy[:, :1])
    up_shape = (1, c1) + tuple(2 * d for d in dims)
    # fused forward tables hold 2 (D + H + W) entries, the w axis last: its entries wrap from output 256 - 2 (D + H) on
    R.judge(f"upsample {dims} y", y[:, 1:].contiguous(), ref[0][:, 1:].contiguous(), r32[0][:, 1:].contiguous(), 1e-6,
            ups_subsets(up_shape, 248, (1, 4)))
    R.judge(f"upsample {dims} dx", ag.grad, ref[1], r32[1], 1e-6, ups_subsets(tuple(x1.shape), 250, (1,)))


@pytest.mark.parametrize("kind,dims", [("_ws", (3, 5, 8)), ("", (3, 4, 5))])
def test_upsample_entry_points_write_and_read_only_their_channel_slice(kind, dims):
    """C ABI, B = 2: C = 3 channels into / out of slice c_off = 2 of Ctot = 7.  `_ws` on W % 4 == 0 runs the separable passes,
    the raw entries on an odd W the fused kernels."""
    g = gen(32)
    B, C, Ctot, c_off = 2, 3, 7, 2
    D, H, W = dims
    x = torch.randn(B, C, D, H, W, generator=g)
    gy = torch.randn(B, C, 2 * D, 2 * H, 2 * W, generator=g)
    ref, r32 = R.upsample(x, gy, torch.float64), R.upsample(x, gy, torch.float32)
    L = _lib.lib()
    fws = torch.empty(max(1, int(L.hp_upsample_trilinear2x_forward_workspace_bytes(B, C, D, H, W)) // 4), device="cuda")
    bws = torch.empty(max(1, int(L.hp_upsample_trilinear2x_backward_workspace_bytes(B, C, D, H, W)) // 4), device="cuda")
    buf = torch.full((B, Ctot, 2 * D, 2 * H, 2 * W), -777.25, device="cuda")
    call("hp_upsample_trilinear2x_forward" + kind, x.cuda(), buf, B, C, D, H, W, Ctot, c_off, *([fws] if kind else []))
    out = buf.cpu()
    assert bool((out[:, :c_off] == -777.25).all()) and bool((out[:, c_off + C:] == -777.25).all())
    R.judge(f"upsample{kind} {dims} slice y", out[:, c_off:c_off + C].contiguous(), ref[0], r32[0], 1e-6)
    dxs = []
    for outside in (0.0, NAN):
        dy = torch.full((B, Ctot, 2 * D, 2 * H, 2 * W), outside)
        dy[:, c_off:c_off + C] = gy
        dx = torch.full((B, C, D, H, W), NAN, device="cuda")
        call("hp_upsample_trilinear2x_backward" + kind, dy.cuda(), dx, B, C, D, H, W, Ctot, c_off, *([bws] if kind else []))
        dxs.append(dx.cpu())
    assert R.same_bits(dxs[0], dxs[1])
    R.judge(f"upsample{kind} {dims} slice dx", dxs[0], ref[1], r32[1], 1e-6)


def test_upsample_cat_in_place_buffer_equals_the_copying_path():
    g = gen(33)
    x1, skip = torch.randn(1, 2, 4, 6, 8, generator=g).cuda(), torch.randn(1, 3, 8, 12, 16, generator=g).cuda()
    y1 = ops.upsample_cat(x1, skip)
    buf = torch.full((1, 5, 8, 12, 16), NAN, device="cuda")
    buf[:, :3] = skip
    y2 = ops.upsample_cat(x1, buf[:, :3], buf)
    assert y2.data_ptr() == buf.data_ptr()      # the skip tensor was not copied
    assert R.same_bits(y1, y2)


# ---------------------------------------------------------------- 4. 1x1x1 convolution
@pytest.fixture(scope="module")
def conv_case():
    """4 -> 1 at B * V = 2 * 266,240 = 532,480 voxels: the forward's 2048-workgroup grid makes a second trip, the backward's
    1024-workgroup grid a second and a third."""
    g = gen(41)
    shape = (2, 4, 8, 128, 260)
    x, w, b = torch.randn(shape, generator=g), torch.randn(1, 4, 1, 1, 1, generator=g), torch.randn(1, generator=g)
    out = (2, 1, 8, 128, 260)
    return x, w, b, torch.randn(out, generator=g), torch.randn(out, generator=g), torch.randn(out, generator=g)


def conv_subsets(shape):
    """the voxels i = b * V + v >= 524,288 of a (B, C, V) tensor: the forward's second trip, the backward's third"""
    B, C = shape[:2]
    V = int(np.prod(shape[2:]))
    m = torch.zeros(B, C, V, dtype=torch.bool)
    for b in range(B):
        m[b, :, max(0, min(V, R.TRIP - b * V)):] = True
    return {"voxels beyond 524288": m.reshape(-1)}


def test_conv1x1_4to1_beyond_one_grid(conv_case):
    x, w, b, gy, _, _ = conv_case
    ref, r32 = R.conv1x1(x, w, b, gy, torch.float64), R.conv1x1(x, w, b, gy, torch.float32)
    xg, wg, bg = leaf(x), leaf(w), leaf(b)
    y = ops.conv3d(xg, wg, bg)
    (y * gy.cuda()).sum().backward()
    R.judge("conv1x1 4->1 y", y, ref[0], r32[0], 1e-6, conv_subsets(y.shape))
    R.judge("conv1x1 4->1 dx", xg.grad, ref[1], r32[1], 1e-6, conv_subsets(x.shape))
    scale = float(np.sqrt(gy.numel()))   # dw, db: cancelling sums of 532,480 products of N(0,1) values, met in float atomics
    R.judge_sum("conv1x1 4->1 dw", wg.grad, ref[2], r32[2], 1e-5, scale)
    R.judge_sum("conv1x1 4->1 db", bg.grad, ref[3], r32[3], 1e-5, scale)


@pytest.mark.parametrize("use", ["both", "dy", "dsum"])
def test_conv1x1_sum_beyond_one_grid(conv_case, use):
    x, w, b, gy, gs, addend = conv_case

    def model(dtype):
        xd, wd, bd, ad = (t.detach().to(dtype).requires_grad_(True) for t in (x, w, b, addend))
        y = F.conv3d(xd, wd, bd)
        s = y + ad
        loss = ((y * gy.to(dtype)).sum() if use != "dsum" else 0) + ((s * gs.to(dtype)).sum() if use != "dy" else 0)
        loss.backward()
        return y.detach(), s.detach(), xd.grad, wd.grad, bd.grad, ad.grad

    ref, r32 = model(torch.float64), model(torch.float32)
    xg, wg, bg, ag = leaf(x), leaf(w), leaf(b), leaf(addend)
    y, s = ops.conv3d_sum(xg, wg, bg, ag)
    loss = ((y * gy.cuda()).sum() if use != "dsum" else 0) + ((s * gs.cuda()).sum() if use != "dy" else 0)
    loss.backward()
    tag = f"conv1x1_sum [{use}]"
    R.judge(tag + " y", y, ref[0], r32[0], 1e-6, conv_subsets(y.shape))
    R.judge(tag + " sum", s, ref[1], r32[1], 1e-6, conv_subsets(y.shape))
    R.judge(tag + " dx", xg.grad, ref[2], r32[2], 1e-6, conv_subsets(x.shape))
    scale = float(np.sqrt(gy.numel())) * (np.sqrt(2.0) if use == "both" else 1.0)
    R.judge_sum(tag + " dw", wg.grad, ref[3], r32[3], 1e-5, scale)
    R.judge_sum(tag + " db", bg.grad, ref[4], r32[4], 1e-5, scale)
    if use == "dy":
        assert ag.grad is None or not bool(ag.grad.any())
    else:
        assert torch.equal(ag.grad.cpu(), gs)      # the addend's gradient is dsum itself


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("cin,cout", [(8, 8), (3, 5), (1, 1)])
def test_conv1x1_forward_other_channel_counts(cin, cout, bias):
    g = gen(42)
    B, dims = 2, (3, 5, 7)
    x, w = torch.randn(B, cin, *dims, generator=g), torch.randn(cout, cin, 1, 1, 1, generator=g)
    b = torch.randn(cout, generator=g) if bias else None
    y = torch.full((B, cout) + dims, NAN, device="cuda")
    call("hp_conv1x1_forward", x.cuda(), w.cuda(), b.cuda() if bias else None, y, B, cin, cout, int(np.prod(dims)))
    R.judge(f"conv1x1 {cin}->{cout} bias={bias} y", y, F.conv3d(x.double(), w.double(), b.double() if bias else None),
            F.conv3d(x, w, b), 1e-6)


# ---------------------------------------------------------------- 5. leaky / add
@pytest.fixture(scope="module")
def leaky_case():
    """n = 2,113,536: n / 4 = 528,384 float4 items > 524,288; exact zeros and pairs that cancel to zero among the inputs"""
    g = gen(51)
    shape = (2, 1, 8, 256, 516)
    a, b, gy = (torch.randn(shape, generator=g) for _ in range(3))
    fa, fb = a.view(-1), b.view(-1)
    fa[::7] = 0.0
    fb[::7] = 0.0
    fb[3::11] = -fa[3::11]
    fa[5::13] = 0.0
    assert a.numel() // 4 > R.TRIP and int(((a + b) == 0).sum()) > 100000
    return a, b, gy


@pytest.mark.parametrize("slope", [0.2, 1.0, 0.0])
@pytest.mark.parametrize("two", [True, False])
def test_leaky_add_beyond_one_grid_is_the_float32_expression(leaky_case, slope, two):
    a, b, gy = leaky_case
    sl = torch.tensor(slope, dtype=torch.float32)
    s = a + b if two else a
    y_ref = torch.where(s > 0, s, s * sl)
    g_ref = torch.where(y_ref > 0, gy, gy * sl)
    ag, bg = leaf(a), leaf(b)
    if slope == 1.0 and two:
        y = ops.add(ag, bg)
    else:
        y = ops.leaky_add(ag, bg if two else None, slope)
    (y * gy.cuda()).sum().backward()
    assert R.same_bits(y, y_ref)
    assert R.same_bits(ag.grad, g_ref)
    if two:
        assert R.same_bits(bg.grad, g_ref)


# ---------------------------------------------------------------- 6. normalize_feature
def test_normalize_feature_first_extremes_across_workgroups_and_trips():
    """nvol = 8, V = 65,835 = 5 x 7 x 1881 (odd: a live tail): 256 chunks per volume, so the scalar loops (min / max search, the
    backward's sums and apply) make a second trip over items 65,536 ... 65,834.  Each volume has its minimum at three indices
    and its maximum at two; the gradient goes to the first of each.  Even volumes: first occurrences in the first trip (later
    ones in the second); odd volumes: every occurrence in the second trip, the last maximum on the tail's last element."""
    g = gen(61)
    V = 5 * 7 * 1881
    x = torch.randn(2, 4, 5, 7, 1881, generator=g)
    f = x.view(8, V)
    assert float(f.min()) > -7.0 and float(f.max()) < 7.0
    for v in range(8):
        mins, maxs = ((100 + 300 * v, 30000, 65700), (5000 + 300 * v, 65800)) if v % 2 == 0 else ((65540, 65700, 65830), (65800, 65834))
        f[v, list(mins)] = -7.5 - v
        f[v, list(maxs)] = 9.25 + v
    gy = torch.randn(x.shape, generator=g)
    ref, r32 = R.normalize_feature(x, gy, torch.float64), R.normalize_feature(x, gy, torch.float32)
    xg = leaf(x)
    y = ops.normalize_feature(xg)
    (y * gy.cuda()).sum().backward()
    plain = torch.ones(8, V, dtype=torch.bool)      # everything but the planted extremes, whose gradients dwarf the others
    for v in range(8):
        plain[v, [100 + 300 * v, 30000, 65700, 5000 + 300 * v, 65800, 65540, 65830, 65834]] = False
    sub = {"tail": R.plane_tail(8, V), "second trip": R.plane_range(8, V, 256 * R.WG, V)}
    R.judge("normalize_feature y", y, ref[0], r32[0], 1e-6, sub)
    R.judge("normalize_feature dx", xg.grad, ref[1], r32[1], 1e-4, dict(sub, plain=plain.reshape(-1), extremes=~plain.reshape(-1)))
    # the routing itself: the reference's gradient at a later occurrence is the plain one, gy * 10 / (max - min)
    yc = y.detach().cpu().view(8, V)
    assert float(yc.min()) == 0.0 and abs(float(yc.max()) - 10.0) < 1e-5


def test_normalize_feature_constant_volume_is_exactly_zero():
    x = torch.full((1, 1, 4, 10, 25), 3.5).cuda()
    assert not bool(ops.normalize_feature(x).any())


# ---------------------------------------------------------------- 7. soft-argmax
# (9,31,37): V = 10,323, 323 logits per forward chunk (> 256 threads), 6 backward chunks; (41,41,41): V = 68,921 > 65,536, the
# backward's 32-chunk cap with a second trip
@pytest.mark.parametrize("kind", ["3 randn", "30 randn", "3 randn + 200"])
@pytest.mark.parametrize("shape", [(1, 3, 9, 31, 37), (1, 2, 41, 41, 41)])
def test_softargmax_chunk_loops(shape, kind):
    g = gen(71)
    B, J, D, H, W = shape
    V = D * H * W
    h = torch.randn(shape, generator=g) * (30.0 if kind == "30 randn" else 3.0) + (200.0 if kind.endswith("200") else 0.0)
    gy = torch.randn(B, 3 * J, generator=g)
    ref, r32 = R.softargmax(h, gy, torch.float64), R.softargmax(h, gy, torch.float32)
    hg = leaf(h)
    y = ops.softmax_integral(hg, J, W, H, D)
    (y * gy.cuda()).sum().backward()
    per = (V + R.SA_CHUNKS - 1) // R.SA_CHUNKS
    bchunks = max(1, min(32, (V + R.WG * 8 - 1) // (R.WG * 8)))
    sub = {"last forward chunk": R.plane_range(B * J, V, (R.SA_CHUNKS - 1) * per, V),
           "beyond the backward's first trip": R.plane_range(B * J, V, bchunks * R.WG, V)}
    R.judge(f"softargmax {shape} {kind} y", y, ref[0], r32[0], 1e-6)
    R.judge(f"softargmax {shape} {kind} dheat", hg.grad, ref[1], r32[1], 1e-5, sub)


# ---------------------------------------------------------------- 8. BCE + Dice
BCE_SHAPE = (5, 105013)   # n = 525,065 > 524,288


def bce_inputs(logits, targets):
    g = gen(81)
    x = torch.randn(BCE_SHAPE, generator=g) * 3
    pick = torch.rand(BCE_SHAPE, generator=g)
    if logits == "1% at +-100":
        x = torch.where(pick < 0.005, torch.full_like(x, 100.0), torch.where(pick > 0.995, torch.full_like(x, -100.0), x))
    t = {"5% ones": (torch.rand(BCE_SHAPE, generator=g) < 0.05).float(), "all zero": torch.zeros(BCE_SHAPE),
         "all one": torch.ones(BCE_SHAPE)}[targets]
    return x, t


@pytest.mark.parametrize("targets", ["5% ones", "all zero", "all one"])
@pytest.mark.parametrize("logits", ["3 randn", "1% at +-100"])
def test_bce_dice_beyond_one_grid_and_saturated_logits(logits, targets):
    x, t = bce_inputs(logits, targets)
    ref, r32 = R.bce_dice(x, t, 1.7, torch.float64), R.bce_dice(x, t, 1.7, torch.float32)
    xg = leaf(x)
    loss = ops.bce_dice(xg, t.cuda())
    (loss * 1.7).backward()
    tag = f"bce_dice [{logits}; {targets}]"
    R.judge(tag + " loss", loss, ref[0], r32[0], 1e-6)
    R.judge(tag + " dlogit", xg.grad, ref[1], r32[1], 1e-5, {"second trip": R.beyond_first_trip(x.numel())})


def test_bce_dice_global_batch_in_one_process_is_the_local_loss():
    """Same sums through hp_bce_dice_partial / _finalize; they meet in fp64 atomics, so their order moves the loss by rounding
    errors of 1e-16, far below one float32 ulp of the result: 1e-12 on the loss, and the gradients' float32 coefficients agree
    to one ulp (2^-23) at worst."""
    x, t = bce_inputs("1% at +-100", "5% ones")
    out = []
    for glob in (False, True):
        xg = leaf(x)
        loss = ops.bce_dice(xg, t.cuda(), global_batch=glob)
        (loss * 1.7).backward()
        out.append((loss.detach().double().item(), xg.grad.cpu()))
    assert abs(out[1][0] - out[0][0]) <= 1e-12 * abs(out[0][0])
    assert R.rel_l2(out[1][1], out[0][1]) <= 2.0 ** -23


# ---------------------------------------------------------------- 9. weighted MSE
@pytest.mark.parametrize("rows", [1, 5])   # n = 72: one pass of the single workgroup; n = 360: its strided loop
def test_weighted_mse_strided_loop_and_zero_weights(rows):
    from hiddenpose_amd.criterion import weighted_mse_loss

    g = gen(91)
    p, t = torch.rand(rows, 72, generator=g) * 60, torch.rand(rows, 72, generator=g) * 60
    w = (torch.rand(rows, 72, generator=g) > 0.2).float()
    ref, r32 = R.weighted_mse(p, t, w, 1.5, torch.float64), R.weighted_mse(p, t, w, 1.5, torch.float32)
    pg = leaf(p)
    loss = weighted_mse_loss(pg, t.cuda(), w.cuda(), True)
    (loss * 1.5).backward()
    R.judge(f"weighted_mse n={72 * rows} loss", loss, ref[0], r32[0], 1e-6)
    R.judge(f"weighted_mse n={72 * rows} dpred", pg.grad, ref[1], r32[1], 1e-6, {"beyond 256": R.beyond_first_trip(72 * rows, 1, R.WG)})
    pz = leaf(p)
    zero = weighted_mse_loss(pz, t.cuda(), torch.zeros_like(w).cuda(), True)
    zero.backward()
    assert zero.item() == 0.0 and not bool(pz.grad.any())


# ---------------------------------------------------------------- 10. depth top-4 / VisibleNet projection
def quantised(shape, g, negatives=False):
    levels = torch.tensor([0.0, 0.25, 0.5, 1.0] + ([-0.5] if negatives else []))
    return levels[torch.randint(0, len(levels), shape, generator=g)]


# HW = 35: one partial workgroup; planes = 3, HW = 175,003: 525,009 pixels, a second trip
@pytest.mark.parametrize("planes,D,HW", [(2, 4, 35), (2, 5, 35), (2, 37, 35), (3, 4, 175003)])
def test_depth_top4_ties_go_to_the_smaller_depth_index(planes, D, HW):
    x = quantised((planes, D, HW), gen(101))
    vals = torch.full((planes, 4, HW), NAN, device="cuda")
    dep = torch.full((planes, 4, HW), NAN, device="cuda")
    call("hp_depth_top4", x.cuda(), vals, dep, planes, D, HW)
    v_ref, d_ref, _ = R.depth_top4(x.numpy())
    assert float((np.diff(np.sort(x.numpy(), axis=1), axis=1) == 0).mean()) > 0.3     # ties everywhere
    assert R.same_bits(vals, torch.from_numpy(v_ref))
    assert R.same_bits(dep, torch.from_numpy(d_ref))


def test_visible_projection_on_tied_values():
    g = gen(102)
    B, C, D, H, W = 2, 3, 5, 4, 7      # the ReLU in front runs 16-byte accesses: a multiple of four elements
    x = quantised((B, C, D, H, W), g, negatives=True)
    y = ops.visible_projection(x.cuda()).cpu()
    r = np.maximum(x.numpy(), np.float32(0)).reshape(B * C, -1)
    mn, mx = r.min(1, keepdims=True), r.max(1, keepdims=True)
    inv = np.float32(1.0) / ((mx - mn) + np.float32(1e-15))
    nrm = ((r - mn) * inv * np.float32(1.0e5)).astype(np.float32).reshape(B * C, D, H * W)
    v_ref, d_ref, _ = R.depth_top4(nrm)
    assert R.same_bits(y[:, :C].contiguous(), torch.from_numpy(v_ref).reshape(B, C, 4, H, W))
    assert R.same_bits(y[:, C:].contiguous(), torch.from_numpy(d_ref).reshape(B, C, 4, H, W))


# ---------------------------------------------------------------- 11. noise augmentation
@pytest.mark.parametrize("n", [100, 23101])   # sigma = 80: radius 320 > 256 threads; n = 100 < radius: both borders in every window
def test_noise_blur_with_a_radius_beyond_one_workgroup(n):
    g = gen(111)
    meas = torch.rand(n, generator=g) * 3.0
    taps, r = ops.gaussian_taps(80.0)
    assert r == 320
    blur = ops.add_noise(meas.cuda(), 80.0, seed=1, poisson=False)
    ref = O.blur_flat_replicate(meas.numpy(), 80.0)
    border = torch.cat([torch.arange(0, min(r, n)), torch.arange(max(n - r, 0), n)]).unique()
    R.judge(f"noise blur sigma 80 n={n}", blur, ref, R.blur32(meas.numpy(), taps, r), 1e-6, {"borders": border})


def test_poisson_draws_around_the_change_of_method():
    """lambda <= 0 draws exactly 0; 1e-3, 11.99 (multiplication method) and 12.0 (transformed rejection): the mean of N draws
    within 6 sigma = 6 sqrt(lambda / N), the variance at the two large means within 3 % (its own sigma is 0.33 %)."""
    N = 200000
    lams = (0.0, -1.0, 1e-3, 11.99, 12.0)
    lam = torch.cat([torch.full((N,), v) for v in lams]).cuda()
    one = torch.ones(1, device="cuda")
    y = torch.full_like(lam, NAN)
    call("hp_noise_blur_poisson", lam, y, lam.numel(), one, 0, 1, 4321)
    y = y.cpu()
    assert torch.equal(y, y.round()) and float(y.min()) >= 0
    for k, m in enumerate(lams):
        s = y[k * N:(k + 1) * N].double()
        print(f"[stage-edge] poisson lambda={m}: mean {s.mean().item():.5f}  var {s.var().item():.5f}")
        if m <= 0:
            assert not bool(s.any())
            continue
        assert abs(s.mean().item() - m) <= 6 * np.sqrt(m / N), (m, s.mean().item())
        if m > 1:
            assert abs(s.var().item() / m - 1) < 0.03, (m, s.var().item())


# ---------------------------------------------------------------- 12. channel slice copy
@pytest.mark.parametrize("V", [8, 4 * 87382])   # 2 * 3 * 87,382 = 524,292 float4 items: four beyond one grid
def test_channel_slice_copy_scatter_then_gather(V):
    g = gen(121)
    B, C, Ctot, c_off = 2, 3, 7, 2
    src = torch.randn(B, C, V, generator=g)
    big = torch.full((B, Ctot, V), -777.25, device="cuda")
    call("hp_channel_slice_copy", src.cuda(), big, B, C, V, Ctot, c_off, 0)
    out = big.cpu()
    assert R.same_bits(out[:, c_off:c_off + C].contiguous(), src)
    assert bool((out[:, :c_off] == -777.25).all()) and bool((out[:, c_off + C:] == -777.25).all())
    back = torch.full((B, C, V), NAN, device="cuda")
    call("hp_channel_slice_copy", big, back, B, C, V, Ctot, c_off, 1)
    assert R.same_bits(back, src)
    assert R.same_bits(big, out)     # gather left the big buffer alone
