"""dim_head 64, the width the three transformer heads' constructors default to (csrc/sformer_kernels.hip k_attention64 /
k_attention_patch_h16_64, csrc/sformer_backward.hip k_attn_bwd_*64): the oracle pinned to the reference at that width (CPU,
tests/golden/head64.npz from make_head64_goldens.py), the attention entries alone against float64, and the modules against
the reference goldens and the oracle (GPU).  Every bar is the one the existing widths are held to (test_sformer.py,
test_sformer_train.py, test_xformers_train.py); the module-level half is in test_head64_modules.py."""
import numpy as np
import pytest
import torch

from hiddenpose_amd import _lib
from hiddenpose_amd import _xformer_autograd as xa
from hiddenpose_amd import testing as hpt
from oracle import nlospose_oracle as O
from test_sformer_train import _attn_ref
from util import rel_l2

HP_ERR_UNSUPPORTED = -2   # include/hiddenpose_hip.h

SF = dict(dim=96, num_frames=3, num_joints=24, image_size=32, patch_size=4, channels=1, depth=2, heads=2, dim_head=64, out_dim=128)
TS = {
    "plain": dict(dim=64, num_frames=4, num_classes=10, image_size=32, patch_size=8, channels=1, depth=2, heads=2, dim_head=64),
    "shift": dict(dim=64, num_frames=4, num_classes=10, image_size=32, patch_size=8, channels=1, depth=2, heads=2, dim_head=64,
                  shift_tokens=True),
}
TP = {  # tests/test_xformers.py's "learnable" case at dim 128, 2 heads (dim // heads = 64)
    "learnable": dict(feature_size=[16, 24], patch_size=[4, 4], num_keypoints=5, dim=128, depth=1, heads=2, mlp_dim=128,
                      heatmap_dim=48, heatmap_size=[8, 6], channels=3, pos_embedding_type="learnable", hidden_heatmap_dim=64),
}
CASES = {"sf": ("sf", SF), "ts_plain": ("ts", TS["plain"]), "ts_shift": ("ts", TS["shift"]), "tp_learnable": ("tp", TP["learnable"])}


def build(key):
    """The module of case `key` with the generators' weight fill, and its input (CPU)."""
    kind, kw = CASES[key]
    if kind == "sf":
        from hiddenpose_amd.NlosPoseSformer import NlosPoseSformer

        m = NlosPoseSformer(**kw)
        hpt.fill_module(m, "sformer.")
        x = torch.rand(2, kw["num_frames"], kw["channels"], kw["image_size"], kw["image_size"], generator=torch.Generator().manual_seed(77))
    elif kind == "ts":
        from hiddenpose_amd.transformer import TimeSformer

        m = TimeSformer(**kw)
        hpt.fill_module(m, "timesformer.")
        with torch.no_grad():
            m.cls_token.copy_(hpt.fill_value("timesformer.cls_token", m.cls_token.shape))
        x = torch.rand(2, kw["num_frames"], kw["channels"], kw["image_size"], kw["image_size"], generator=torch.Generator().manual_seed(78))
    else:
        from hiddenpose_amd.tokenpose import TokenPose_L_base

        m = TokenPose_L_base(**kw)
        hpt.fill_module(m, "tokenpose.")
        x = torch.rand(2, kw["channels"], kw["feature_size"][0], kw["feature_size"][1], generator=torch.Generator().manual_seed(79))
    return kind, kw, m, x


def loss_weights(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(78), dtype=torch.float64)


def oracle_forward(kind, kw, x, sd):
    if kind == "sf":
        return O.nlospose_sformer(x, {"sformer." + k: t for k, t in sd.items()}, patch_size=kw["patch_size"], heads=kw["heads"])
    if kind == "ts":
        return O.timesformer(x, sd, patch_size=kw["patch_size"], heads=kw["heads"], shift_tokens=kw.get("shift_tokens", False))
    return O.tokenpose_base(x, sd, patch_size=kw["patch_size"][0], heads=kw["heads"], num_keypoints=kw["num_keypoints"],
                            heatmap_size=kw["heatmap_size"], pos_embedding_type=kw["pos_embedding_type"])


def oracle_grads(kind, kw, m, x, device="cpu", R=None):
    """float64 autograd of the oracle: ({parameter name: grad or None}, input grad, output).  A parameter the module keeps
    frozen (requires_grad False) stays frozen."""
    names = dict(m.named_parameters())
    sd = {k: v.detach().to(device, torch.float64).requires_grad_(k in names and names[k].requires_grad) for k, v in m.state_dict().items()}
    xd = x.detach().to(device, torch.float64).requires_grad_(True)
    with torch.device(device):   # the oracle's rotary tables are built with factory calls
        y = oracle_forward(kind, kw, xd, sd)
    R = loss_weights(y.shape) if R is None else R
    (y * R.to(device)).sum().backward()
    return {k: sd[k].grad for k in names}, xd.grad, y.detach()


def golden_compare(g, key, grads, xgrad, tol):
    worst = rel_l2(xgrad, g[f"{key}_input"])
    assert worst < tol, ("input", worst)
    for k, gr in grads.items():
        if gr is None:
            continue
        gr = gr.detach().cpu().double()
        if f"{key}/{k}" in g:
            e = rel_l2(gr, g[f"{key}/{k}"])
        else:
            idx = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).choice(gr.numel(), size=min(64, gr.numel()),
                                                                                  replace=False).astype(np.int64))
            ref_l2 = float(g[f"{key}/{k}/l2"])
            e = max(abs(float(gr.norm()) - ref_l2) / ref_l2, rel_l2(gr.reshape(-1)[idx], g[f"{key}/{k}/val"]))
        worst = max(worst, e)
        assert e < tol, (k, e)
    return worst


# ----------------------------------------------------------------------------------------------------------------- CPU

@pytest.mark.parametrize("key", list(CASES))
def test_oracle_matches_reference_at_dim_head_64(key, golden):
    kind, kw, m, x = build(key)
    grads, xgrad, y = oracle_grads(kind, kw, m, x)
    g = golden("head64.npz")
    e = rel_l2(y, g[f"{key}_y"])
    worst = golden_compare(g, key, grads, xgrad, 1e-6)
    print(f"{key}: forward rel-L2 {e:.2e}, worst gradient rel-L2 {worst:.2e}")
    assert e < 1e-6
    assert sorted(k for k, v in grads.items() if v is None) == sorted(g[f"{key}_none"].tolist())


# ----------------------------------------------------------------------------------------------------------------- GPU

# B, heads, nj, n, frames: nj 0 / 1 / 24 / 32; n 3 / 17 (below one 32-key tile), 64, 300 and 1024 (ragged, above one 128-query
# block); one frame and many; 16 x 300 and 2 x 1024 tokens give the joint queries 32 and 16 key splits
LAYOUTS = [(1, 2, 24, 64, 2), (2, 2, 0, 300, 1), (1, 2, 1, 17, 5), (2, 3, 24, 3, 7), (1, 2, 24, 300, 16), (1, 4, 24, 1024, 2),
           (1, 2, 0, 17, 1), (2, 2, 32, 33, 2), (1, 1, 1, 64, 1)]
DH = 64


def _ids(c):
    return "B%d_h%d_nj%d_n%d_f%d" % c


def _inputs(layout, dh=DH, seed=11):
    B, heads, nj, n, f = layout
    ntok = nj + f * n
    g = torch.Generator().manual_seed(seed)
    Q, K, K0, V = (torch.randn(B, heads, ntok, dh, generator=g) * (dh ** -0.25) for _ in range(4))
    K[:, :, :nj] = K0[:, :, :nj]   # the joint rows of K carry no RoPE
    dO = torch.randn(B, ntok, heads * dh, generator=g)
    return Q, K, K0, V, dO


def _forward(L, q, k, k0, v, layout, dh, out, lse=None, prec=0, ws=None):
    B, heads, nj, n, f = layout
    ntok = nj + f * n
    st = _lib.current_stream_handle(q.device)
    if ws is None:
        ws = torch.empty(int(L.hp_sformer_attention_workspace_bytes(B, heads, dh)) // 4 + 1, device=q.device)
    if lse is not None:
        _lib.check(L.hp_sformer_attention_lse(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), lse.data_ptr(), B,
                                              heads, dh, ntok, nj, n, f, ws.data_ptr(), st), "hp_sformer_attention_lse")
    else:
        _lib.check(L.hp_sformer_attention(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), B, heads, dh, ntok, nj,
                                          n, f, prec, ws.data_ptr(), st), "hp_sformer_attention")


def _backward(L, q, k, k0, v, out, do, lse, layout, dh, grads, ws=None):
    B, heads, nj, n, f = layout
    ntok = nj + f * n
    nb = L.hp_sformer_attention_backward_workspace_bytes(B, heads, dh, ntok, nj, f)
    if ws is None:
        ws = torch.empty(int(nb) // 4 + 1, device=q.device)
    dq, dk, dk0, dv = grads
    _lib.check(L.hp_sformer_attention_backward(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), do.data_ptr(),
                                               lse.data_ptr(), dq.data_ptr(), dk.data_ptr(), dk0.data_ptr(), dv.data_ptr(), B, heads, dh,
                                               ntok, nj, n, f, ws.data_ptr(), nb, _lib.current_stream_handle(q.device)),
               "hp_sformer_attention_backward")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_attention_forward_vs_float64(layout):
    """hp_sformer_attention_lse / hp_sformer_attention at dh 64: fp32 `out` over all rows < 1e-5 and lse < 1e-6 (the bars of
    test_attention_backward_vs_float64); on the patch rows fp32 < 2e-6, bf16 < 1e-2, fp16 < 1.5e-3 (the bars of
    test_16bit_patch_attention_op_vs_float64; the inputs scale as dh^-0.25, so the scores keep unit variance)."""
    B, heads, nj, n, f = layout
    L = _lib.lib()
    dev = torch.device("cuda")
    ntok = nj + f * n
    Q, K, K0, V, _ = _inputs(layout)
    q, k, k0, v = (t.to(dev).contiguous() for t in (Q, K, K0, V))
    out = torch.empty(B, ntok, heads * DH, device=dev)
    lse = torch.empty(B, heads, ntok, device=dev)
    _forward(L, q, k, k0, v, layout, DH, out, lse)
    ref, ref_lse = _attn_ref(*(t.to(dev, torch.float64) for t in (Q, K, K0, V)), nj, n, f)
    ref = ref.permute(0, 2, 1, 3).reshape(B, ntok, -1)
    e_all, e_lse = rel_l2(out, ref), rel_l2(lse, ref_lse)
    errs = {}
    for name, prec in (("fp32", 0), ("bf16", 1), ("fp16", 4)):
        o = torch.zeros(B, ntok, heads * DH, device=dev)
        _forward(L, q, k, k0, v, layout, DH, o, None, prec)
        if prec == 0:
            assert torch.equal(o, out)   # the lse entry's `out` is the plain entry's
        else:
            assert torch.equal(o[:, :nj], out[:, :nj])   # joint-token queries stay fp32
        errs[name] = rel_l2(o[:, nj:], ref[:, nj:])
    print(layout, f"out {e_all:.2e} lse {e_lse:.2e} patch rows", {k2: f"{v2:.2e}" for k2, v2 in errs.items()})
    assert e_all < 1e-5 and e_lse < 1e-6
    assert errs["fp32"] < 2e-6 and errs["bf16"] < 1e-2 and errs["fp16"] < 1.5e-3


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_attention_backward_vs_float64(layout):
    """hp_sformer_attention_backward at dh 64 against float64 autograd: dQ, dK, dK0, dV each < 1e-5; dK0 exactly zero without
    joint tokens; two calls bitwise equal."""
    B, heads, nj, n, f = layout
    L = _lib.lib()
    dev = torch.device("cuda")
    ntok = nj + f * n
    Q, K, K0, V, dO = _inputs(layout)
    q, k, k0, v, do = (t.to(dev).contiguous() for t in (Q, K, K0, V, dO))
    out = torch.empty(B, ntok, heads * DH, device=dev)
    lse = torch.empty(B, heads, ntok, device=dev)
    _forward(L, q, k, k0, v, layout, DH, out, lse)
    r1 = xa.attention_backward(q, k, k0, v, out, do, lse, B, heads, DH, ntok, nj, n, f)
    r2 = xa.attention_backward(q, k, k0, v, out, do, lse, B, heads, DH, ntok, nj, n, f)
    torch.cuda.synchronize()
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)
    Qd, Kd, K0d, Vd = (t.to(dev, torch.float64).requires_grad_(True) for t in (Q, K, K0, V))
    ref, _ = _attn_ref(Qd, Kd, K0d, Vd, nj, n, f)
    (ref * dO.to(dev, torch.float64).view(B, ntok, heads, DH).permute(0, 2, 1, 3)).sum().backward()
    errs = [rel_l2(a, t.grad) for a, t in zip(r1, (Qd, Kd, K0d, Vd)) if t.grad is not None]
    print(layout, "dQ dK dK0 dV", ["%.2e" % e for e in errs])
    assert max(errs) < 1e-5
    if nj == 0:
        assert float(r1[2].abs().max()) == 0.0


GUARD = 64 * 1024                                  # floats either side (256 KB)
SENT = float.fromhex("0x1.5a5a5ap+100")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [(2, 3, 24, 37, 3), (1, 2, 7, 300, 2)], ids=_ids)
def test_attention_kernels_write_only_their_outputs(layout):
    """`out`, `lse`, dQ, dK, dK0, dV of the dh-64 calls sit between two sentinel-filled guard regions (the pattern of
    test_linear_and_geglu_epilogues_write_only_their_output): the guards stay bit for bit, every output element is written."""
    B, heads, nj, n, f = layout
    L = _lib.lib()
    dev = torch.device("cuda")
    ntok = nj + f * n
    Q, K, K0, V, dO = _inputs(layout, seed=13)
    q, k, k0, v, do = (t.to(dev).contiguous() for t in (Q, K, K0, V, dO))

    def guarded(shape):
        cnt = int(np.prod(shape))
        buf = torch.full((GUARD + cnt + GUARD,), SENT, device=dev)
        return buf, buf[GUARD:GUARD + cnt].view(shape)

    def intact(buf, t):
        return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + t.numel():] == SENT).all())

    names = ["out", "lse", "dQ", "dK", "dK0", "dV"]
    shapes = [(B, ntok, heads * DH), (B, heads, ntok)] + [(B, heads, ntok, DH)] * 4
    bufs = [guarded(s) for s in shapes]
    out, lse = bufs[0][1], bufs[1][1]
    _forward(L, q, k, k0, v, layout, DH, out, lse)
    _backward(L, q, k, k0, v, out, do, lse, layout, DH, [b[1] for b in bufs[2:]])
    torch.cuda.synchronize()
    for name, (buf, t) in zip(names, bufs):
        assert intact(buf, t), f"{name} was written outside its tensor"
        assert not bool((t == SENT).any()), f"{name} has unwritten elements"
    for prec in (0, 1, 4):
        buf, o = guarded(shapes[0])
        _forward(L, q, k, k0, v, layout, DH, o, None, prec)
        torch.cuda.synchronize()
        assert intact(buf, o) and not bool((o == SENT).any()), prec
    ref, ref_lse = _attn_ref(*(t.to(dev, torch.float64) for t in (Q, K, K0, V)), nj, n, f)
    assert rel_l2(out, ref.permute(0, 2, 1, 3).reshape(B, ntok, -1)) < 1e-5 and rel_l2(lse, ref_lse) < 1e-6


@pytest.mark.gpu
def test_widths_alternate_on_one_stream_without_leaking_state():
    """Forward and backward at dh 32 and dh 64 alternately on one stream with ONE forward and ONE backward workspace, sized for
    the larger width: the dh-32 results equal those of a run without the dh-64 calls, bit for bit (and the dh-64 ones theirs)."""
    L = _lib.lib()
    dev = torch.device("cuda")
    layout = (2, 2, 24, 150, 3)
    B, heads, nj, n, f = layout
    ntok = nj + f * n
    ws_f = torch.empty(max(int(L.hp_sformer_attention_workspace_bytes(B, heads, d)) for d in (32, 64)) // 4 + 1, device=dev)
    ws_b = torch.empty(max(int(L.hp_sformer_attention_backward_workspace_bytes(B, heads, d, ntok, nj, f)) for d in (32, 64)) // 4 + 1,
                       device=dev)

    def run(dh, shared):
        q, k, k0, v, do = (t.to(dev).contiguous() for t in _inputs(layout, dh, seed=17))
        res = [torch.empty(B, ntok, heads * dh, device=dev), torch.empty(B, heads, ntok, device=dev)] + [torch.empty_like(q) for _ in range(4)]
        _forward(L, q, k, k0, v, layout, dh, res[0], res[1], ws=ws_f if shared else None)
        _backward(L, q, k, k0, v, res[0], do, res[1], layout, dh, res[2:], ws=ws_b if shared else None)
        return res

    alone = {dh: run(dh, False) for dh in (32, 64)}
    torch.cuda.synchronize()
    for rnd in range(2):
        for dh in (32, 64, 32):
            got = run(dh, True)
            for a, b in zip(got, alone[dh]):
                assert torch.equal(a, b), (rnd, dh)


@pytest.mark.gpu
def test_qkv_prepare_and_its_backward_at_dim_head_64_vs_float64():
    """hp_sformer_qkv_prepare / _backward take any dh; at 64 the axial table is 64 wide (rot_dim = dh)."""
    from hiddenpose_amd.NlosPoseSformer import NlosPoseSformer

    dev = torch.device("cuda")
    L = _lib.lib()
    st = _lib.current_stream_handle(dev)
    g = torch.Generator().manual_seed(4)
    B, heads, dh, nj, hp, wp, f = 2, 3, 64, 24, 4, 5, 2
    n = hp * wp
    ntok = nj + f * n
    m = NlosPoseSformer(dim=64, num_frames=f, dim_head=dh, heads=heads)
    sin_t, cos_t = m.image_rot_emb.tables(hp, wp, dev)
    rd = sin_t.shape[-1]
    assert rd == 64
    qkv = torch.randn(B, ntok, 3 * heads * dh, generator=g)
    grads = [torch.randn(B, heads, ntok, dh, generator=g) for _ in range(4)]
    qkvc = qkv.to(dev)
    outs = [torch.empty(B, heads, ntok, dh, device=dev) for _ in range(4)]
    _lib.check(L.hp_sformer_qkv_prepare(qkvc.data_ptr(), *(t.data_ptr() for t in outs), B, ntok, heads, dh, nj, n, dh ** -0.5,
                                        sin_t.data_ptr(), cos_t.data_ptr(), rd, st), "prep")
    dqkv = torch.empty(B, ntok, 3 * heads * dh, device=dev)
    gd = [t.to(dev) for t in grads]
    _lib.check(L.hp_sformer_qkv_prepare_backward(gd[0].data_ptr(), gd[1].data_ptr(), gd[2].data_ptr(), gd[3].data_ptr(), dqkv.data_ptr(), B,
                                                 ntok, heads, dh, nj, n, dh ** -0.5, sin_t.data_ptr(), cos_t.data_ptr(), rd, st), "prep_bwd")
    qd = qkv.double().requires_grad_(True)
    q, k, v = (t.reshape(B, ntok, heads, dh).permute(0, 2, 1, 3) for t in qd.chunk(3, -1))
    q = q * dh ** -0.5
    sn, cs = sin_t.cpu().double(), cos_t.cpu().double()
    rot = lambda t: torch.cat((t[..., :rd] * cs + O._rotate_every_two(t[..., :rd]) * sn, t[..., rd:]), -1)
    Qr = torch.cat((q[:, :, :nj], rot(q[:, :, nj:].reshape(B, heads, f, n, dh)).reshape(B, heads, f * n, dh)), 2)
    Kr = torch.cat((k[:, :, :nj], rot(k[:, :, nj:].reshape(B, heads, f, n, dh)).reshape(B, heads, f * n, dh)), 2)
    fw = [rel_l2(a, b.detach()) for a, b in zip(outs, (Qr, Kr, k, v))]
    sum(((a * b.double()).sum() for a, b in zip((Qr, Kr, k, v), grads))).backward()
    eb = rel_l2(dqkv, qd.grad)
    print("qkv_prepare at dh 64: Q K K0 V", ["%.2e" % e for e in fw], f"backward {eb:.2e}")
    assert max(fw) < 1e-6 and eb < 1e-6


@pytest.mark.gpu
def test_other_widths_stay_refused_and_name_the_built_set():
    L = _lib.lib()
    dev = torch.device("cuda")
    buf = torch.zeros(1 << 16, device=dev)
    p = buf.data_ptr()
    st = _lib.current_stream_handle(dev)
    for dh in (8, 48, 128):
        n, nj, f = 16, 1, 4
        ntok = nj + f * n
        rcs = [L.hp_sformer_attention(p, p, p, p, p, 1, 1, dh, ntok, nj, n, f, 0, p, st),
               L.hp_sformer_attention_lse(p, p, p, p, p, p, 1, 1, dh, ntok, nj, n, f, p, st)]
        msgs = [L.hp_last_error_string()]
        nb = L.hp_sformer_attention_backward_workspace_bytes(1, 1, dh, ntok, nj, f)
        rcs.append(L.hp_sformer_attention_backward(p, p, p, p, p, p, p, p, p, p, p, 1, 1, dh, ntok, nj, n, f, p, nb, st))
        msgs.append(L.hp_last_error_string())
        assert rcs == [HP_ERR_UNSUPPORTED] * 3, (dh, rcs)
        for msg in msgs:
            assert b"not built (16, 24, 32, 64)" in msg, msg
