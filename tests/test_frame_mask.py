"""Frame masks for TimeSformer (models/transformer.py:208-253; hiddenpose_amd/transformer.py forward(video, mask),
csrc/sformer_masked.hip): the golden file and the argument checks of the masked C entries (CPU); the masked attention
entries against float64, against their unmasked counterparts (all-true mask: equal bits) and against each other (grouped
== generic), their guard regions, the module against goldens captured from the reference run with a mask, and the
properties the mask must have (GPU).  Bars are those the neighbouring tests use for the same quantities:
tests/test_sformer_train.py (out 1e-5, lse 1e-6, attention gradients 1e-5), tests/test_xformers.py / test_xformers_train.py
(module output and gradients against the reference goldens 1e-4)."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from hiddenpose_amd import _lib
from hiddenpose_amd import _xformer_autograd as xa
from hiddenpose_amd import testing as hpt
from test_xformers_train import golden_compare, loss_weights
from util import rel_l2

HP_ERR_BAD_ARG, HP_ERR_UNSUPPORTED = -1, -2   # include/hiddenpose_hip.h
KEYS = ("plain6", "scatter", "dh64", "shift")


def _module(g, key):
    """The golden config's module, weights and video (tests/test_xformers.py `_ts`), and its (2, f) bool mask."""
    from hiddenpose_amd.transformer import TimeSformer

    kw = json.loads(str(g[f"{key}_cfg"]))
    m = TimeSformer(**kw)
    hpt.fill_module(m, "timesformer.")
    with torch.no_grad():
        m.cls_token.copy_(hpt.fill_value("timesformer.cls_token", m.cls_token.shape))
    video = torch.rand(2, kw["num_frames"], kw["channels"], kw["image_size"], kw["image_size"],
                       generator=torch.Generator().manual_seed(78))
    return kw, m, video, torch.from_numpy(g[f"{key}_mask"])


# ----------------------------------------------------------------------------------------------------------------- CPU

def test_golden_file_has_the_declared_keys(golden):
    g = golden("frame_mask.npz")
    masks = {"plain6": ("111100", "111111"), "scatter": ("101101", "011111"), "dh64": ("11100", "10011"), "shift": ("11110", "11011")}
    for key in KEYS:
        kw, m, video, mask = _module(g, key)
        assert mask.dtype == torch.bool and mask.shape == (2, kw["num_frames"])
        assert ["".join("1" if v else "0" for v in row) for row in mask.tolist()] == list(masks[key])
        assert g[f"{key}_y"].shape == (2, 72) and g[f"{key}_y"].dtype == np.float64
        assert g[f"{key}_input"].shape == tuple(video.shape)
        assert g[f"{key}_none"].tolist() == []
        for k, p in m.named_parameters():
            if p.numel() <= 4096:
                assert g[f"{key}/{k}"].shape == tuple(p.shape), k
            else:
                assert g[f"{key}/{k}/l2"].shape == () and g[f"{key}/{k}/val"].shape == (64,), k
    assert json.loads(str(g["plain6_cfg"])) == json.loads(str(g["scatter_cfg"]))
    assert json.loads(str(g["dh64_cfg"]))["dim_head"] == 64 and json.loads(str(g["shift_cfg"]))["shift_tokens"] is True
    # a prefix mask equals truncation: the property the GPU test relies on, in the reference itself
    d = float(np.abs(g["plain6_y"][0] - g["plain6_y_trunc4"][0]).max())
    print(f"reference: |y[0] (mask 111100) - y (first 4 frames, no mask)| max {d:.2e}")
    assert d < 1e-12
    # the masked frames' input gradient is exactly zero in the reference (shift_tokens False)
    for key in ("plain6", "scatter", "dh64"):
        gi, mask = g[f"{key}_input"], g[f"{key}_mask"]
        assert float(np.abs(gi[~mask]).max()) == 0.0
        assert all(float(np.abs(gi[b, j]).max()) > 0 for b in range(2) for j in range(mask.shape[1]) if mask[b, j])


def _host_call(L, name, dh, nj, n, groups, key_mask=True, B=1, heads=2):
    """One masked entry on HOST buffers that are never dereferenced: every check below fails before the first device call."""
    ntok = nj + n * groups
    buf = (C.c_float * 16)()
    p = C.addressof(buf)
    km = p if key_mask else None
    if name == "hp_sformer_attention_masked":
        return L.hp_sformer_attention_masked(p, p, p, p, p, B, heads, dh, ntok, nj, n, groups, km, 1, p, None)
    if name == "hp_sformer_attention_lse_masked":
        return L.hp_sformer_attention_lse_masked(p, p, p, p, p, p, B, heads, dh, ntok, nj, n, groups, km, 1, p, None)
    nb = getattr(L, name + "_workspace_bytes")(B, heads, dh, ntok, nj, groups)
    return getattr(L, name)(p, p, p, p, p, p, p, p, p, p, p, B, heads, dh, ntok, nj, n, groups, km, 1, p, nb, None)


ENTRIES = ["hp_sformer_attention_masked", "hp_sformer_attention_lse_masked", "hp_sformer_attention_backward_masked",
           "hp_sformer_attention_backward_grouped_masked"]


@pytest.mark.parametrize("name", ENTRIES)
def test_masked_entries_check_their_arguments_without_a_device(name):
    L = _lib.lib()
    err = lambda: L.hp_last_error_string().decode()   # noqa: E731
    assert _host_call(L, name, 32, 1, 8, 4, key_mask=False) == HP_ERR_BAD_ARG
    assert "key_mask" in err() and name in err()
    assert _host_call(L, name, 32, 0, 8, 4) == HP_ERR_UNSUPPORTED
    assert "num_joints 0" in err() and name in err()
    assert _host_call(L, name, 20, 1, 8, 4) == HP_ERR_UNSUPPORTED
    assert "dim_head 20 not built" in err() and name in err()
    if name.endswith("grouped_masked"):
        assert _host_call(L, name, 64, 1, 8, 4) == HP_ERR_UNSUPPORTED
        assert "dim_head 64 not built (16, 24, 32)" in err()
        assert _host_call(L, name, 32, 1, 65, 4) == HP_ERR_UNSUPPORTED and "tokens per group" in err()
    assert _host_call(L, name, 32, 33, 8, 4) == HP_ERR_BAD_ARG      # num_joints > 32


def test_masked_workspace_sizes_answer_without_a_device():
    L = _lib.lib()
    for (B, heads, dh, ntok, nj, groups) in [(2, 4, 16, 1 + 6 * 16, 1, 16), (4, 8, 64, 1 + 8 * 64, 1, 64), (1, 2, 32, 24 + 3 * 50, 24, 50)]:
        ref = L.hp_sformer_attention_backward_workspace_bytes(B, heads, dh, ntok, nj, groups)
        assert ref > 0
        assert L.hp_sformer_attention_backward_masked_workspace_bytes(B, heads, dh, ntok, nj, groups) == ref
        assert L.hp_sformer_attention_backward_grouped_masked_workspace_bytes(B, heads, dh, ntok, nj, groups) == \
            L.hp_sformer_attention_backward_grouped_workspace_bytes(B, heads, dh, ntok, nj, groups)


# ----------------------------------------------------------------------------------------------------------------- GPU

def _masked_attn_ref(Q, K, K0, V, nj, n, f, km, mask_patch_queries):
    """tests/test_sformer_train.py `_attn_ref` extended by the reference's rule (models/transformer.py:110-141):
    sim.masked_fill_(~mask, -finfo.max) on the joint queries always and on the patch queries when mask_patch_queries; lse
    from the same masked scores.  km (B, ntok) bool; the joint tokens count as True whatever km says."""
    B, h, ntok, dh = Q.shape
    neg = -torch.finfo(Q.dtype).max
    km = km.clone()
    km[:, :nj] = True
    s = Q[:, :, :nj] @ K0.transpose(-1, -2)
    s = s.masked_fill(~km[:, None, None, :], neg)
    outs, lses = [torch.softmax(s, -1) @ V], [torch.logsumexp(s, -1)]
    pq = Q[:, :, nj:].reshape(B, h, f, n, dh)
    pk = K[:, :, nj:].reshape(B, h, f, n, dh)
    pv = V[:, :, nj:].reshape(B, h, f, n, dh)
    kk = torch.cat((K[:, :, None, :nj].expand(-1, -1, f, -1, -1), pk), 3)
    vv = torch.cat((V[:, :, None, :nj].expand(-1, -1, f, -1, -1), pv), 3)
    s = pq @ kk.transpose(-1, -2)
    if mask_patch_queries:
        kg = torch.cat((km[:, None, :nj].expand(-1, f, -1), km[:, nj:].reshape(B, f, n)), 2)   # (B, f, nj + n)
        s = s.masked_fill(~kg[:, None, :, None, :], neg)
    outs.append((torch.softmax(s, -1) @ vv).reshape(B, h, f * n, dh))
    lses.append(torch.logsumexp(s, -1).reshape(B, h, f * n))
    return torch.cat(outs, 2), torch.cat(lses, 2)


LAYOUTS = [  # B, heads, dh, nj, n, groups: dh 16 / 24 / 32 / 64, nj 1 and 24, n below, at and off multiples of 32, 2 .. 300 groups
    (1, 2, 16, 1, 16, 37), (2, 1, 24, 1, 2, 300), (1, 2, 32, 24, 3, 50), (2, 2, 32, 1, 17, 29), (1, 2, 24, 24, 64, 5),
    (2, 2, 32, 1, 32, 6), (1, 2, 16, 24, 33, 4), (1, 2, 32, 1, 200, 2), (1, 2, 64, 1, 5, 49), (1, 2, 64, 24, 100, 3),
    (1, 1, 64, 1, 64, 2), (2, 2, 24, 1, 100, 3),
]
GROUPED_LAYOUTS = [c for c in LAYOUTS if c[2] != 64 and c[4] <= 64]
PATTERNS = ("prefix", "scattered", "one", "none", "all")
_lid = lambda c: "B%d_h%d_dh%d_nj%d_n%d_g%d" % c   # noqa: E731


def _pattern(name, B, nj, n, groups):
    """(B, ntok) bool key mask over [nj joint tokens | groups x n]; the joint tokens' entries are deliberately False where
    the pattern is not "all": the entries must ignore them."""
    m = torch.zeros(B, groups, n, dtype=torch.bool)
    if name == "prefix":        # the first members of every group (TimeSformer's time layout of a prefix frame mask) ...
        for b in range(B):
            m[b, :, :max(1, (n * (b + 1)) // (B + 1))] = True
            m[b, : groups // 3] = b % 2 == 0    # ... and whole groups on or off (its spatial layout)
    elif name == "scattered":
        m = torch.rand(B, groups, n, generator=torch.Generator().manual_seed(21)) < 0.6
    elif name == "one":
        m[:, :, n // 2] = True
    elif name == "all":
        m[:] = True
    joint = torch.full((B, nj), name == "all", dtype=torch.bool)
    return torch.cat((joint, m.reshape(B, groups * n)), 1)


def _inputs(case, seed):
    B, heads, dh, nj, n, groups = case
    ntok = nj + groups * n
    g = torch.Generator().manual_seed(seed)
    Q, K, K0, V = (torch.randn(B, heads, ntok, dh, generator=g) * (dh ** -0.25) for _ in range(4))
    K[:, :, :nj] = K0[:, :, :nj]   # the joint rows of K carry no RoPE
    dO = torch.randn(B, ntok, heads * dh, generator=g)
    return Q, K, K0, V, dO


def _forward(L, q, k, k0, v, case, km, mpq, out, lse):
    """hp_sformer_attention_lse_masked (lse given) or hp_sformer_attention_masked; km None: the unmasked entries."""
    B, heads, dh, nj, n, groups = case
    ntok = nj + groups * n
    st = _lib.current_stream_handle(q.device)
    ws = torch.empty(int(L.hp_sformer_attention_workspace_bytes(B, heads, dh)) // 4 + 1, device=q.device)
    a = (q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr())
    d = (B, heads, dh, ntok, nj, n, groups)
    if km is None:
        if lse is None:
            _lib.check(L.hp_sformer_attention(*a, *d, 0, ws.data_ptr(), st), "hp_sformer_attention")
        else:
            _lib.check(L.hp_sformer_attention_lse(*a, lse.data_ptr(), *d, ws.data_ptr(), st), "hp_sformer_attention_lse")
    elif lse is None:
        _lib.check(L.hp_sformer_attention_masked(*a, *d, km.data_ptr(), mpq, ws.data_ptr(), st), "hp_sformer_attention_masked")
    else:
        _lib.check(L.hp_sformer_attention_lse_masked(*a, lse.data_ptr(), *d, km.data_ptr(), mpq, ws.data_ptr(), st),
                   "hp_sformer_attention_lse_masked")


def _backward(L, q, k, k0, v, out, do, lse, case, km, mpq, grads, grouped=False):
    B, heads, dh, nj, n, groups = case
    ntok = nj + groups * n
    name = "hp_sformer_attention_backward_grouped_masked" if grouped else "hp_sformer_attention_backward_masked"
    nb = getattr(L, name + "_workspace_bytes")(B, heads, dh, ntok, nj, groups)
    ws = torch.empty(int(nb) // 4 + 1, device=q.device)
    _lib.check(getattr(L, name)(q.data_ptr(), k.data_ptr(), k0.data_ptr(), v.data_ptr(), out.data_ptr(), do.data_ptr(), lse.data_ptr(),
                                *(t.data_ptr() for t in grads), B, heads, dh, ntok, nj, n, groups, km.data_ptr(), mpq, ws.data_ptr(), nb,
                                _lib.current_stream_handle(q.device)), name)


def _run_masked(L, dev, case, tensors, km_bool, mpq, grouped=False):
    """(out, lse, dQ, dK, dK0, dV, out of the inference entry) of the masked entries."""
    B, heads, dh, nj, n, groups = case
    ntok = nj + groups * n
    q, k, k0, v, do = tensors
    km = km_bool.to(dev).to(torch.uint8).contiguous()
    out, out_inf = torch.empty(B, ntok, heads * dh, device=dev), torch.empty(B, ntok, heads * dh, device=dev)
    lse = torch.empty(B, heads, ntok, device=dev)
    grads = [torch.empty_like(q) for _ in range(4)]
    _forward(L, q, k, k0, v, case, km, mpq, out, lse)
    _forward(L, q, k, k0, v, case, km, mpq, out_inf, None)
    _backward(L, q, k, k0, v, out, do, lse, case, km, mpq, grads, grouped)
    return [out, lse, *grads, out_inf]


def _grad_err(a, ref, scale):
    """rel_l2 against the float64 gradient.  Where that gradient is identically zero (a soft-max over ONE attendable key has
    the constant probability 1: nj = 1 with nothing else valid) rel_l2 is undefined; the error is then measured against the
    norm of the incoming gradient dO, which every attention gradient is linear in (Q, K, V are O(1) here)."""
    if float(ref.norm()) == 0.0:
        return float(a.double().norm()) / scale
    return rel_l2(a, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("mpq", [0, 1])
@pytest.mark.parametrize("case", LAYOUTS, ids=_lid)
def test_masked_attention_vs_float64(case, mpq):
    B, heads, dh, nj, n, groups = case
    L = _lib.lib()
    dev = torch.device("cuda")
    ntok = nj + groups * n
    Q, K, K0, V, dO = _inputs(case, seed=31)
    tensors = [t.to(dev).contiguous() for t in (Q, K, K0, V, dO)]
    for pat in PATTERNS:
        km = _pattern(pat, B, nj, n, groups)
        r1 = _run_masked(L, dev, case, tensors, km, mpq)
        r2 = _run_masked(L, dev, case, tensors, km, mpq)
        torch.cuda.synchronize()
        for a, b in zip(r1, r2):
            assert torch.equal(a, b), (pat, "two calls differ")
        assert torch.equal(r1[0], r1[6]), (pat, "the inference entry's out differs from the training forward's")
        Qd, Kd, K0d, Vd = (t.to(dev, torch.float64).requires_grad_(True) for t in (Q, K, K0, V))
        ref, ref_lse = _masked_attn_ref(Qd, Kd, K0d, Vd, nj, n, groups, km.to(dev), mpq)
        e_out = rel_l2(r1[0], ref.detach().permute(0, 2, 1, 3).reshape(B, ntok, -1))
        e_lse = rel_l2(r1[1], ref_lse.detach())
        dOd = dO.to(dev, torch.float64)
        (ref * dOd.view(B, ntok, heads, dh).permute(0, 2, 1, 3)).sum().backward()
        errs = [_grad_err(a, t.grad, float(dOd.norm())) for a, t in zip(r1[2:6], (Qd, Kd, K0d, Vd))]
        print(case, "mpq", mpq, pat, "out %.2e lse %.2e" % (e_out, e_lse), "dQ dK dK0 dV", ["%.2e" % e for e in errs])
        assert e_out < 1e-5 and e_lse < 1e-6, pat
        assert max(errs) < 1e-5, pat
        # a masked key gets exactly zero through the queries that leave it out: dK0 (joint queries) always; dK and dV too when the
        # patch queries apply the mask
        dead = ~km.to(dev)
        dead[:, :nj] = False
        if bool(dead.any()):
            sel = dead[:, None, :].expand(B, heads, ntok)
            for name, t in [("dK0", r1[4])] + ([("dK", r1[3]), ("dV", r1[5])] if mpq else []):
                assert float(t[sel].abs().max()) == 0.0, (pat, name)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LAYOUTS, ids=_lid)
def test_all_true_mask_is_bit_equal_to_the_unmasked_entries(case):
    B, heads, dh, nj, n, groups = case
    L = _lib.lib()
    dev = torch.device("cuda")
    ntok = nj + groups * n
    tensors = [t.to(dev).contiguous() for t in _inputs(case, seed=32)]
    q, k, k0, v, do = tensors
    out, out_inf = torch.empty(B, ntok, heads * dh, device=dev), torch.empty(B, ntok, heads * dh, device=dev)
    lse = torch.empty(B, heads, ntok, device=dev)
    _forward(L, q, k, k0, v, case, None, 0, out, lse)
    _forward(L, q, k, k0, v, case, None, 0, out_inf, None)
    plain = [out, lse, *xa.attention_backward(q, k, k0, v, out, do, lse, B, heads, dh, ntok, nj, n, groups), out_inf]
    km = torch.ones(B, ntok, dtype=torch.bool)
    names = ("out", "lse", "dQ", "dK", "dK0", "dV", "out (inference entry)")
    for mpq in (0, 1):
        got = _run_masked(L, dev, case, tensors, km, mpq)
        torch.cuda.synchronize()
        same = [bool(torch.equal(a, b)) for a, b in zip(got, plain)]
        print(case, "mpq", mpq, dict(zip(names, same)))
        assert all(same), (mpq, dict(zip(names, same)))
    if case in GROUPED_LAYOUTS:
        got = _run_masked(L, dev, case, tensors, km, 1, grouped=True)
        rg = xa.attention_backward_grouped(q, k, k0, v, out, do, lse, B, heads, dh, ntok, nj, n, groups)
        for name, a, b in zip(names[2:6], got[2:6], rg):
            assert torch.equal(a, b), ("grouped", name)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GROUPED_LAYOUTS, ids=_lid)
def test_masked_grouped_backward_is_bit_equal_to_masked_generic_backward(case):
    B, heads, dh, nj, n, groups = case
    L = _lib.lib()
    dev = torch.device("cuda")
    tensors = [t.to(dev).contiguous() for t in _inputs(case, seed=33)]
    for mpq in (0, 1):
        for pat in PATTERNS:
            km = _pattern(pat, B, nj, n, groups)
            gen = _run_masked(L, dev, case, tensors, km, mpq)
            grp = _run_masked(L, dev, case, tensors, km, mpq, grouped=True)
            grp2 = _run_masked(L, dev, case, tensors, km, mpq, grouped=True)
            torch.cuda.synchronize()
            for name, a, b, c in zip(("dQ", "dK", "dK0", "dV"), gen[2:6], grp[2:6], grp2[2:6]):
                assert torch.equal(a, b), (mpq, pat, name)
                assert torch.equal(b, c), (mpq, pat, name, "two calls differ")


GUARD = 64 * 1024                                  # floats either side (256 KB), as tests/test_head64.py
SENT = float.fromhex("0x1.5a5a5ap+100")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [(2, 3, 32, 24, 37, 3), (1, 2, 64, 7, 300, 2), (2, 2, 16, 1, 6, 70), (1, 2, 24, 1, 33, 5)], ids=_lid)
def test_masked_entries_write_only_their_outputs_and_read_only_their_mask(case):
    """The poison / guard pattern of tests/test_head64.py: `out`, `lse`, dQ .. dV sit between sentinel-filled guards that stay
    bit for bit while every output element is written.  key_mask is the LAST B * ntok bytes of its allocation, preceded by a
    guard region: results with that region all zero and all 0xff are equal, and equal to those with a tensor of its own (an
    index below the mask would read the guard and change a result; nothing is allocated behind it)."""
    B, heads, dh, nj, n, groups = case
    L = _lib.lib()
    dev = torch.device("cuda")
    ntok = nj + groups * n
    tensors = [t.to(dev).contiguous() for t in _inputs(case, seed=34)]
    q, k, k0, v, do = tensors
    km_bool = _pattern("scattered", B, nj, n, groups)
    grouped_ok = dh != 64 and n <= 64

    def guarded(shape):
        cnt = int(np.prod(shape))
        buf = torch.full((GUARD + cnt + GUARD,), SENT, device=dev)
        return buf, buf[GUARD:GUARD + cnt].view(shape)

    def intact(buf, t):
        return bool((buf[:GUARD] == SENT).all()) and bool((buf[GUARD + t.numel():] == SENT).all())

    names = ["out", "lse", "dQ", "dK", "dK0", "dV"]
    shapes = [(B, ntok, heads * dh), (B, heads, ntok)] + [(B, heads, ntok, dh)] * 4
    results = []
    for mpq in (0, 1):
        for grouped in ((False, True) if grouped_ok else (False,)):
            for fill in (0, 255):
                mbuf = torch.full((4 * GUARD + B * ntok,), fill, dtype=torch.uint8, device=dev)
                km = mbuf[4 * GUARD:].view(B, ntok)
                km.copy_(km_bool.to(dev).to(torch.uint8))
                bufs = [guarded(s) for s in shapes]
                _forward(L, q, k, k0, v, case, km, mpq, bufs[0][1], bufs[1][1])
                _backward(L, q, k, k0, v, bufs[0][1], do, bufs[1][1], case, km, mpq, [b[1] for b in bufs[2:]], grouped)
                ibuf, inf = guarded(shapes[0])
                _forward(L, q, k, k0, v, case, km, mpq, inf, None)
                torch.cuda.synchronize()
                for name, (buf, t) in zip(names + ["out (inference entry)"], bufs + [(ibuf, inf)]):
                    assert intact(buf, t), f"{name} was written outside its tensor"
                    assert not bool((t == SENT).any()), f"{name} has unwritten elements"
                assert bool((mbuf[:4 * GUARD] == fill).all())
                results.append([b[1].clone() for b in bufs])
            own = _run_masked(L, dev, case, tensors, km_bool, mpq, grouped)
            for res in results[-2:]:
                for name, a, b in zip(names, res, own):
                    assert torch.equal(a, b), (mpq, grouped, name, "depends on the bytes in front of key_mask")


def _train_run(m, video, mask, R=None):
    """Training-path output, {name: grad}, video grad."""
    m.zero_grad(set_to_none=True)
    x = video.detach().clone().requires_grad_(True)
    y = m.train()(x, mask=mask)
    assert y.grad_fn is not None
    R = loss_weights(y.shape) if R is None else R
    (y.double() * R.to(y.device)).sum().backward()
    return y.detach(), {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}, x.grad.detach()


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS)
def test_masked_timesformer_vs_reference_golden(key, golden):
    g = golden("frame_mask.npz")
    kw, m, video, mask = _module(g, key)
    m, video, mask = m.cuda(), video.cuda(), mask.cuda()
    y0 = m.eval()(video, mask=mask)
    assert y0.grad_fn is None and y0.shape == (2, 72)
    e_y = rel_l2(y0, g[f"{key}_y"])
    y, grads, vgrad = _train_run(m, video, mask)
    worst = golden_compare(g, key, grads, vgrad, 1e-4)
    print(f"{key}: eval forward rel-L2 {e_y:.2e}, worst gradient rel-L2 {worst:.2e}")
    assert e_y < 1e-4
    assert sorted(k for k, v in grads.items() if v is None) == sorted(g[f"{key}_none"].tolist())
    assert torch.equal(y, y0), "the training path's output differs from the no-graph path's"


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["plain6", "dh64"])
def test_masked_timesformer_properties(key, golden):
    g = golden("frame_mask.npz")
    kw, m, video, mask = _module(g, key)
    m, video, mask = m.cuda(), video.cuda(), mask.cuda()
    # 1. the pixels of masked frames do not matter (shift_tokens False)
    other = video.clone()
    other[~mask] = (torch.rand(other[~mask].shape, generator=torch.Generator().manual_seed(91)) * 9 - 4).cuda()
    y0 = m.eval()(video, mask=mask)
    assert torch.equal(m.eval()(other, mask=mask), y0)
    y, grads, vgrad = _train_run(m, video, mask)
    y_o, grads_o, _ = _train_run(m, other, mask)
    assert torch.equal(y, y0) and torch.equal(y_o, y0)
    # 2. their input gradient is exactly zero; every valid frame's is not
    assert float(vgrad[~mask].abs().max()) == 0.0
    assert all(float(vgrad[b, j].abs().max()) > 0 for b in range(2) for j in range(mask.shape[1]) if bool(mask[b, j]))
    # 3. an all-true mask is mask=None: forward bit for bit, every gradient bit for bit except the Linear weight gradients (their
    #    split reduction meets in fp32 atomics by the section's contract: compared at 1e-5)
    ones = torch.ones_like(mask)
    assert torch.equal(m.eval()(video, mask=ones), m.eval()(video))
    y_n, grads_n, vgrad_n = _train_run(m, video, None)
    y_1, grads_1, vgrad_1 = _train_run(m, video, ones)
    assert torch.equal(y_1, y_n) and torch.equal(vgrad_1, vgrad_n)
    linear_w = {name + ".weight" for name, mod in m.named_modules() if isinstance(mod, torch.nn.Linear)}
    for k in grads_n:
        if k in linear_w:
            e = rel_l2(grads_1[k], grads_n[k])
            assert e < 1e-5, (k, e)
        else:
            assert torch.equal(grads_1[k], grads_n[k]), k
    if key == "plain6":
        # 4. a prefix mask is truncation: sample 0 (mask 111100) against the same module on its first 4 frames without a mask
        yt = m.eval()(video[:1, :4].contiguous())
        e = rel_l2(y0[:1], yt)
        print(f"plain6: sample 0 with mask 111100 vs its first 4 frames unmasked: rel-L2 {e:.2e} "
              f"(vs the reference's truncated output {rel_l2(y0[:1], g['plain6_y_trunc4']):.2e})")
        assert e < 1e-4
    # a sample without a valid frame is legal: its queries see the class token only
    none = mask.clone()
    none[0] = False
    yz = m.eval()(video, mask=none)
    assert bool(torch.isfinite(yz).all()) and torch.equal(yz[1], y0[1])


@pytest.mark.gpu
def test_mask_refusals(golden):
    from hiddenpose_amd.NlosPoseSformer import NlosPoseSformer
    from hiddenpose_amd.tokenpose import TokenPose_L_base
    from test_sformer_train import CFGS
    from test_xformers import TP

    g = golden("frame_mask.npz")
    kw, m, video, mask = _module(g, "plain6")
    m, video = m.cuda().eval(), video.cuda()
    b, f = video.shape[:2]
    with pytest.raises(ValueError, match="float32"):
        m(video, mask=mask.cuda().float())
    with pytest.raises(ValueError, match=rf"\({b}, {f + 1}\)"):
        m(video, mask=torch.ones(b, f + 1, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="cpu"):
        m(video, mask=mask.cpu())
    with pytest.raises(ValueError):
        m.train()(video, mask=mask.cuda().float())
    assert m.eval()(video, mask=mask.cuda()).shape == (2, 72)
    # the other two heads refuse a mask exactly as before
    s = NlosPoseSformer(**CFGS["small"]).cuda()
    with pytest.raises(AssertionError, match="not supported"):
        s(torch.rand(1, 4, 1, 32, 32, device="cuda"), mask=torch.ones(1, 4, dtype=torch.bool, device="cuda"))
    t = TokenPose_L_base(**TP["learnable"]).cuda()
    with pytest.raises(AssertionError, match="masks are not supported"):
        t(torch.rand(1, 3, 16, 24, device="cuda"), mask=torch.ones(1, 5, dtype=torch.bool, device="cuda"))
