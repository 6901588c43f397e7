"""rotary_emb=False for TimeSformer and NlosPoseSformer (models/transformer.py:182-187, models/NlosPoseSformer.py:55-60; DESIGN
4.4.8), the part that needs no device: the modules construct and own the reference's learned table under the reference's key,
their state_dict equals the schema captured from the reference (tests/golden/pos_emb.npz) and round-trips strictly, a clip
longer than the table is an IndexError, and hp_tokens_assemble_forward / _backward refuse bad arguments with HP_ERR_BAD_ARG and
a message naming the argument before any device call."""
import json

import pytest
import torch

import hiddenpose_amd._xformer_autograd as xa

KEYS = ("ts_plain", "ts_short", "ts_mask", "ts_shift", "ts_dh64", "sf_short")
FAKE = 0x1000      # a non-null address that is never dereferenced: every check below comes before any device call
HP_ERR_BAD_ARG = -1


def module(g, key):
    from hiddenpose_amd.NlosPoseSformer import NlosPoseSformer
    from hiddenpose_amd.transformer import TimeSformer

    kw = json.loads(str(g[f"{key}_cfg"]))
    assert kw["rotary_emb"] is False
    return kw, (TimeSformer if key.startswith("ts_") else NlosPoseSformer)(**kw)


@pytest.mark.parametrize("key", KEYS)
def test_modules_construct_with_the_reference_state_dict(key, golden):
    g = golden("pos_emb.npz")
    kw, m = module(g, key)
    sd = m.state_dict()
    assert sorted([k, list(v.shape)] for k, v in sd.items()) == json.loads(str(g[f"{key}_sd"]))
    assert not any("rot_emb" in k for k in sd)
    assert not hasattr(m, "frame_rot_emb") and not hasattr(m, "image_rot_emb")
    table = "pos_emb" if key.startswith("ts_") else "pose_emb"
    n = (kw["image_size"] // kw["patch_size"]) ** 2
    emb = getattr(m, table)
    assert isinstance(emb, torch.nn.Embedding) and tuple(emb.weight.shape) == (kw["num_frames"] * n + 1, kw["dim"])
    assert emb.weight.requires_grad and m.position_table() is emb.weight
    # nn.Embedding's default initialisation, N(0, 1): nothing re-initialises the table
    torch.manual_seed(5)
    fresh = type(m)(**kw)
    torch.manual_seed(5)
    twin = type(m)(**kw)
    assert torch.equal(getattr(fresh, table).weight, getattr(twin, table).weight)
    w = emb.weight.detach()
    assert abs(float(w.mean())) < 0.1 and 0.9 < float(w.std()) < 1.1
    # a strict round trip through a fresh module
    other = type(m)(**kw)
    assert other.load_state_dict(sd, strict=True).missing_keys == []
    assert all(torch.equal(v, other.state_dict()[k]) for k, v in sd.items())


@pytest.mark.parametrize("key", ["ts_plain", "sf_short"])
def test_function_takes_the_table(key, golden):
    """The table is one more tensor of the training path, right behind the leading tokens; the rotary module has none."""
    kw, m = module(golden("pos_emb.npz"), key)
    ps = xa.timesformer_params(m) if key.startswith("ts_") else xa.trainable_params(m)
    assert ps[3] is m.position_table()
    rot = type(m)(**dict(kw, rotary_emb=True))
    ps_rot = xa.timesformer_params(rot) if key.startswith("ts_") else xa.trainable_params(rot)
    assert rot.position_table() is None and len(ps_rot) == len(ps) - 1
    assert "frame_rot_emb.inv_freqs" in rot.state_dict() and "image_rot_emb.scales" in rot.state_dict()
    if key.startswith("ts_"):
        assert {id(p) for p in ps} == {id(p) for p in m.parameters()}


def test_a_clip_longer_than_the_table_is_an_index_error(golden):
    """Raised from shapes alone, before the device check: a CPU tensor gets the IndexError, not the 'needs a HIP device' error."""
    g = golden("pos_emb.npz")
    kw, m = module(g, "ts_plain")      # 4 frames of 16 patches: 65 rows
    with pytest.raises(IndexError, match=r"ntok 81 .* 65 rows.* 4 frames"):
        m(torch.zeros(1, 5, 1, 32, 32))
    with pytest.raises(IndexError, match=r"ntok 101 .* 65 rows.* 2 frames"):
        m(torch.zeros(1, 4, 1, 40, 40))      # a larger image: 25 patches per frame
    kw, m = module(g, "sf_short")      # 8 frames of 4 patches: 33 rows, 24 of them taken by the joint tokens
    for f in (3, 8):
        with pytest.raises(IndexError, match=rf"ntok {24 + 4 * f} .* 33 rows.* 2 frames"):
            m(torch.zeros(2, f, 2, 16, 16))
    # a clip that fits passes the check and reaches the device check
    from hiddenpose_amd._lib import HiddenPoseHipError

    with pytest.raises(HiddenPoseHipError, match="HIP device"):
        m(torch.zeros(2, 2, 2, 16, 16))


def refused(L, rc, *words):
    msg = L.hp_last_error_string()
    assert rc == HP_ERR_BAD_ARG, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def test_argument_checks_come_before_any_device_call(hip_lib):
    L = hip_lib
    fwd = lambda lead=FAKE, emb=FAKE, pos=FAKE, x=FAKE, B=2, nl=1, ntok=17, dim=64, rows=17: \
        L.hp_tokens_assemble_forward(lead, emb, pos, x, B, nl, ntok, dim, rows, None)   # noqa: E731
    bwd = lambda dx=FAKE, dlead=FAKE, dpos=FAKE, demb=FAKE, B=2, nl=1, ntok=17, dim=64, rows=17: \
        L.hp_tokens_assemble_backward(dx, dlead, dpos, demb, B, nl, ntok, dim, rows, None)   # noqa: E731
    refused(L, fwd(x=None), "hp_tokens_assemble_forward", "null x")
    refused(L, fwd(emb=None), "hp_tokens_assemble_forward", "null emb")
    refused(L, fwd(lead=None), "hp_tokens_assemble_forward", "null lead")
    refused(L, bwd(dx=None), "hp_tokens_assemble_backward", "null dx")
    for call, who in ((fwd, "hp_tokens_assemble_forward"), (bwd, "hp_tokens_assemble_backward")):
        refused(L, call(ntok=1), who, "Ntok 1 must exceed nl 1")
        refused(L, call(nl=24, ntok=20), who, "Ntok 20 must exceed nl 24")
        refused(L, call(nl=-1), who, "nl -1")
        refused(L, call(B=0), who, "B 0")
        refused(L, call(B=-3), who, "B -3")
        refused(L, call(dim=0), who, "dim 0")
        refused(L, call(ntok=18), who, "Ntok 18 exceeds pos_rows 17")
    # without a table pos_rows is not read: these pass every check (and would launch, so they are not called here with a
    # device pointer); all three backward outputs null is success without a launch
    assert bwd(dlead=None, dpos=None, demb=None, ntok=18) == 0
