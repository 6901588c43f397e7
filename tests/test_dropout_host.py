"""CPU-side checks of the seeded dropout (hp_dropout_forward / hp_dropout_mask / hp_ge[g]lu_backward_dropout):
the NumPy model of the generator that the GPU tests compare against (known answers, keep rate, stream independence), every
refusal of the C entries as a status and a message with no device present, and the golden file's per-site kept counts."""
import numpy as np
import pytest

import dropout_ref as D

FAKE = 0x1000      # a non-null address that is never dereferenced: every check below comes before any device call
N = 1 << 20


@pytest.mark.parametrize("counter,key,expect", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, expect):
    assert " ".join("%08x" % int(v) for v in D.philox4x32_10(counter, key)) == expect


def test_threshold_and_scale_ends():
    assert D.threshold(0.0) == 0 and D.threshold(1.0) == 1 << 32 and D.threshold(0.5) == 1 << 31
    assert D.keep_mask(1000, 0, 0.0, 7, 7).all() and not D.keep_mask(1000, 0, 1.0, 7, 7).any()
    assert D.scale(0.0) == 1.0 and D.scale(1.0) == 0.0 and D.scale(0.5) == 2.0
    assert D.stream_id(3, 5) == (3 << 20) | 5


@pytest.mark.parametrize("seed,stream", [(1234, 0), (1234, 1), (0x9E3779B97F4A7C15, 0x70003)])
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_rate(p, seed, stream):
    """The kept count of 2^20 elements within 4 sigma of n (1 - p), sigma = sqrt(n p (1 - p))."""
    kept = int(D.keep_mask(N, 0, p, seed, stream).sum())
    z = (kept - N * (1 - p)) / np.sqrt(N * p * (1 - p))
    print(f"p {p} seed {seed:#x} stream {stream:#x}: kept {kept}, {z:+.2f} sigma")
    assert abs(z) <= 4.0


def test_streams_are_independent():
    """Streams 0 and 1 at p = 0.5 agree on a fraction of the elements within 4 sigma of 1/2 (sigma = sqrt(n) / 2 elements)."""
    agree = int((D.keep_mask(N, 0, 0.5, 1234, 0) == D.keep_mask(N, 0, 0.5, 1234, 1)).sum())
    z = (agree - N / 2) / (np.sqrt(N) / 2)
    print(f"streams 0 / 1 agree on {agree} of {N}: {z:+.2f} sigma")
    assert abs(z) <= 4.0


def test_mask_does_not_depend_on_slicing():
    whole = D.keep_mask(70001, 5, 0.3, 99, 4)
    parts = np.concatenate([D.keep_mask(1023, 5, 0.3, 99, 4), D.keep_mask(70001 - 1023, 5 + 1023, 0.3, 99, 4)])
    assert np.array_equal(whole, parts)
    assert np.array_equal(D.keep_mask(9, (1 << 34) + 1, 0.5, 1, 2), D.keep_mask(12, 1 << 34, 0.5, 1, 2)[1:10])


def refused(hip_lib, rc, *words):
    msg = hip_lib.hp_last_error_string()
    assert rc == -1, (rc, msg)
    for w in words:
        assert w.encode() in msg, (w, msg)


def test_argument_checks_come_before_any_device_call(hip_lib):
    L = hip_lib
    fwd = lambda x=FAKE, a=None, y=FAKE, n=8, first=0, p=0.1: L.hp_dropout_forward(x, a, y, n, first, p, 1, 2, None)
    msk = lambda m=FAKE, n=8, first=0, p=0.1: L.hp_dropout_mask(m, n, first, p, 1, 2, None)
    geglu = lambda u=FAKE, dg=FAKE, du=FAKE, rows=2, hid=4, p=0.1: L.hp_geglu_backward_dropout(u, dg, du, rows, hid, p, 1, 2, None)
    gelu = lambda u=FAKE, dy=FAKE, du=FAKE, n=8, p=0.1: L.hp_gelu_backward_dropout(u, dy, du, n, p, 1, 2, None)
    refused(L, fwd(x=None), "hp_dropout_forward", "null x")
    refused(L, fwd(y=None), "hp_dropout_forward", "null y")
    refused(L, msk(m=None), "hp_dropout_mask", "null mask")
    for call, who in ((fwd, "hp_dropout_forward"), (msk, "hp_dropout_mask")):
        refused(L, call(n=-1), who, "n -1")
        refused(L, call(first=-1), who, "first -1")
    for call, who in ((fwd, "hp_dropout_forward"), (msk, "hp_dropout_mask"), (geglu, "hp_geglu_backward_dropout"),
                      (gelu, "hp_gelu_backward_dropout")):
        for bad in (-0.1, 1.5, float("nan")):
            refused(L, call(p=bad), who, "outside [0, 1]")
    for kw in ({"u": None}, {"dg": None}, {"du": None}, {"rows": 0}, {"hid": 0}):
        refused(L, geglu(**kw), "hp_geglu_backward_dropout", "bad argument")
    for kw in ({"u": None}, {"dy": None}, {"du": None}, {"n": 0}):
        refused(L, gelu(**kw), "hp_gelu_backward_dropout", "bad argument")
    # nothing to do: success without a launch (no device is touched, so this passes without one)
    assert fwd(x=None, y=None, n=0) == 0 and fwd(n=0, p=1.0) == 0
    assert msk(m=None, n=0) == 0


KEYS = ("sf_small", "ts_plain", "ts_plain_ff", "tp_learnable", "tp_sinefull")
SEED, STEP = 1234, 3    # tests/golden/make_dropout_goldens.py


@pytest.mark.parametrize("key", KEYS)
def test_golden_kept_counts_are_the_models(key, golden):
    g = golden("dropout_grads.npz")
    ps, kept, numel = g[f"{key}_p"], g[f"{key}_kept"], g[f"{key}_numel"]
    assert len(ps) == len(kept) == len(numel) == {"sf_small": 4, "ts_plain": 6, "ts_plain_ff": 6, "tp_learnable": 10,
                                                  "tp_sinefull": 19}[key]
    for site, (p, k, n) in enumerate(zip(ps, kept, numel)):
        assert int(D.keep_mask(int(n), 0, float(p), SEED, D.stream_id(STEP, site)).sum()) == int(k), (key, site)
    if key == "ts_plain_ff":
        assert [float(p) for p in ps] == [0.0, 0.0, 0.2] * 2 and all(int(k) == int(n) for p, k, n in zip(ps, kept, numel) if p == 0)
