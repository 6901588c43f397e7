"""CPU-side checks of the strided FeatureExtraction entry points of the C ABI (hp_fe_entry_*, hp_bcast_add_forward,
hp_channel_sum): the symbols exist, the workspace query is positive and monotone, and every invalid argument is refused with
HP_ERR_BAD_ARG before any device call (so these run without a GPU; the pointers are never dereferenced)."""
import pytest

from hiddenpose_amd import _lib

HP_ERR_BAD_ARG = -1
P = 0x1000   # a non-null address that a refused call never touches

NEW_SYMBOLS = ["hp_fe_entry_forward", "hp_fe_entry_backward_workspace_bytes", "hp_fe_entry_backward", "hp_bcast_add_forward",
               "hp_channel_sum"]


def test_new_symbols_exist(hip_lib):
    for name in NEW_SYMBOLS:
        assert hasattr(hip_lib, name), name
        assert name in _lib.SIGNATURES, name


@pytest.mark.parametrize("stride", [1, 2])
def test_backward_workspace_positive_and_monotone(hip_lib, stride):
    q = hip_lib.hp_fe_entry_backward_workspace_bytes
    for D, H, W in [(1, 1, 1), (7, 9, 11), (64, 64, 64), (1024, 256, 256)]:
        prev = 0
        for B in (1, 2, 3, 8):
            n = q(B, 2, D, H, W, stride)
            assert n > 0 and n % 4 == 0 and n >= prev, (B, D, H, W, n, prev)
            prev = n
        prev = 0
        for C in (1, 2, 3, 4, 5, 9, 64):
            n = q(2, C, D, H, W, stride)
            assert n > 0 and n >= prev, (C, D, H, W, n, prev)
            prev = n
    # arguments the backward would refuse need no workspace
    assert q(1, 1, 8, 8, 8, 3) == 0 and q(1, 0, 8, 8, 8, 2) == 0 and q(0, 1, 8, 8, 8, 2) == 0 and q(1, 1, 8, 0, 8, 2) == 0


def _forward(hip_lib, x=P, w=P, bias=P, box_w=P, a=P, box=P, B=1, C=2, D=8, H=8, W=8, stride=2):
    return hip_lib.hp_fe_entry_forward(x, w, bias, box_w, a, box, B, C, D, H, W, stride, None)


def _backward(hip_lib, x=P, ga=P, gbox=P, w=P, box_w=P, dw=P, dbias=P, dbox_w=P, gx=P, B=1, C=2, D=8, H=8, W=8, stride=2, ws=P):
    return hip_lib.hp_fe_entry_backward(x, ga, gbox, w, box_w, dw, dbias, dbox_w, gx, B, C, D, H, W, stride, ws, None)


BAD_SHAPES = [dict(stride=0), dict(stride=3), dict(stride=-2), dict(C=0), dict(C=-1), dict(B=0), dict(D=0), dict(H=-4), dict(W=0),
              dict(D=1 << 11, H=1 << 9, W=1 << 9)]   # 2^29 voxels per sample: past the kernels' 32-bit byte offsets


@pytest.mark.parametrize("kw", BAD_SHAPES, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_invalid_shapes_are_refused(hip_lib, kw):
    assert _forward(hip_lib, **kw) == HP_ERR_BAD_ARG
    assert hip_lib.hp_last_error_string()
    assert _backward(hip_lib, **kw) == HP_ERR_BAD_ARG


@pytest.mark.parametrize("name", ["x", "w", "box_w", "a", "box"])
def test_forward_null_required_pointer_is_refused(hip_lib, name):
    assert _forward(hip_lib, **{name: None}) == HP_ERR_BAD_ARG
    assert b"null" in hip_lib.hp_last_error_string()


@pytest.mark.parametrize("name", ["x", "ga", "gbox", "w", "box_w", "dw", "dbox_w", "ws"])
def test_backward_null_required_pointer_is_refused(hip_lib, name):
    assert _backward(hip_lib, **{name: None}) == HP_ERR_BAD_ARG
    assert b"null" in hip_lib.hp_last_error_string()


def test_join_invalid_arguments_are_refused(hip_lib):
    add, csum = hip_lib.hp_bcast_add_forward, hip_lib.hp_channel_sum
    for args in [(None, P, P, 1, 2, 8), (P, None, P, 1, 2, 8), (P, P, None, 1, 2, 8), (P, P, P, 0, 2, 8), (P, P, P, 1, 0, 8),
                 (P, P, P, 1, 2, 0), (P, P, P, 256, 256, 8)]:
        assert add(*args, None) == HP_ERR_BAD_ARG, args
    for args in [(None, P, 1, 2, 8), (P, None, 1, 2, 8), (P, P, 0, 2, 8), (P, P, 1, 0, 8), (P, P, 1, 2, 0), (P, P, 65536, 2, 8)]:
        assert csum(*args, None) == HP_ERR_BAD_ARG, args
