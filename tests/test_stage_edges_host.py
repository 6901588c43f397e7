"""Host-side argument checks of the U-Net / feature / loss stage entry points (csrc/unet_kernels.hip and the stage half of
csrc/misc_kernels.hip): every call below is refused BEFORE any device call, so the file runs on a machine without a GPU.  The
pointers are four host floats: a call that got past its checks would hand them to a kernel launch, which no device is there
to take."""
import ctypes as C

import pytest

HP_ERR_BAD_ARG, HP_ERR_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def p():
    one = (C.c_float * 4)()
    yield C.cast(one, C.c_void_p)


def check(lib, ret, *words, code=HP_ERR_BAD_ARG):
    """the call returned `code` and the library's message names every one of `words`"""
    assert ret == code, (ret, lib.hp_last_error_string())
    msg = lib.hp_last_error_string()
    for w in words:
        assert w in msg, (w, msg)


def test_maxpool_refuses_odd_sizes(hip_lib, p):
    for dims in ((3, 4, 4), (4, 5, 4), (4, 4, 7)):
        check(hip_lib, hip_lib.hp_maxpool3d_k2_forward(p, p, 1, *dims, None), b"hp_maxpool3d_k2_forward", b"even sizes")
        check(hip_lib, hip_lib.hp_maxpool3d_k2_backward(p, p, p, 1, *dims, None), b"hp_maxpool3d_k2_backward", b"even sizes")
        check(hip_lib, hip_lib.hp_maxpool3d_k2_backward_add(p, p, p, 1024, p, 1, 2, *dims, None),
              b"hp_maxpool3d_k2_backward_add", b"even sizes")


def test_channel_slice_copy_refuses_ragged_planes_and_slices_outside_the_buffer(hip_lib, p):
    for gather in (0, 1):
        check(hip_lib, hip_lib.hp_channel_slice_copy(p, p, 1, 1, 6, 2, 0, gather, None), b"hp_channel_slice_copy")   # V % 4 != 0
        check(hip_lib, hip_lib.hp_channel_slice_copy(p, p, 1, 3, 8, 4, 2, gather, None), b"hp_channel_slice_copy")   # 2 + 3 > 4
        check(hip_lib, hip_lib.hp_channel_slice_copy(p, p, 1, 1, 8, 4, -1, gather, None), b"hp_channel_slice_copy")  # c_off < 0


def test_conv1x1_refuses_what_it_has_no_kernel_for(hip_lib, p):
    check(hip_lib, hip_lib.hp_conv1x1_forward(p, p, p, p, 1, 9, 1, 4, None), b"at most 8 channels")
    check(hip_lib, hip_lib.hp_conv1x1_forward(p, p, p, p, 1, 1, 9, 4, None), b"at most 8 channels")
    check(hip_lib, hip_lib.hp_conv1x1_forward_sum(p, p, p, p, p, None, 1, 4, 1, 4, None), b"go together")    # addend without sum_out
    check(hip_lib, hip_lib.hp_conv1x1_forward_sum(p, p, p, None, p, p, 1, 4, 1, 4, None), b"go together")    # sum_out without addend
    check(hip_lib, hip_lib.hp_conv1x1_backward(p, p, p, p, p, p, 1, 3, 1, 4, None), b"3 -> 1", code=HP_ERR_UNSUPPORTED)
    check(hip_lib, hip_lib.hp_conv1x1_backward_sum(p, p, p, p, p, p, p, 1, 4, 2, 4, None), b"4 -> 2", code=HP_ERR_UNSUPPORTED)


def test_upsample_refuses_bad_slices_and_axes_beyond_its_tables(hip_lib, p):
    raw = (("hp_upsample_trilinear2x_forward", ()), ("hp_upsample_trilinear2x_backward", ()))
    ws = (("hp_upsample_trilinear2x_forward_ws", (p,)), ("hp_upsample_trilinear2x_backward_ws", (p,)))
    for name, extra in raw + ws:
        f = getattr(hip_lib, name)
        check(hip_lib, f(p, p, 1, 3, 2, 2, 4, 4, 2, *extra, None), name.encode())     # c_off + C = 5 > Ctot = 4
        check(hip_lib, f(p, p, 1, 1, 2, 2, 4, 4, -1, *extra, None), name.encode())    # c_off < 0
    for name, _ in raw:
        check(hip_lib, getattr(hip_lib, name)(p, p, 1, 1, 1024, 1024, 1, 1, 0, None), name.encode(), b"must not exceed 2048")
    # the workspace entries reach the same refusal through their fall-back: an axis beyond the separable kernels' tables
    for name, extra in ws:
        check(hip_lib, getattr(hip_lib, name)(p, p, 1, 1, 2047, 1, 1, 1, 0, *extra, None), b"must not exceed 2048")


def test_small_stage_entries_refuse_their_bad_sizes(hip_lib, p):
    check(hip_lib, hip_lib.hp_depth_top4(p, p, p, 1, 3, 4, None), b"depth must be >= 4")
    check(hip_lib, hip_lib.hp_leaky_add_forward(p, p, p, 6, 0.2, None), b"hp_leaky_add_forward")
    check(hip_lib, hip_lib.hp_leaky_backward(p, p, p, 6, 0.2, None), b"hp_leaky_backward")
    check(hip_lib, hip_lib.hp_noise_blur_poisson(p, p, 4, p, 2049, 0, 1, None), b"hp_noise_blur_poisson")
    check(hip_lib, hip_lib.hp_noise_blur_poisson(p, p, 4, p, -1, 0, 1, None), b"hp_noise_blur_poisson")
    check(hip_lib, hip_lib.hp_normalize_feature_forward(p, p, 1, 1 << 32, 10.0, p, None), b"hp_normalize_feature_forward")
    check(hip_lib, hip_lib.hp_normalize_feature_forward(p, p, 0, 4, 10.0, p, None), b"hp_normalize_feature_forward")


def _gn_forward(lib, p, B, C_, G, V):
    return lib.hp_groupnorm_relu_forward_v2(p, p, B, C_, G, V, p, p, 1e-5, None, p, p, p, p, p, None)


def _gn_backward(lib, p, B, C_, G, V):
    return lib.hp_groupnorm_relu_backward_v2(p, p, p, B, C_, G, V, p, p, p, p, p, p, p, p, None)


def test_groupnorm_refuses_channels_that_do_not_split_into_groups(hip_lib, p):
    check(hip_lib, _gn_forward(hip_lib, p, 1, 6, 4, 8), b"hp_groupnorm_relu_forward", b"multiple of G")
    check(hip_lib, _gn_backward(hip_lib, p, 1, 6, 4, 8), b"hp_groupnorm_relu_backward", b"multiple of G")
    check(hip_lib, hip_lib.hp_groupnorm_relu_forward(p, p, 1, 6, 4, 8, p, p, 1e-5, p, p, p, None), b"multiple of G")


def test_groupnorm_refuses_empty_sizes_instead_of_dividing_by_zero(hip_lib, p):
    """G = 0 used to reach `C % G` inside the argument check: an integer division by zero on the host (SIGFPE), not a refusal."""
    for B, C_, G, V in ((1, 4, 0, 8), (0, 4, 2, 8), (1, 0, 2, 8), (1, 4, 2, 0), (1, 4, -2, 8)):
        check(hip_lib, _gn_forward(hip_lib, p, B, C_, G, V), b"hp_groupnorm_relu_forward", b"must be positive")
        check(hip_lib, _gn_backward(hip_lib, p, B, C_, G, V), b"hp_groupnorm_relu_backward", b"must be positive")
    check(hip_lib, hip_lib.hp_groupnorm_relu_forward(p, p, 1, 4, 0, 8, p, p, 1e-5, p, p, p, None), b"must be positive")
