"""CPU tests of how the host planner treats the row-panel kernel's variant id (csrc/conv_plan.hip rowpanel_ok):
honoured only when forced on a conv the kernel can run, never picked by the scoring, no GroupNorm statistics.
The planner dereferences no pointer, so every pointer is a dummy."""
import ctypes as C

import pytest

ROWPANEL = 49


def _gemm(_lib, M, N, K, ksize=1):
    a = _lib.ConvArgs()
    a.batch, a.ho, a.wo, a.cout, a.nseg = 1, M, 1, N, 1
    s = a.seg[0]
    s.src0 = 0x1000; s.c_split = K; s.cin = K; s.ld0 = K; s.h = M; s.w = 1
    s.ksize = ksize; s.stride = 1; s.pad = ksize // 2
    a.weight = 0x2000; a.out = 0x3000; a.out_ld = N
    a.k_total = ksize * ksize * ((K + 63) // 64 * 64)
    return a


def _plan(sdk, a):
    from sd_amd import _lib
    info = _lib.ConvPlanInfo()
    rc = sdk.library().sdk_conv2d_plan(C.byref(a), C.byref(info))
    return rc, info


@pytest.mark.parametrize("M,N,K", [(65536, 960, 320), (65536, 320, 320), (257, 200, 96), (300, 2560, 32)])
def test_forced_rowpanel_is_honoured(sdk, M, N, K):
    from sd_amd import _lib
    L = sdk.library()
    L.sdk_kernel_name.restype = C.c_char_p
    assert L.sdk_kernel_name(ROWPANEL) == b"conv_rowpanel_kernel"
    a = _gemm(_lib, M, N, K)
    rc, auto = _plan(sdk, a)
    assert rc == 0 and auto.variant != ROWPANEL            # the scoring never picks it
    a.variant_hint = ROWPANEL + 1
    for split in (0, 1):
        a.split_k = split
        rc, info = _plan(sdk, a)
        assert rc == 0 and info.variant == ROWPANEL and info.split_k == 1 and info.workspace_bytes == 0
        assert info.grid_tiles == -(-M // 256) * -(-N // 160) and info.gn_chunks == 0
        assert info.flops == 2.0 * M * N * K
    a.residual, a.res_ld = 0x4000, N                        # bias and residual stay inside its reach
    a.bias = 0x5000
    rc, info = _plan(sdk, a)
    assert rc == 0 and info.variant == ROWPANEL
    a.gn_partial = 0x6000                                   # it emits no GroupNorm statistics
    rc, _ = _plan(sdk, a)
    assert rc != 0


def test_forced_rowpanel_falls_back_outside_its_reach(sdk):
    """K > 320, K % 32 != 0, 3x3, N > 2560, an embedding row, a split of K, the GEGLU and fp32 outputs, a second
    segment's worth of concat: the forced id is not honoured and the plan is the one of the unforced call."""
    from sd_amd import _lib

    def differs(mut, M=600, N=640, K=320, ksize=1):
        a = _gemm(_lib, M, N, K, ksize)
        mut(a)
        rc0, auto = _plan(sdk, a)
        a.variant_hint = ROWPANEL + 1
        rc, info = _plan(sdk, a)
        assert rc == rc0 == 0
        assert info.variant == auto.variant != ROWPANEL, (info.variant, auto.variant)

    differs(lambda a: None, K=352)
    differs(lambda a: None, K=72)
    differs(lambda a: None, K=64, ksize=3)
    differs(lambda a: None, N=2568)

    def row_bias(a):
        a.row_bias, a.row_bias_ld = 0x7000, a.cout
    differs(row_bias)

    def split2(a):
        a.split_k = 2
    differs(split2)

    def geglu(a):
        a.out_mode, a.out_ld = 2, a.cout // 2
    differs(geglu)

    def rows_f32(a):
        a.out_mode = 3
    differs(rows_f32)

    def concat(a):
        s = a.seg[0]
        s.c_split, s.ld0, s.src1, s.ld1 = 64, 64, 0x8000, a.seg[0].cin - 64
    differs(concat)
