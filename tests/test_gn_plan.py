"""CPU tests of the GroupNorm host plan (``sdk_group_norm_plan``): the planner every GroupNorm entry point routes
through, called with dummy non-null addresses — no device is touched and no pointer is followed.  The routing table
below was derived by hand from the thresholds and reciprocal-exactness rules, not from the planner's output."""
import ctypes as C

import pytest

GIVEN, SLICE, CHUNKED, PARTS = "given", "slice", "chunked", "parts"
NONE, IN_STATS, FLAT, ROW, STRIDE = "none", "in_stats", "flat", "row", "stride"


def _args(_lib, B, H, W, Ch, groups=32, c_split=None):
    a = _lib.GroupNormArgs()
    a.src0, a.scale, a.shift = 0x1000, 0x2000, 0x3000
    a.c_split = c_split or Ch
    if a.c_split < Ch:
        a.src1, a.ld1 = 0x4000, Ch - a.c_split
    a.ld0 = a.c_split
    a.batch, a.hw, a.channels, a.groups, a.eps = B, H * W, Ch, groups, 1e-5
    return a


def _plan(sdk, a, H, W, pad, nch=(0, 0), stats=True, apply=True, single=True):
    """(rc, (stats, apply, launches), workspace_bytes)"""
    from sd_amd import _lib
    info = _lib.GroupNormPlanInfo()
    rc = sdk.library().sdk_group_norm_plan(C.byref(a), int(stats), int(apply), H, W, pad, nch[0], nch[1], int(single),
                                           C.byref(info))
    return rc, (_lib.GN_STATS[info.stats], _lib.GN_APPLY[info.apply], info.launches), info.workspace_bytes


# B, H, W, C, groups, c_split, pad, (nch0, nch1) -> statistics, apply, launches
TABLE = [
    ((3, 7, 5, 64, 32, None, 1, (0, 0)), (SLICE, IN_STATS, 1)),
    ((2, 8, 8, 2560, 32, None, 0, (0, 0)), (SLICE, IN_STATS, 1)),
    ((2, 32, 32, 320, 32, None, 1, (0, 0)), (SLICE, FLAT, 2)),
    ((2, 64, 64, 320, 32, None, 1, (0, 0)), (CHUNKED, FLAT, 3)),
    ((2, 64, 64, 320, 32, None, 0, (0, 0)), (CHUNKED, FLAT, 3)),
    ((2, 16, 16, 640, 32, None, 1, (4, 0)), (PARTS, IN_STATS, 1)),
    ((2, 16, 16, 960, 32, 640, 1, (2, 1)), (PARTS, IN_STATS, 1)),
    ((2, 16, 16, 640, 32, None, 1, (32, 0)), (PARTS, FLAT, 2)),
    ((2, 32, 32, 320, 32, None, 1, (4, 0)), (PARTS, FLAT, 2)),
    ((1, 128, 128, 32, 32, None, 1, (0, 0)), (CHUNKED, ROW, 3)),
    ((1, 128, 128, 32, 32, None, 0, (0, 0)), (CHUNKED, STRIDE, 3)),
    ((2, 16, 16, 8, 8, None, 1, (0, 0)), (SLICE, STRIDE, 2)),
    ((2, 16, 16, 8, 8, None, 0, (0, 0)), (SLICE, STRIDE, 2)),
    ((1, 128, 128, 8, 8, None, 1, (0, 0)), (CHUNKED, STRIDE, 3)),
]


@pytest.mark.parametrize("case, want", TABLE)
def test_group_norm_plan_table(sdk, case, want):
    from sd_amd import _lib
    B, H, W, Ch, groups, c_split, pad, nch = case
    a = _args(_lib, B, H, W, Ch, groups, c_split)
    rc, got, ws = _plan(sdk, a, H, W, pad, nch)
    assert rc == 0, sdk.library().sdk_last_error()
    assert got == want
    # the workspace is the chunked statistics' alone
    assert ws == (sdk.library().sdk_group_norm_workspace(B, H * W, Ch) if want[0] == CHUNKED else 0)
    if want[0] == CHUNKED:
        assert ws > 0


def test_group_norm_plan_film_never_single_launch(sdk):
    """sdk_group_norm_film folds FiLM into the affine between statistics and apply: two launches where
    sdk_group_norm takes one."""
    from sd_amd import _lib
    rc, got, _ = _plan(sdk, _args(_lib, 3, 7, 5, 64), 7, 5, 1, single=False)
    assert rc == 0 and got == (SLICE, FLAT, 2)
    rc, got, _ = _plan(sdk, _args(_lib, 2, 16, 16, 640), 16, 16, 1, (4, 0), single=False)
    assert rc == 0 and got == (PARTS, FLAT, 2)


def test_group_norm_plan_halves(sdk):
    """The statistics-only and apply-only entry points are the two halves of the same plan."""
    from sd_amd import _lib
    a = _args(_lib, 2, 64, 64, 320)
    assert _plan(sdk, a, 64, 64, 0, apply=False)[1] == (CHUNKED, NONE, 2)
    assert _plan(sdk, a, 64, 64, 1, stats=False)[1] == (GIVEN, FLAT, 1)
    assert _plan(sdk, _args(_lib, 2, 8, 8, 2560), 8, 8, 0, apply=False)[1] == (SLICE, NONE, 1)
    assert _plan(sdk, _args(_lib, 2, 16, 16, 640), 16, 16, 0, (4, 0), apply=False)[1] == (PARTS, NONE, 1)
    # a concat with partials for one source only has none
    assert _plan(sdk, _args(_lib, 2, 16, 16, 960, c_split=640), 16, 16, 1, (2, 0))[1] == (SLICE, FLAT, 2)
    a = _args(_lib, 1, 128, 128, 32)
    assert _plan(sdk, a, 128, 128, 1, stats=False)[1] == (GIVEN, ROW, 1)
    assert _plan(sdk, a, 128, 128, 0, stats=False)[1] == (GIVEN, STRIDE, 1)
    a.batch = 0                                                    # an empty batch is no work
    assert _plan(sdk, a, 128, 128, 1)[:2] == (0, (GIVEN, NONE, 0))


def _bad(sdk, mutate, H=16, W=16, pad=1, nch=(0, 0), Ch=64, c_split=None, **kw):
    from sd_amd import _lib
    a = _args(_lib, 2, 16, 16, Ch, c_split=c_split)
    assert _plan(sdk, a, 16, 16, 1, **kw)[0] == 0                  # well-formed before
    mutate(a)
    return _plan(sdk, a, H, W, pad, nch, **kw)[0] != 0


def test_group_norm_plan_validates_on_host(sdk):
    """Every argument error the GroupNorm entry points report is reported by the plan."""
    def setter(**fields):
        def f(a):
            for k, v in fields.items():
                setattr(a, k, v)
        return f
    nop = setter()
    assert _bad(sdk, setter(src0=None))
    assert _bad(sdk, setter(scale=None), stats=False)              # a given affine must be there
    assert _bad(sdk, setter(shift=None), single=False)              # FiLM folds into the buffers
    assert _bad(sdk, setter(channels=60, c_split=60))               # channels % 8
    assert _bad(sdk, setter(c_split=60))                            # c_split % 8
    assert _bad(sdk, setter(c_split=0))
    assert _bad(sdk, setter(c_split=72))                            # c_split > channels
    assert _bad(sdk, setter(groups=0))
    assert _bad(sdk, setter(groups=24))                             # channels % groups
    assert _bad(sdk, setter(channels=8192, c_split=8192, groups=1))  # > 256 channels per group
    assert _bad(sdk, setter(channels=8192, c_split=8192, groups=1), nch=(4, 0), apply=False)   # ... from partials too
    assert _bad(sdk, setter(ld0=60))                                # ld % 8
    assert _bad(sdk, setter(ld1=20), c_split=32)
    assert _bad(sdk, setter(src1=None), c_split=32)                 # concat without src1
    assert _bad(sdk, nop, H=16, W=15)                               # h*w != hw
    assert _bad(sdk, nop, H=0, W=0)
    assert _bad(sdk, nop, pad=5)
    assert _bad(sdk, nop, pad=-1)
    assert _bad(sdk, nop, nch=(5, 0))                               # chunks must divide hw
    assert _bad(sdk, nop, nch=(-1, 0))
    assert _bad(sdk, nop, nch=(4, 5), c_split=32)
    # more than 4096 channels: only the single-launch form takes them (hw <= 64), the statistics pass does not
    from sd_amd import _lib
    a = _args(_lib, 1, 8, 8, 8192)
    assert _plan(sdk, a, 8, 8, 1)[:2] == (0, (SLICE, IN_STATS, 1))
    assert _plan(sdk, a, 8, 8, 1, single=False)[0] != 0
    assert _plan(sdk, a, 8, 8, 1, apply=False)[0] != 0
    assert sdk.library().sdk_group_norm_plan(None, 1, 1, 8, 8, 1, 0, 0, 1, C.byref(_lib.GroupNormPlanInfo())) != 0
    assert sdk.library().sdk_group_norm_plan(C.byref(a), 1, 1, 8, 8, 1, 0, 0, 1, None) != 0
