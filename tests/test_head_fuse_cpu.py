"""CPU: the Detect towers' fused-tail switch (modules.HEAD_FUSE, YOLOSOD_HEAD_FUSE) and the library's host-side routing
query and setter (yolosod_debug_conv3x3_head_fused / yolosod_debug_set_conv3x3_head_fuse)."""
import pytest

from yolosod_amd import _hip
from yolosod_amd.nn import modules as M


def test_switch_spellings():
    assert M._onoff_switch("YOLOSOD_HEAD_FUSE", "1") is True
    assert M._onoff_switch("YOLOSOD_HEAD_FUSE", " 0 ") is False
    for bad in ("", "on", "true", "2", "-1", "0,1"):
        with pytest.raises(ValueError, match="YOLOSOD_HEAD_FUSE"):
            M._onoff_switch("YOLOSOD_HEAD_FUSE", bad)
    assert M.HEAD_FUSE is (M.HEAD_FUSE_DEFAULT == "1")  # the default (no YOLOSOD_HEAD_FUSE in the test environment)
    assert M.HEAD_FUSE_DEFAULT in ("0", "1")


def test_query_follows_the_64_channel_group_rule():
    """Automatic: a level fuses when its 64 -> 64 launch runs in 64-channel groups (form field groups == 1)."""
    lib = _hip.load_library()
    assert lib.yolosod_debug_set_conv3x3_head_fuse(-1) == -1  # automatic is the default
    assert lib.yolosod_debug_conv3x3_head_fused(32, 160, 160)      # the bench: P2
    assert lib.yolosod_debug_conv3x3_head_fused(32, 80, 80)        # P3
    assert not lib.yolosod_debug_conv3x3_head_fused(32, 40, 40)    # P4: 32-channel groups
    assert not lib.yolosod_debug_conv3x3_head_fused(32, 20, 20)    # P5
    assert not lib.yolosod_debug_conv3x3_head_fused(2, 160, 160)   # the census tests' batch
    assert lib.yolosod_debug_conv3x3_head_fused(8, 320, 320) and lib.yolosod_debug_conv3x3_head_fused(8, 160, 160)
    assert not lib.yolosod_debug_conv3x3_head_fused(8, 80, 80)     # n1280 at batch 8: P2 and P3 only
    assert not lib.yolosod_debug_conv3x3_head_fused(32, 160, 162)  # W % 4 != 0: never
    for B, H, W in ((32, 160, 160), (32, 80, 80), (32, 40, 40), (32, 20, 20), (2, 160, 160), (8, 80, 80)):
        groups = lib.yolosod_debug_conv3x3_form(B, 64, H, W) >> 2
        assert bool(lib.yolosod_debug_conv3x3_head_fused(B, H, W)) == (groups == 1), (B, H, W)
    assert _hip.conv3x3_head_fused(32, 160, 160) and not _hip.conv3x3_head_fused(2, 160, 160)


def test_setter_returns_the_previous_value():
    lib = _hip.load_library()
    try:
        assert lib.yolosod_debug_set_conv3x3_head_fuse(1) == -1
        assert lib.yolosod_debug_conv3x3_head_fused(2, 8, 8)
        assert not lib.yolosod_debug_conv3x3_head_fused(2, 8, 6)
        assert lib.yolosod_debug_set_conv3x3_head_fuse(0) == 1
        assert not lib.yolosod_debug_conv3x3_head_fused(32, 160, 160)
        assert lib.yolosod_debug_set_conv3x3_head_fuse(7) == 0  # ignored
        assert lib.yolosod_debug_set_conv3x3_head_fuse(-1) == 0
    finally:
        lib.yolosod_debug_set_conv3x3_head_fuse(-1)


def test_prepared_block_sizes():
    lib = _hip.load_library()
    assert lib.yolosod_detect_head_prep_bytes(64) == 2 * 4 * 1024 * 2 + 256
    for nc in (1, 10, 16):
        assert lib.yolosod_detect_head_prep_bytes(nc) == 2 * 1024 * 2 + 256
    for bad in (0, 17, 32, 128):
        assert lib.yolosod_detect_head_prep_bytes(bad) == 0
