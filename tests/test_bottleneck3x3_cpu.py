"""CPU: the fused Bottleneck's switch (modules.BOTTLENECK_FUSE, YOLOSOD_BOTTLENECK_FUSE) and the library's host-side
routing query and setter (yolosod_debug_bottleneck3x3_fused / yolosod_debug_set_bottleneck3x3_fuse)."""
import pytest

from yolosod_amd import _hip
from yolosod_amd.nn import modules as M


def test_switch_spellings():
    assert M._onoff_switch("YOLOSOD_BOTTLENECK_FUSE", "1") is True
    assert M._onoff_switch("YOLOSOD_BOTTLENECK_FUSE", " 0 ") is False
    for bad in ("", "on", "true", "2", "-1", "0,1"):
        with pytest.raises(ValueError, match="YOLOSOD_BOTTLENECK_FUSE"):
            M._onoff_switch("YOLOSOD_BOTTLENECK_FUSE", bad)
    assert M.BOTTLENECK_FUSE is True  # the default


def test_query_routes_by_map_size():
    lib = _hip.load_library()
    assert lib.yolosod_debug_set_bottleneck3x3_fuse(-1) == -1  # automatic is the default
    assert not lib.yolosod_debug_bottleneck3x3_fused(2, 160, 160)   # 6.6 MB: the census tests' sizes
    assert not lib.yolosod_debug_bottleneck3x3_fused(2, 64, 64)
    assert lib.yolosod_debug_bottleneck3x3_fused(32, 160, 160)      # the bench, 105 MB
    assert lib.yolosod_debug_bottleneck3x3_fused(8, 320, 320)       # n1280
    assert not lib.yolosod_debug_bottleneck3x3_fused(32, 160, 162)  # W % 4 != 0: never
    assert not _hip.bottleneck3x3_fused(2, 64, 64) and _hip.bottleneck3x3_fused(32, 160, 160)


def test_setter_returns_the_previous_value():
    lib = _hip.load_library()
    try:
        assert lib.yolosod_debug_set_bottleneck3x3_fuse(1) == -1
        assert lib.yolosod_debug_bottleneck3x3_fused(2, 64, 64)
        assert not lib.yolosod_debug_bottleneck3x3_fused(2, 64, 62)
        assert lib.yolosod_debug_set_bottleneck3x3_fuse(0) == 1
        assert not lib.yolosod_debug_bottleneck3x3_fused(32, 160, 160)
        assert lib.yolosod_debug_set_bottleneck3x3_fuse(7) == 0  # ignored
        assert lib.yolosod_debug_set_bottleneck3x3_fuse(-1) == 0
    finally:
        lib.yolosod_debug_set_bottleneck3x3_fuse(-1)
