"""Host side of the segmented tile operators (include/stair_hip.h: stair_set_tile_split, stair_ctx_set_tile_split,
stair_tile_segments): how many 64-row segments a clip of T frames runs as, and where the switch lives.  No GPU."""
import ctypes as C

import pytest

from stair_amd._lib import lib, StairConfig


@pytest.fixture(autouse=True)
def default_switch():
    yield
    lib.stair_set_tile_split(-1)


SEGMENTS = [(1, 1), (32, 1), (64, 1), (65, 2), (128, 2), (129, 3), (141, 3)]


def test_segments_follow_the_process_wide_switch():
    for T, S in SEGMENTS:                       # default: on
        assert lib.stair_tile_segments(T) == S, T
    assert lib.stair_set_tile_split(0) == 0
    for T, _ in SEGMENTS:
        assert lib.stair_tile_segments(T) == 1, T
    assert lib.stair_set_tile_split(1) == 0
    for T, S in SEGMENTS:
        assert lib.stair_tile_segments(T) == S, T
    assert lib.stair_set_tile_split(0) == 0 and lib.stair_set_tile_split(-1) == 0
    for T, S in SEGMENTS:
        assert lib.stair_tile_segments(T) == S, T


def test_context_override_is_per_context_and_inherits():
    cfg = StairConfig(512, 2048, 300, 172, 128, 36, 1)
    a, b = C.c_void_p(), C.c_void_p()
    assert lib.stair_ctx_create(C.byref(cfg), C.byref(a)) == 0 and lib.stair_ctx_create(C.byref(cfg), C.byref(b)) == 0
    try:
        v = C.c_int32(7)
        for h in (a, b):
            assert lib.stair_ctx_get_tile_split(h, C.byref(v)) == 0 and v.value == -1
        assert lib.stair_ctx_set_tile_split(a, 0) == 0
        assert lib.stair_ctx_get_tile_split(a, C.byref(v)) == 0 and v.value == 0
        assert lib.stair_ctx_get_tile_split(b, C.byref(v)) == 0 and v.value == -1           # the other context is untouched
        assert lib.stair_ctx_set_tile_split(b, 1) == 0 and lib.stair_ctx_get_tile_split(b, C.byref(v)) == 0 and v.value == 1
        assert lib.stair_ctx_get_tile_split(a, C.byref(v)) == 0 and v.value == 0
        assert lib.stair_ctx_set_tile_split(a, -5) == 0 and lib.stair_ctx_get_tile_split(a, C.byref(v)) == 0 and v.value == -1
        # the two tile switches of a context are independent of each other
        assert lib.stair_ctx_set_tile_split(a, 0) == 0
        assert lib.stair_ctx_get_tile_pack(a, C.byref(v)) == 0 and v.value == -1
        # the override is not one of the numbered options: their table is as long as it was
        assert lib.stair_ctx_set_option(a, 5, 1) != 0 and b'unknown option' in lib.stair_last_error()
        # a context's override does not move the process-wide figure
        assert lib.stair_tile_segments(100) == 2
        assert lib.stair_ctx_set_tile_split(None, 1) != 0 and lib.stair_ctx_get_tile_split(a, None) != 0
    finally:
        lib.stair_ctx_destroy(a); lib.stair_ctx_destroy(b)
