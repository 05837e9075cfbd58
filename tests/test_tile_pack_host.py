"""Host side of the packed tile operators (include/stair_hip.h: stair_set_tile_pack, stair_ctx_set_tile_pack,
stair_tile_pack_factor, stair_tile_work_items): how many instances share a 64-row tile, and where the switch lives.  No GPU."""
import ctypes as C

import pytest

from stair_amd._lib import lib, StairConfig


@pytest.fixture(autouse=True)
def default_switch():
    yield
    lib.stair_set_tile_pack(-1)


FACTORS = [(1, 64), (5, 12), (8, 8), (21, 3), (32, 2), (33, 1), (64, 1)]


def test_pack_factor_follows_the_process_wide_switch():
    for T, P in FACTORS:
        assert lib.stair_tile_pack_factor(T) == P, T
    assert lib.stair_set_tile_pack(0) == 0
    for T, _ in FACTORS:
        assert lib.stair_tile_pack_factor(T) == 1, T
    assert lib.stair_set_tile_pack(-1) == 0
    for T, P in FACTORS:
        assert lib.stair_tile_pack_factor(T) == P, T
    assert lib.stair_set_tile_pack(1) == 0 and lib.stair_tile_pack_factor(8) == 8


def test_context_override_is_per_context_and_inherits():
    cfg = StairConfig(512, 2048, 300, 172, 64, 36, 1)
    a, b = C.c_void_p(), C.c_void_p()
    assert lib.stair_ctx_create(C.byref(cfg), C.byref(a)) == 0 and lib.stair_ctx_create(C.byref(cfg), C.byref(b)) == 0
    try:
        v = C.c_int32(7)
        for h in (a, b):
            assert lib.stair_ctx_get_tile_pack(h, C.byref(v)) == 0 and v.value == -1
        assert lib.stair_ctx_set_tile_pack(a, 0) == 0
        assert lib.stair_ctx_get_tile_pack(a, C.byref(v)) == 0 and v.value == 0
        assert lib.stair_ctx_get_tile_pack(b, C.byref(v)) == 0 and v.value == -1            # the other context is untouched
        assert lib.stair_ctx_set_tile_pack(b, 1) == 0 and lib.stair_ctx_get_tile_pack(b, C.byref(v)) == 0 and v.value == 1
        assert lib.stair_ctx_get_tile_pack(a, C.byref(v)) == 0 and v.value == 0
        assert lib.stair_ctx_set_tile_pack(a, -5) == 0 and lib.stair_ctx_get_tile_pack(a, C.byref(v)) == 0 and v.value == -1
        # the override is not one of the numbered options: their table is as long as it was
        assert lib.stair_ctx_set_option(a, 5, 1) != 0 and b'unknown option' in lib.stair_last_error()
        # a context's override does not move the process-wide factor
        assert lib.stair_tile_pack_factor(8) == 8
        assert lib.stair_ctx_set_tile_pack(None, 1) != 0 and lib.stair_ctx_get_tile_pack(a, None) != 0
    finally:
        lib.stair_ctx_destroy(a); lib.stair_ctx_destroy(b)


def test_work_item_counter_reads_and_resets_without_a_device():
    n = C.c_int64(-1)
    assert lib.stair_tile_work_items(C.byref(n), 1) == 0 and n.value >= 0
    assert lib.stair_tile_work_items(C.byref(n), 0) == 0 and n.value == 0
    assert lib.stair_tile_work_items(None, 0) == 0
