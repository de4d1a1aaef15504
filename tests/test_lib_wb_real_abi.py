"""The real-sample front end's C entry points: header, binding and Makefile agree; what needs no ctx (NULL-ctx returns, ssdr_wb_real_taps,
the Channelizer's helpers) runs anywhere.  The rules of a live ctx are in tests/test_gpu_wb_real.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import wb_real_ref as R  # noqa: E402

NAMES = ("ssdr_wb_real_taps", "ssdr_set_wb_real_zone", "ssdr_get_wb_real_zone", "ssdr_push_wideband_real", "ssdr_read_wb_real",
         "ssdr_get_wb_real_state", "ssdr_wb_real_stats")


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def test_header_binding_and_makefile_agree(S):
    from supersdr_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    assert "#define SSDR_WB_REAL_TAPS 103" in src and L.WB_REAL_TAPS == 103 == R.N
    assert "SSDR_K_SQUELCH = 11, SSDR_K_COUNT = 12" in src           # the stage has no SSDR_K_* slot: its stats are its own
    for name in NAMES:
        assert hasattr(L.lib, name) and name in L.EXPORTS
        proto = re.search(r"int %s\((.*?)\);" % name, src, re.S)
        assert proto, name
        n_args = len([a for a in re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S).split(",") if a.strip()])
        assert n_args == len(L._SIGS[name][1]), name
    make = open(os.path.join(ROOT, "supersdr_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", make, re.M).group(1).split()
    hdrs = re.search(r"^HDRS = (.*)$", make, re.M).group(1).split()
    assert "ssdr_wb_real.hip" in srcs and "ssdr_api_wbreal.cpp" in srcs and "ssdr_wb_real_taps.h" in hdrs
    for m in ("wb_real_taps", "set_wb_real_zone", "get_wb_real_zone", "push_wideband_real", "push_wideband_real_device", "read_wb_real",
              "wb_real_state", "wb_real_stats"):
        assert callable(getattr(S.SsdrEngine, m))
    from supersdr_amd.workers import IQHub
    for m in ("feed_wideband_real", "set_wideband_zone", "wideband_zone"):
        assert callable(getattr(IQHub, m))


def test_null_ctx(S):
    from supersdr_amd import _lib as L
    z, x = np.array([1], np.uint32), np.zeros(64, np.int16)
    n, ms, idx = C.c_uint32(), C.c_float(), C.c_uint64()
    assert L.lib.ssdr_set_wb_real_zone(None, 0, 1, z.ctypes.data) == L.EINVAL
    assert L.lib.ssdr_get_wb_real_zone(None, z.ctypes.data, C.byref(n)) == L.EINVAL
    assert L.lib.ssdr_push_wideband_real(None, x.ctypes.data, 1, 0) == L.EINVAL
    assert L.lib.ssdr_read_wb_real(None, x.ctypes.data, 0) == L.EINVAL
    assert L.lib.ssdr_get_wb_real_state(None, x.ctypes.data, C.byref(idx)) == L.EINVAL
    assert L.lib.ssdr_wb_real_stats(None, C.byref(ms), C.byref(n), 0) == L.EINVAL
    assert L.lib.ssdr_wb_real_taps(None) == L.EINVAL
    assert z[0] == 1 and not x.any()


def test_the_librarys_table_is_the_references(S):
    q = S.SsdrEngine.wb_real_taps()
    assert q.dtype == np.int32 and q.shape == (103,) and np.array_equal(q, R.Q)


def test_channelizer_helpers_values_and_refusals():
    from supersdr_amd.iqstream import Channelizer
    ch = Channelizer(2, 2)
    F = 6.144e6
    assert ch.real_rate(F) == 12.288e6 and ch.REAL_USABLE == 0.45
    # zone 0: RF 0 .. F, the stream's centre at F / 2; row r is centred on r * F / 1024
    assert ch.real_offset_of(F / 2, F, 0) == 0.0 and ch.real_offset_of(0.0, F, 0) == -F / 2
    assert ch.real_offset_of(1.5e6, F) == 1.5e6 - F / 2
    for r in (0, 1, 52, 511, 512, 700, 972, 1023):
        assert ch.real_row_of(r * F / 1024, F, 0) == (r, 0.0)
        assert ch.real_row_of(F + r * F / 1024, F, 1) == (r, 0.0)       # zone 1: row r is centred on F + r * F / 1024 -- not mirrored
        assert ch.real_usable(r * F / 1024, F, 0) == ch.real_usable(F + r * F / 1024, F, 1) == (52 <= r <= 972)
    row, res = ch.real_row_of(700 * F / 1024 + 1234.5, F, 0)
    assert row == 700 and res == pytest.approx(1234.5, abs=1e-6) and ch.real_row_of(700 * F / 1024 + 1234.5, F, 0) == ch.row_of(ch.real_offset_of(700 * F / 1024 + 1234.5, F, 0), F)
    # zone 1: RF F .. 2F, the stream's centre at 3F / 2
    assert ch.real_offset_of(1.5 * F, F, 1) == 0.0 and ch.real_offset_of(F, F, 1) == -F / 2
    # the usable band: within 0.45 F of the centre
    assert ch.real_usable(0.05 * F + 1.0, F, 0) and not ch.real_usable(0.05 * F - 1.0, F, 0)
    assert ch.real_usable(0.95 * F - 1.0, F, 0) and not ch.real_usable(0.95 * F + 1.0, F, 0)
    assert ch.real_usable(1.5 * F, F, 1) and not ch.real_usable(1.96 * F, F, 1) and not ch.real_usable(1.04 * F, F, 1)
    assert ch.real_usable(0.5 * F, F, 1) is False and ch.real_usable(1.5 * F, F, 0) is False and ch.real_usable(-1.0, F, 0) is False
    # outside the zone, and a zone that is none
    for rf, zone in ((-1.0, 0), (F, 0), (2 * F, 0), (F - 1.0, 1), (2 * F, 1), (0.0, 1), (float("nan"), 0)):
        with pytest.raises(ValueError):
            ch.real_offset_of(rf, F, zone)
        with pytest.raises(ValueError):
            ch.real_row_of(rf, F, zone)
    for zone in (2, -1, 0.5, None):
        with pytest.raises(ValueError):
            ch.real_offset_of(F / 2, F, zone)
        with pytest.raises(ValueError):
            ch.real_usable(F / 2, F, zone)
