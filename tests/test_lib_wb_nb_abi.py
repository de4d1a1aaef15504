"""The wideband noise blanker's C entry points: header, binding and Makefile agree; what needs no ctx (NULL-ctx returns,
ssdr_wb_nb_gate_samples) runs anywhere.  The rules of a live ctx are in tests/test_gpu_wb_nb.py."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
import wb_nb_ref as R  # noqa: E402

NAMES = ("ssdr_set_wb_noise_blanker", "ssdr_get_wb_noise_blanker", "ssdr_wb_nb_gate_samples", "ssdr_wb_nb_mask", "ssdr_wb_nb_counts",
         "ssdr_get_wb_nb_state", "ssdr_wb_nb_stats")


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def test_header_binding_and_makefile_agree(S):
    from supersdr_amd import _lib as L
    from supersdr_amd.iqstream import Channelizer
    src = open(os.path.join(ROOT, "include", "ssdr.h")).read()
    assert "#define SSDR_WB_NB_BLOCK 4096" in src and L.WB_NB_BLOCK == 4096 == Channelizer.NB_BLOCK == R.W
    assert "SSDR_K_SQUELCH = 11, SSDR_K_COUNT = 12" in src           # the stage has no SSDR_K_* slot: its stats are its own
    for name in NAMES:
        assert hasattr(L.lib, name) and name in L.EXPORTS
        proto = re.search(r"int %s\((.*?)\);" % name, src, re.S)
        assert proto, name
        n_args = len([a for a in re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S).split(",") if a.strip()])
        assert n_args == len(L._SIGS[name][1]), name
    srcs = re.search(r"^SRCS = (.*)$", open(os.path.join(ROOT, "supersdr_amd", "csrc", "Makefile")).read(), re.M).group(1).split()
    assert "ssdr_wb_nb.hip" in srcs and "ssdr_api_wbnb.cpp" in srcs
    for m in ("set_wb_noise_blanker", "get_wb_noise_blanker", "wb_nb_mask", "wb_nb_counts", "wb_nb_state", "wb_nb_stats"):
        assert callable(getattr(S.SsdrEngine, m))


def test_null_ctx(S):
    from supersdr_amd import _lib as L
    g, t = np.array([37], np.uint32), np.array([20], np.uint32)
    n, ms = C.c_uint32(), C.c_float()
    out = np.zeros(64, np.uint64)
    assert L.lib.ssdr_set_wb_noise_blanker(None, 0, 1, g.ctypes.data, t.ctypes.data) == L.EINVAL
    assert L.lib.ssdr_get_wb_noise_blanker(None, g.ctypes.data, t.ctypes.data, C.byref(n)) == L.EINVAL
    assert L.lib.ssdr_wb_nb_mask(None, out.ctypes.data, 0) == L.EINVAL
    assert L.lib.ssdr_wb_nb_counts(None, out.ctypes.data, None) == L.EINVAL
    assert L.lib.ssdr_get_wb_nb_state(None, g.ctypes.data, None, None) == L.EINVAL
    assert L.lib.ssdr_wb_nb_stats(None, C.byref(ms), C.byref(n), 0) == L.EINVAL
    assert (g[0], t[0]) == (37, 20)


def test_gate_samples_values_and_refusals(S):
    from supersdr_amd import _lib as L
    from supersdr_amd.iqstream import Channelizer
    ch = Channelizer(1, 2)
    g = C.c_uint32(77)
    rng = np.random.default_rng(26)
    rates = (12.288e6, 20250.0 * 512, 20250.0 * 1024, 6.144e6, 48e3)
    for rate in rates:
        for us in [0.01, 1.0, 3.0, 100.0, 4096 / 12.288, 4096e6 / rate] + list(rng.uniform(0.05, 4000e6 / rate, 40)):
            want = int(np.ceil(float(us) * float(rate) / 1e6))
            if 1 <= want <= 4096:
                assert L.lib.ssdr_wb_nb_gate_samples(us, rate, C.byref(g)) == L.OK and g.value == want, (us, rate)
                assert ch.nb_gate_samples(us, rate) == want == R.gate_samples(us, rate)
            else:
                g.value = 77
                assert L.lib.ssdr_wb_nb_gate_samples(us, rate, C.byref(g)) == L.EINVAL and g.value == 77, (us, rate)
    g.value = 77
    for us, rate in ((0.0, 12.288e6), (-1.0, 12.288e6), (333.4, 12.288e6), (1e12, 12.288e6), (float("nan"), 12.288e6), (float("inf"), 12.288e6),
                     (3.0, 0.0), (3.0, -12.288e6), (3.0, float("nan")), (3.0, float("inf"))):
        assert L.lib.ssdr_wb_nb_gate_samples(us, rate, C.byref(g)) == L.EINVAL and g.value == 77, (us, rate)
        with pytest.raises(ValueError):
            ch.nb_gate_samples(us, rate)
    assert L.lib.ssdr_wb_nb_gate_samples(3.0, 12.288e6, None) == L.EINVAL
    assert L.lib.ssdr_wb_nb_gate_samples(3.0, 12.288e6, C.byref(g)) == L.OK and g.value == 37
