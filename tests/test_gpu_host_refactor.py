"""What the shared helpers of the C API's host code (csrc/ssdr_api.cpp) must keep as it was, pinned on the GPU: the seven
stage timers beside the SSDR_K_* slots are independent of each other and of those slots, and the two entry points that change
the input rate keep their own order of refusals although they share one body (change_input_rate)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chan_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import supersdr_amd
    return supersdr_amd


def test_stage_timers_are_independent(S):
    """de-emphasis, views, sub-receivers, channeliser, scopes, the tuned receivers' DDC and their audio: each counts its own launches
    (with or without profiling), keeps its own time (with profiling only), and a reset of one -- the tuned receivers' two go together
    -- touches neither the others nor an SSDR_K_* slot"""
    from supersdr_amd import _lib as L
    with S.SsdrEngine(1024) as eng:                      # the channeliser's minimum: one stream
        eng.set_profiling(True)
        eng.set_channelizer(1, 1, K.proto(1, 1, 2.0))
        eng.set_wb_scopes([(0, 0, 0.0)])
        eng.set_wf_views([(0, 2, 0.0)])
        eng.set_subrx([(1, 0, S.default_params("am"))])
        eng.set_deemphasis(0, [(1, 0)])                  # channel 0 is in AM: the setting acts
        eng.set_wb_rx([(1, 0, 0.0, S.default_params("am"))])

        def wb_rx(k):                                    # the tuned receivers' two timers, which ssdr_wb_rx_stats reads and resets together
            def stats(reset=False):
                got = eng.wb_rx_stats(reset=reset)
                return got[k], got[2 + k]
            return stats
        together = {"wbrx_ddc", "wbrx_audio"}
        stages = {"deemp": eng.deemp_stats, "view": eng.wf_view_stats, "subrx": eng.subrx_stats,
                  "chan": eng.channelizer_stats, "scope": eng.wb_scope_stats, "wbrx_ddc": wb_rx(0), "wbrx_audio": wb_rx(1)}
        n_slots = 0                                      # SSDR_K_COUNT, asked of the library: the first `which` it refuses
        while L.lib.ssdr_kernel_stats(eng._ctx, n_slots, None, None, 0) == L.OK:
            n_slots += 1
        assert n_slots > L.K_SQUELCH
        slots = lambda: [eng.kernel_stats(k) for k in range(n_slots)]       # noqa: E731
        for name, stats in stages.items():
            assert stats() == (0.0, 0), name
        k0 = slots()
        iq = K.wideband(1, K.n_in(2, 1, 1), 7)
        eng.push_wideband(iq)
        eng.run_chain()
        eng.sync()
        # the launch counts of the commit before the helpers (one push, one chain run: one launch of every stage)
        want = {"deemp": 1, "view": 1, "subrx": 1, "chan": 1, "scope": 1, "wbrx_ddc": 1, "wbrx_audio": 1}
        for name, stats in stages.items():
            ms, n = stats()
            print(name, ms, n)
            assert n == want[name] and ms > 0.0, (name, ms, n)
        k1 = slots()
        assert k1 != k0 and k1[L.K_WF][1] == 1 and k1[L.K_AUDIO][1] == 1
        for name, stats in stages.items():               # a reset of one: that one is zero, nobody else moved
            before = {m: s() for m, s in stages.items()}
            assert stats(reset=True) == before[name]
            after = {m: s() for m, s in stages.items()}
            for gone in (together if name in together else {name}):
                assert after.pop(gone) == (0.0, 0)
                before.pop(gone)
            assert after == before, name
            assert slots() == k1, name
        eng.set_profiling(False)
        eng.push_wideband(iq)
        eng.run_chain()
        eng.sync()
        for name, stats in stages.items():               # launches are counted without profiling, time is not
            assert stats() == (0.0, 1), name
        assert slots() == k1
        eng.push_wideband(iq)                            # the DDC counts a launch per push, the receivers' audio one per run
        eng.sync()
        assert stages["wbrx_ddc"]() == (0.0, 2) and stages["wbrx_audio"]() == (0.0, 1) and stages["subrx"]() == (0.0, 1)


def test_rate_changes_keep_their_own_refusal_order(S):
    """ssdr_set_decimation refuses an open feed before it accepts the current value, ssdr_set_kiwi_rate accepts the current value
    first; only the decimation refuses while a channel is in synchronous AM"""
    from supersdr_amd import _lib as L
    lib = L.lib

    def config(eng):
        v = [C.c_uint32() for _ in range(4)]
        assert lib.ssdr_get_config(eng._ctx, *[C.byref(x) for x in v]) == L.OK
        return tuple(x.value for x in v)                 # hop, decim, averaging, kiwi_rate

    with S.SsdrEngine(2) as eng:
        eng.feed_open(2)                                 # (the shortest batch a feed takes: a whole line)
        assert lib.ssdr_set_decimation(eng._ctx, 1) == L.ESTATE
        assert lib.ssdr_set_kiwi_rate(eng._ctx, 12000) == L.OK
        assert lib.ssdr_set_decimation(eng._ctx, 2) == L.ESTATE
        assert lib.ssdr_set_kiwi_rate(eng._ctx, 20250) == L.ESTATE
        eng.feed_close()
        eng.set_params(0, [S.default_params("sam")])
        before = config(eng)
        assert before == (1024, 1, 1, 12000)
        assert lib.ssdr_set_decimation(eng._ctx, 2) == L.ESTATE
        assert config(eng) == before
        assert lib.ssdr_set_kiwi_rate(eng._ctx, 20250) == L.OK
        assert config(eng) == (1024, 1, 1, 20250)
