"""The noise blanker's control plane on CPU: "SET nb=<gate_us> th=<thresh>" through GpuStream and IQHub.

The GPU engine is the twin-backed test double of tests/test_host_workers.py, extended by a set_noise_blanker that applies
nb_ref's blank() to its channels' audio input (the waterfall keeps the input as it came), so the PCM a client receives must be
the twin's on blank(X)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nb_ref as NB  # noqa: E402
import refload  # noqa: E402
import twinlib  # noqa: E402
from test_host_workers import TwinEngine  # noqa: E402


class NbTwinEngine(TwinEngine):
    def __init__(self, n_ch):
        super().__init__(n_ch)
        self.nb_calls = []
        self.gate = np.zeros(n_ch, np.int64)
        self.th = np.zeros(n_ch, np.int64)
        self.nb_state = [NB.State() for _ in range(n_ch)]

    def set_noise_blanker(self, first, gate_us, thresh):
        for i, (g, t) in enumerate(zip(gate_us, thresh)):
            c = first + i
            self.nb_calls.append((c, int(g), int(t)))
            on = g != 0 and t != 0
            self.gate[c] = NB.gate_samples(int(g), 1, getattr(self, "kiwi_rate", 12000)) if on else 0
            self.th[c] = t if on else 0
            self.nb_state[c] = NB.State()

    def run_audio(self):
        plain = self.iq
        self.iq = NB.blank_all(plain, self.gate, self.th, 1, self.nb_state)[0]
        try:
            return super().run_audio()
        finally:
            self.iq = plain


def expected_pcm(X, gates, ths, params):
    """the twin's PCM on blank(X), all in one run (the hub's frames come in order, the twin's state carries across them)"""
    import supersdr_amd as S
    n_ch = X.shape[0]
    consts = np.zeros(n_ch, twinlib.CONSTS_DTYPE)
    taps = np.zeros((n_ch, 128), np.float32)
    for c in range(n_ch):
        consts[c], taps[c] = S.compile_params(params[c])
    st, hist = twinlib.fresh_state(consts)
    Xb, m = NB.blank_all(X, gates, ths, 1)
    return twinlib.load().audio(Xb, consts, taps, st, hist)[0], m


def synth(n_ch, n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = np.stack([2000 * np.cos(0.11 * t) + rng.normal(0, 300, n), 2000 * np.sin(0.11 * t) + rng.normal(0, 300, n)], -1)
    x = np.repeat(x[None], n_ch, 0)
    for s in range(1500, n, 613):
        x[:, s] = (32767, -30000)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def run_hub(engine, X, msgs, channel=1):
    from supersdr_amd.workers import GpuStream, IQHub
    n_ch, n = X.shape[0], X.shape[1]
    hub = IQHub(n_ch, engine=engine, gpu_post=False)
    stream = GpuStream(hub, channel, "SND", 7100.0)
    for m in msgs:
        stream.send_message(m)
    for k in range(n // 1024):
        for c in range(n_ch):
            hub.feed(c, X[c, k * 1024:(k + 1) * 1024])
    frames = [np.concatenate([np.asarray(hub.snd_queue[c].get_nowait()) for _ in range(n // 512)]) for c in range(n_ch)]
    hub.close()
    return np.stack(frames), stream


def test_set_nb_through_gpustream_gives_the_twin_on_blank_x():
    import supersdr_amd as S
    n_ch, n = 3, 12 * 1024
    X = synth(n_ch, n, 1)
    eng = NbTwinEngine(n_ch)
    pcm, _ = run_hub(eng, X, ["SET nb=100 th=20", "SET squelch=1 max=3", "SET nb algo=1", "SET keepalive"])
    assert eng.nb_calls == [(1, 100, 20)]                    # squelch and the newer "nb algo=" interface are accepted and ignored
    want, m = expected_pcm(X, [0, NB.gate_samples(100), 0], [0, 20, 0], [S.default_params("am")] * n_ch)
    assert m[1].any() and not m[[0, 2]].any()
    assert np.array_equal(pcm, want)
    plain, _ = expected_pcm(X, [0, 0, 0], [0, 0, 0], [S.default_params("am")] * n_ch)
    assert not np.array_equal(pcm[1], plain[1]) and np.array_equal(pcm[0], plain[0])


def test_set_nb_off_and_bad_values():
    from supersdr_amd.workers import GpuStream, IQHub
    eng = NbTwinEngine(2)
    hub = IQHub(2, engine=eng, gpu_post=False)
    s = GpuStream(hub, 0, "SND", 7100.0)
    s.send_message(b"SET nb=500 th=10")
    s.send_message("SET nb=0 th=10")                         # 0 = off
    for bad in ("SET nb=20000 th=20", "SET nb=100 th=1", "SET nb=100 th=5000", "SET nb=-5 th=20", "SET nb=100", "SET nb=x th=2"):
        with pytest.raises(ValueError):
            s.send_message(bad)
    assert eng.nb_calls == [(0, 500, 10), (0, 0, 10)]
    assert eng.th[0] == 0 and eng.gate[0] == 0
    with pytest.raises(ValueError):
        hub.set_noise_blanker(1, 10001, 20)
    assert len(eng.nb_calls) == 2
    hub.close()


def test_hub_without_a_blanker_in_its_engine_still_runs():
    """an engine double without set_noise_blanker keeps working as long as nobody asks for the blanker"""
    from supersdr_amd.workers import GpuStream, IQHub
    hub = IQHub(2, engine=TwinEngine(2), gpu_post=False)
    s = GpuStream(hub, 0, "SND", 7100.0)
    s.send_message("SET mod=usb low_cut=300 high_cut=2700 freq=7101.000")
    s.send_message("SET squelch=0 max=0")
    X = synth(2, 2048, 3)
    for c in range(2):
        hub.feed(c, X[c])
    assert hub.snd_queue[0].qsize() == 4
    hub.close()


@pytest.mark.skipif(not refload.available(), reason="the reference (kiwi/client.py) is not on this box")
def test_the_references_own_set_noise_blanker_drives_the_gpustream():
    """kiwi/client.py's KiwiSDRStream.set_noise_blanker / set_squelch, the reference's own code, talking to a GpuStream"""
    import supersdr_amd as S
    from supersdr_amd.workers import GpuStream, IQHub
    _, _, KC = refload.load()
    n_ch, n = 2, 8 * 1024
    X = synth(n_ch, n, 4)
    eng = NbTwinEngine(n_ch)
    hub = IQHub(n_ch, engine=eng, gpu_post=False)
    kiwi = KC.KiwiSDRStream.__new__(KC.KiwiSDRStream)
    KC.KiwiSDRStreamBase.__init__(kiwi)
    kiwi._stream_name = "SND"
    kiwi._stream = GpuStream(hub, 1, "SND", 7100.0)
    kiwi.set_noise_blanker(250, 15)
    kiwi.set_squelch(1, 10)
    assert eng.nb_calls == [(1, 250, 15)]
    with pytest.raises(ValueError):
        kiwi.set_noise_blanker(250, 1)
    for k in range(n // 1024):
        for c in range(n_ch):
            hub.feed(c, X[c, k * 1024:(k + 1) * 1024])
    pcm = np.stack([np.concatenate([np.asarray(hub.snd_queue[c].get_nowait()) for _ in range(n // 512)]) for c in range(n_ch)])
    hub.close()
    want, m = expected_pcm(X, [0, NB.gate_samples(250)], [0, 15], [S.default_params("am")] * n_ch)
    assert m[1].any() and np.array_equal(pcm, want)
