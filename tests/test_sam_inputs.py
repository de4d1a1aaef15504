"""The synchronous-AM GPU cases (tests/sam_cases.py) audited against the definition alone, without a GPU: they must be inputs on
which a single-precision chain CAN be held to the float64 definition.

  * the loop's largest phase error stays under 2.5 rad in every case: no cycle slip (a slip is a branch cut of the arctangent where
    fp32 and float64 may part ways for good) -- hence offsets within +-150 Hz and carriers 45 dB over the noise;
  * no output sample clips;
  * a float32 emulation of the whole chain (complex64 mixer and FIR sums, float32 loop and DC estimate: sam_ref's fp32=True) stays
    under HALF of tests.tolerances.PCM_RMS_TOL against the definition on every case channel.  Measured here: largest RMS
    1.9e-6 of full scale (12 kHz) and 2.3e-6 (20.25 kHz), largest sample difference 1 LSB; if a case fails the half, the case
    changes, not the cap."""
import numpy as np
import pytest

import sam_cases as SC
from tolerances import PCM_RMS_TOL


@pytest.mark.parametrize("n_ch,rate", SC.SHAPES)
def test_no_cycle_slip_no_clipping_and_the_rows_are_what_they_say(n_ch, rate):
    ref = SC.reference(n_ch, rate)
    rows = SC.sam_rows(n_ch)
    assert rows and 0 not in rows and n_ch - 1 not in rows                     # SAM rows sit between rows of the other modes
    assert all(not SC.is_sam(c - 1) and not SC.is_sam(c + 1) for c in rows)
    assert {SC.name_of(c) for c in rows} == {"sam", "sal", "sau"}
    worst_e = max(np.abs(ref[c][2]).max() for c in rows)
    print("%d channels at %d Hz: %d SAM rows, largest |e| %.2f rad" % (n_ch, rate, len(rows), worst_e))
    assert worst_e < 2.5
    for c in rows:
        pcm, rssi, e, car = ref[c]
        assert np.abs(pcm.astype(np.int32)).max() < 32767, c
        assert np.abs(pcm.astype(np.int32)).max() > 1000, c                       # and it is not silence
        assert abs(SC.offset(c)) <= 150.0
        # two-sided rows read their offset; one-sided ones wander around it (a carrier with one sideband is phase-modulated)
        tol = 0.5 if SC.name_of(c) == "sam" else 8.0
        assert abs(car[-1, 0] - SC.offset(c)) < tol, (c, car[-1, 0], SC.offset(c))


@pytest.mark.parametrize("n_ch,rate", SC.SHAPES)
def test_a_float32_chain_stays_under_half_the_pcm_tolerance(n_ch, rate):
    ref, emu = SC.reference(n_ch, rate), SC.reference(n_ch, rate, fp32=True)
    rms, lsb, hz, ph = [], [], [], []
    for c in SC.sam_rows(n_ch):
        d = ref[c][0].astype(np.float64) - emu[c][0].astype(np.float64)
        rms.append(np.sqrt((d ** 2).mean()) / 32768.0)
        lsb.append(np.abs(d).max())
        hz.append(np.abs(ref[c][3][:, 0] - emu[c][3][:, 0]).max())
        ph.append(SC.phase_diff(ref[c][3][:, 1], emu[c][3][:, 1]).max())
    print("%d channels at %d Hz, float32 emulation against the definition: largest RMS %.2e of full scale, largest sample difference %d LSB, "
          "carrier read-back within %.1e Hz and %.1e rad" % (n_ch, rate, max(rms), max(lsb), max(hz), max(ph)))
    assert max(rms) < 0.5 * PCM_RMS_TOL
