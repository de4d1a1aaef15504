"""The IMA-ADPCM encoder's definition (tests/adpcm_ref.py) against the decoder the wire contract is fixed by: the known answer,
and encoder and decoder in lockstep -- same state after every chunk, the decoder's samples the encoder's reconstruction -- over
random streams and the inputs that drive the clamps.  Where the reference is on the box, its own ImaAdpcmDecoder agrees."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import adpcm_ref as A  # noqa: E402
import refload  # noqa: E402
import ssdr_oracle as O  # noqa: E402


def test_known_answer():
    out, rec, st = A.encode([100, 100])
    assert out.tolist() == [0x77]
    assert rec.tolist() == [11, 41]
    assert st.tolist() == [16, 41]
    dec, idx, prev = O.ima_adpcm_decode(bytes(out))
    assert dec.tolist() == [11, 41] and (idx, prev) == (16, 41)


def test_tables_are_the_decoders():
    assert tuple(A.STEP.tolist()) == O.IMA_STEP and tuple(A.ADJ.tolist()) == O.IMA_ADJ


def lockstep(x, chunk):
    """encode x [n_streams, m] chunk by chunk with the state carried; decode every stream's bytes with the oracle's decoder, its
    state carried too: the states agree after every chunk and the decoded samples are the reconstruction"""
    n, m = x.shape
    st = np.zeros((n, 2), np.int32)
    dst = [(0, 0)] * n
    for lo in range(0, m, chunk):
        out, rec, st = A.encode(x[:, lo:lo + chunk], st)
        for k in range(n):
            dec, idx, prev = O.ima_adpcm_decode(bytes(out[k]), *dst[k])
            dst[k] = (idx, prev)
            assert np.array_equal(dec, rec[k]), (k, lo)
            assert (idx, prev) == tuple(st[k].tolist()), (k, lo)
    return st


def test_lockstep_gaussian_streams():
    rng = np.random.default_rng(11)
    x = np.clip(np.rint(rng.normal(0, [[300], [3000], [12000]], (3, 4096))), -32768, 32767).astype(np.int16)
    lockstep(x, 512)
    lockstep(x, 2)


def test_lockstep_edge_inputs():
    m = 2048
    silence = np.zeros(m, np.int16)
    square = np.where(np.arange(m) % 2, -32768, 32767).astype(np.int16)         # full scale, every sample
    slow_square = np.where((np.arange(m) // 32) % 2, -32768, 32767).astype(np.int16)   # long enough to reach both sample clamps
    step_up = square.copy()                                                      # pins the index at 88 ...
    step_up[m // 2:] = 0                                                         # ... then a long run back down to 0
    x = np.stack([silence, square, slow_square, step_up])
    lockstep(x, 512)
    for sq in (square, slow_square):
        _, rec, st = A.encode(sq)
        assert rec.min() == -32768
    assert A.encode(slow_square)[1].max() == 32767
    # the index reaches 88, and after the signal settles it walks back to 0
    idx = []
    s = np.zeros(2, np.int32)
    for lo in range(0, m, 2):
        _, _, s = A.encode(step_up[lo:lo + 2], s)
        idx.append(int(s[0]))
    assert idx[m // 4 - 1] == 88 and idx[-1] == 0
    out, rec, st = A.encode(silence)
    assert (np.abs(rec) <= 1).all() and st[0] == 0


def test_wf_line_format():
    rng = np.random.default_rng(3)
    line = np.clip(np.rint(rng.normal(135, 8, 1024)), 0, 255).astype(np.int64)
    enc = A.encode_wf_lines(line[None])
    assert enc.shape == (1, A.WF_BYTES) == (1, 517)
    dec, _, _ = O.ima_adpcm_decode(bytes(enc[0]))
    assert dec.shape == (1034,)
    _, rec, _ = A.encode(np.concatenate([line, np.repeat(line[-1:], 10)]))
    assert np.array_equal(dec, rec)
    err = np.abs(dec[:1024].astype(np.int64) - line)
    assert err[12:].max() <= 32                  # lossy, but it tracks the line once the step has grown to its level


def test_argument_errors():
    with pytest.raises(ValueError):
        A.encode([1, 2, 3])
    with pytest.raises(ValueError):
        A.encode([1, 2], [89, 0])
    with pytest.raises(ValueError):
        A.encode([1, 2], [0, 40000])


@pytest.mark.skipif(not refload.available(), reason="the reference is not on this box")
def test_reference_decoder_agrees():
    KC = refload.load()[2]
    rng = np.random.default_rng(5)
    x = np.clip(np.rint(rng.normal(0, 4000, (2, 2048))), -32768, 32767).astype(np.int16)
    x[1, ::2], x[1, 1::2] = 32767, -32768
    for k in range(2):
        d = KC.ImaAdpcmDecoder()
        st = np.zeros(2, np.int32)
        for lo in range(0, 2048, 512):
            out, rec, st = A.encode(x[k, lo:lo + 512], st)
            got = np.array(d.decode(bytes(out)), np.int16)
            assert np.array_equal(got, rec)
            assert (d.index, d.prev) == tuple(st.tolist())
    d = KC.ImaAdpcmDecoder()
    assert list(d.decode(bytes(A.encode([100, 100])[0]))) == [11, 41] and (d.index, d.prev) == (16, 41)
