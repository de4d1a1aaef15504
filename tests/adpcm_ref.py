"""The IMA-ADPCM encoder of the compressed Kiwi wire formats, defined once, in NumPy.

The decoder on the client's end is fixed by the reference (kiwi/client.py:58-87, restated as ssdr_oracle.ima_adpcm_decode): an
89-entry step table, the index adjust table, low nibble first, diff = step>>3 (+step>>2, +step>>1, +step), clamps on the sample and
on the index.  The encoder is the standard IMA one, run in lockstep with that decoder -- per sample x, with step = T[index]:

    d = x - prev; code = 0
    if d < 0:           code = 8; d = -d
    if d >= step:       code |= 4; d -= step
    if d >= step >> 1:  code |= 2; d -= step >> 1
    if d >= step >> 2:  code |= 1
    prev, index = the decoder's own update for `code`

so both ends always hold the same (index, prev).  Vectorised across streams, serial along each stream.  The GPU encoder
(supersdr_amd/csrc/ssdr_adpcm_enc.hip) is held to this bit for bit.

Wire use: SND frames ("SET compression=1") are 512 samples -> 256 bytes with the state carried for the whole connection from (0, 0);
W/F lines ("SET wf_comp=1") are the 1024 byte values as samples 0..255 plus WF_PAD samples repeating the last one, encoded from (0, 0)
per line -> 517 bytes; the client decodes 1034 samples and keeps the first 1024 (kiwi/client.py:476-479)."""
import numpy as np

STEP = np.array((7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60,
                 66, 73, 80, 88, 97, 107, 118, 130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371,
                 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707,
                 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132,
                 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623,
                 27086, 29794, 32767), np.int64)
ADJ = np.array((-1, -1, -1, -1, 2, 4, 6, 8, -1, -1, -1, -1, 2, 4, 6, 8), np.int64)
WF_PAD = 10
WF_BYTES = (1024 + WF_PAD) // 2


def encode(pcm, state=None):
    """pcm int [n_streams, n_samples] (or [n_samples]), n_samples even; state int [n_streams, 2] {index, prev} or None for (0, 0)
    -> (uint8 [n_streams, n_samples // 2] low nibble first, the encoder's reconstruction int16 [n_streams, n_samples] -- what
    the decoder returns for those bytes --, the new state int32 [n_streams, 2])"""
    x = np.asarray(pcm, np.int64)
    one = x.ndim == 1
    if one:
        x = x[None]
    n, m = x.shape
    if m % 2:
        raise ValueError("an even number of samples per stream")
    st = np.zeros((n, 2), np.int64) if state is None else np.array(state, np.int64).reshape(n, 2)
    index, prev = st[:, 0].copy(), st[:, 1].copy()
    if ((index < 0) | (index > 88)).any() or ((prev < -32768) | (prev > 32767)).any():
        raise ValueError("state out of range")
    codes = np.empty((n, m), np.int64)
    rec = np.empty((n, m), np.int16)
    for i in range(m):
        step = STEP[index]
        d = x[:, i] - prev
        code = np.where(d < 0, 8, 0)
        d = np.abs(d)
        b = d >= step
        code |= np.where(b, 4, 0)
        d = d - np.where(b, step, 0)
        b = d >= (step >> 1)
        code |= np.where(b, 2, 0)
        d = d - np.where(b, step >> 1, 0)
        code |= np.where(d >= (step >> 2), 1, 0)
        # the decoder's update (kiwi/client.py:74-87)
        diff = step >> 3
        diff = diff + np.where(code & 1, step >> 2, 0) + np.where(code & 2, step >> 1, 0) + np.where(code & 4, step, 0)
        diff = np.where(code & 8, -diff, diff)
        prev = np.clip(prev + diff, -32768, 32767)
        index = np.clip(index + ADJ[code], 0, 88)
        codes[:, i] = code
        rec[:, i] = prev
    out = (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)
    new = np.stack([index, prev], 1).astype(np.int32)
    if one:
        return out[0], rec[0], new[0]
    return out, rec, new


def encode_stream(pcm, state=None):
    """encode() of ONE stream in plain Python integers -> (uint8 [n_samples // 2], the new state int32 [2]).  The same steps as
    encode(), to which tests/test_stage_matrix_inputs.py holds it byte for byte; for streams of 10^5 samples, where encode()'s
    per-sample NumPy calls are the slow part."""
    x = [int(v) for v in np.asarray(pcm).reshape(-1)]
    if len(x) % 2:
        raise ValueError("an even number of samples per stream")
    index, prev = (0, 0) if state is None else (int(state[0]), int(state[1]))
    if not (0 <= index <= 88 and -32768 <= prev <= 32767):
        raise ValueError("state out of range")
    step_t, adj_t = [int(v) for v in STEP], [int(v) for v in ADJ]
    codes = bytearray(len(x))
    for i, s in enumerate(x):
        step = step_t[index]
        d = s - prev
        code = 0
        if d < 0:
            code, d = 8, -d
        diff = step >> 3
        if d >= step:
            code |= 4
            d -= step
            diff += step
        if d >= step >> 1:
            code |= 2
            d -= step >> 1
            diff += step >> 1
        if d >= step >> 2:
            code |= 1
            diff += step >> 2
        prev = max(-32768, prev - diff) if code & 8 else min(32767, prev + diff)
        index = min(88, max(0, index + adj_t[code]))
        codes[i] = code
    c = np.frombuffer(bytes(codes), np.uint8)
    return (c[0::2] | (c[1::2] << 4)).astype(np.uint8), np.array([index, prev], np.int32)


def encode_wf_lines(lines):
    """byte lines int [n, 1024] (values 0..255) -> uint8 [n, 517]: each line from (0, 0), WF_PAD samples of its last byte behind it"""
    b = np.asarray(lines, np.int64)
    b = b.reshape(-1, b.shape[-1])
    padded = np.concatenate([b, np.repeat(b[:, -1:], WF_PAD, 1)], 1)
    return encode(padded)[0]
