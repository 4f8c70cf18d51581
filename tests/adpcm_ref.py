"""A pure-Python model of the IMA ADPCM stage (include/jbonsai_amd.h "IMA ADPCM"): the geometry, the encoder with the
block-local start index, the decoder, and a second encoder mode that carries the step index from block to block the
way the serial encoders do (carry=True), for the quality gate.  Written from the rule text, not from the library."""
import numpy as np

STEP = [7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45, 50, 55, 60, 66, 73, 80, 88, 97,
        107, 118, 130, 143, 157, 173, 190, 209, 230, 253, 279, 307, 337, 371, 408, 449, 494, 544, 598, 658, 724, 796,
        876, 963, 1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066, 2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871,
        5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899, 15289, 16818, 18500, 20350, 22385, 24623,
        27086, 29794, 32767]
IDX = [-1, -1, -1, -1, 2, 4, 6, 8]
assert len(STEP) == 89


def block_align(hz, a=0):
    if a:
        if a % 4 or not 32 <= a <= 8192:
            raise ValueError("block_align")
        return a
    return 256 if hz < 22050 else 512 if hz < 44100 else 1024


def geometry(hz, n, a=0):
    """(A, samples per block, blocks, bytes)"""
    A = block_align(hz, a)
    spb = 2 * (A - 4) + 1
    nb = -(-n // spb)
    return A, spb, nb, nb * A


def quantise(x):
    """The 16-bit sink's rule: clamp, then truncate toward zero.  Integer arrays pass through."""
    x = np.asarray(x)
    if x.dtype.kind in "iu":
        return [int(v) for v in x]
    return [int(v) for v in np.trunc(np.clip(x.astype(np.float64), -32768.0, 32767.0))]


def code_of(s, pred, idx):
    step = STEP[idx]
    diff = s - pred
    sign = 8 if diff < 0 else 0
    diff = abs(diff)
    delta = 0
    vp = step >> 3
    if diff >= step:
        delta = 4
        diff -= step
        vp += step
    step >>= 1
    if diff >= step:
        delta |= 2
        diff -= step
        vp += step
    step >>= 1
    if diff >= step:
        delta |= 1
        vp += step
    pred = max(-32768, min(32767, pred - vp if sign else pred + vp))
    idx = max(0, min(88, idx + IDX[delta]))
    return delta | sign, pred, idx


def start_index(b):
    d = sum(abs(b[k] - b[k - 1]) for k in range(1, 9)) // 8
    for i, s in enumerate(STEP):
        if s >= d:
            return i
    return 88


def encode(x, hz, a=0, carry=False, force_i0=None, trace=None):
    """The stream's bytes.  carry: every block but the first starts at the index the block before ended with (the
    first at 0, as a serial encoder's fresh state does); force_i0: every block starts there; trace: a list that
    receives (pred, idx) after every coded sample."""
    s = quantise(x)
    n = len(s)
    A, spb, nb, _ = geometry(hz, n, a)
    out = bytearray()
    idx = 0
    for blk in range(nb):
        b = s[blk * spb:(blk + 1) * spb]
        b = b + [s[-1]] * (spb - len(b))
        pred = b[0]
        if force_i0 is not None:
            idx = force_i0
        elif not carry:
            idx = start_index(b)
        out += bytes([pred & 0xff, (pred >> 8) & 0xff, idx, 0])
        codes = []
        for k in range(1, spb):
            c, pred, idx = code_of(b[k], pred, idx)
            codes.append(c)
            if trace is not None:
                trace.append((pred, idx))
        out += bytes(codes[2 * j] | (codes[2 * j + 1] << 4) for j in range(A - 4))
    return bytes(out)


def decode(data, A, n):
    """The first n samples of the blocks, as int16."""
    spb = 2 * (A - 4) + 1
    out = []
    for blk in range(-(-n // spb)):
        y = data[blk * A:(blk + 1) * A]
        pred = int.from_bytes(y[0:2], "little", signed=True)
        idx = min(y[2], 88)
        out.append(pred)
        for k in range(1, spb):
            by = y[4 + (k - 1) // 2]
            c = by & 15 if k & 1 else by >> 4
            step = STEP[idx]
            vp = step >> 3
            if c & 4:
                vp += step
            if c & 2:
                vp += step >> 1
            if c & 1:
                vp += step >> 2
            pred = max(-32768, min(32767, pred - vp if c & 8 else pred + vp))
            idx = max(0, min(88, idx + IDX[c & 7]))
            out.append(pred)
    return np.array(out[:n], dtype=np.int16)


def snr_db(x, y):
    x = np.asarray(x, dtype=np.float64)
    e = x - np.asarray(y, dtype=np.float64)
    return 10.0 * np.log10(np.sum(x * x) / np.sum(e * e))


def speech_like(fs, seconds=3.0, seed=1):
    """The quality gate's signal: a harmonic tone with a wandering pitch under a syllable-rate envelope, plus noise,
    scaled to peak 20000 and rounded."""
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * fs)) / fs
    f0 = 120 + 30 * np.sin(2 * np.pi * 0.7 * t)
    phase = 2 * np.pi * np.cumsum(f0) / fs
    x = np.zeros_like(t)
    for k in range(1, int(min(3500, fs / 2.2) / 150)):
        x += k ** -1.2 * np.sin(k * phase)
    env = np.maximum(np.sin(2 * np.pi * 1.3 * t), 0) ** 2 + 0.001
    x = x * env + 0.02 * rng.standard_normal(t.size) * (env + 0.05)
    return np.round(x * (20000 / np.max(np.abs(x))))
