"""An independent, strict FLAC decoder (RFC 9639) for the library's FLAC contract (include/jbonsai_amd.h "FLAC").

decode(data) -> (samples, info) rejects, with FlacError, anything outside that contract: a stream that is not "fLaC"
+ one STREAMINFO block (marked last) + frames; a frame sync, reserved bit or blocking bit out of place; frame numbers
that do not count up from 0; a block-size, rate or bit-depth code outside the streamable subset (rate and depth
coded in every frame, block size <= 4608, LPC order <= 12, partition order <= 8) or against STREAMINFO; a bad CRC-8
or CRC-16; a subframe type, wasted-bits flag, LPC precision or shift out of range; an invalid partition order;
nonzero padding; residuals or samples out of range; STREAMINFO fields that disagree with the frames.  Samples are
rebuilt with Python integers (exact)."""
import numpy as np


class FlacError(ValueError):
    pass


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


def _crc16_table():
    t = []
    for i in range(256):
        c = i << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xFFFF if c & 0x8000 else (c << 1) & 0xFFFF
        t.append(c)
    return t


_T16 = _crc16_table()


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _T16[(c >> 8) ^ b]
    return c


_BS = {1: 192, 2: 576, 3: 1152, 4: 2304, 5: 4608, 8: 256, 9: 512, 10: 1024, 11: 2048, 12: 4096, 13: 8192,
       14: 16384, 15: 32768}
_RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000,
          11: 96000}
_FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


class _Reader:
    """MSB-first bit reader over bytes; unary codes found through the positions of the one bits."""

    def __init__(self, data: bytes):
        self.data = data
        self.n = len(data) * 8
        self.pos = 0
        self.ones = np.flatnonzero(np.unpackbits(np.frombuffer(data, dtype=np.uint8))).tolist()
        self.oi = 0

    def bits(self, k: int) -> int:
        if k == 0:
            return 0
        if self.pos + k > self.n:
            raise FlacError("read past the end of the stream")
        b0, b1 = self.pos >> 3, (self.pos + k + 7) >> 3
        v = int.from_bytes(self.data[b0:b1], "big")
        v >>= (b1 * 8) - (self.pos + k)
        self.pos += k
        return v & ((1 << k) - 1)

    def sbits(self, k: int) -> int:
        v = self.bits(k)
        return v - (1 << k) if k and v >> (k - 1) else v

    def unary(self) -> int:
        ones, i, pos = self.ones, self.oi, self.pos
        while i < len(ones) and ones[i] < pos:
            i += 1
        if i >= len(ones):
            raise FlacError("unary code runs past the end")
        q = ones[i] - pos
        self.pos = pos + q + 1
        self.oi = i + 1
        return q


def _utf8_number(r: _Reader) -> int:
    b = r.bits(8)
    if b < 0x80:
        return b
    n = 0
    while b & (0x80 >> n):
        n += 1
    if n < 2 or n > 7:
        raise FlacError("bad coded frame number")
    v = b & (0x7F >> n)
    for _ in range(n - 1):
        c = r.bits(8)
        if c & 0xC0 != 0x80:
            raise FlacError("bad coded frame number continuation")
        v = (v << 6) | (c & 0x3F)
    return v


def _residual(r: _Reader, bs: int, order: int, out: list):
    method = r.bits(2)
    if method > 1:
        raise FlacError("reserved residual coding method")
    pbits = 4 if method == 0 else 5
    esc = (1 << pbits) - 1
    p = r.bits(4)
    if p > 8:
        raise FlacError("partition order above 8 (subset)")
    if bs % (1 << p):
        raise FlacError("block size not divisible by the partition count")
    plen = bs >> p
    if plen <= order:
        raise FlacError("first partition not longer than the predictor order")
    for j in range(1 << p):
        m = plen - (order if j == 0 else 0)
        k = r.bits(pbits)
        if k == esc:
            nb = r.bits(5)
            for _ in range(m):
                out.append(r.sbits(nb) if nb else 0)
        else:
            for _ in range(m):
                q = r.unary()
                u = (q << k) | r.bits(k)
                out.append((u >> 1) ^ -(u & 1))
    for v in out:
        if v < -(1 << 31) or v >= (1 << 31):
            raise FlacError("residual outside 32 bits")


def _subframe(r: _Reader, bs: int, info: dict):
    if r.bits(1):
        raise FlacError("subframe padding bit set")
    t = r.bits(6)
    if r.bits(1):
        raise FlacError("wasted-bits flag set")
    if t == 0:
        info["types"].append("constant")
        return [r.sbits(16)] * bs
    if t == 1:
        info["types"].append("verbatim")
        return [r.sbits(16) for _ in range(bs)]
    if 8 <= t <= 12:
        order = t - 8
        if order > bs:
            raise FlacError("FIXED order above the block size")
        s = [r.sbits(16) for _ in range(order)]
        res = []
        _residual(r, bs, order, res)
        c = _FIXED[order]
        for e in res:
            s.append(e + sum(c[j] * s[-1 - j] for j in range(order)))
        info["types"].append(f"fixed{order}")
        return s
    if t >= 32:
        order = t - 31
        if order > 12:
            raise FlacError("LPC order above 12 (subset)")
        if order > bs:
            raise FlacError("LPC order above the block size")
        s = [r.sbits(16) for _ in range(order)]
        prec = r.bits(4)
        if prec == 15:
            raise FlacError("LPC precision code 1111")
        prec += 1
        shift = r.sbits(5)
        if shift < 0 or shift > 15:
            raise FlacError("LPC shift outside 0..15")
        qc = [r.sbits(prec) for _ in range(order)]
        res = []
        _residual(r, bs, order, res)
        for e in res:
            acc = 0
            for j in range(order):
                acc += qc[j] * s[-1 - j]
            s.append(e + (acc >> shift))
        info["types"].append(f"lpc{order}")
        return s
    raise FlacError(f"reserved subframe type {t}")


def decode(data: bytes):
    """(int16 samples, info) of a stream in the library's FLAC contract; FlacError otherwise."""
    data = bytes(data)
    if len(data) < 42 or data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    if data[4] != 0x80 or data[5:8] != b"\x00\x00\x22":
        raise FlacError("expected one STREAMINFO block, marked last, of 34 bytes")
    si = data[8:42]
    min_bs, max_bs = int.from_bytes(si[0:2], "big"), int.from_bytes(si[2:4], "big")
    min_fs, max_fs = int.from_bytes(si[4:7], "big"), int.from_bytes(si[7:10], "big")
    v = int.from_bytes(si[10:18], "big")
    rate, ch, bps, total = v >> 44, (v >> 41) & 7, ((v >> 36) & 31) + 1, v & ((1 << 36) - 1)
    if min_bs != max_bs or min_bs < 16 or min_bs > 4608:
        raise FlacError("STREAMINFO block sizes")
    if ch != 0 or bps != 16:
        raise FlacError("not mono 16-bit")
    if rate == 0:
        raise FlacError("STREAMINFO rate 0")
    if any(si[18:34]):
        raise FlacError("MD5 is not zero")
    bs_nom = min_bs
    out = []
    sizes = []
    info = {"rate": rate, "block_size": bs_nom, "total": total, "min_frame": min_fs, "max_frame": max_fs,
            "types": [], "frames": 0}
    pos = 42
    fno = 0
    r = _Reader(data)
    while pos < len(data):
        r.pos = 8 * pos
        if r.bits(14) != 0x3FFE:
            raise FlacError("frame sync")
        if r.bits(1):
            raise FlacError("frame header reserved bit")
        if r.bits(1):
            raise FlacError("variable blocking")
        bcode, rcode = r.bits(4), r.bits(4)
        chan, ssize, resv = r.bits(4), r.bits(3), r.bits(1)
        if chan != 0:
            raise FlacError("channel assignment is not mono")
        if ssize != 4:
            raise FlacError("sample size code is not 16 bits (subset: never from STREAMINFO)")
        if resv:
            raise FlacError("frame header reserved bit (after the sample size)")
        num = _utf8_number(r)
        if num != fno:
            raise FlacError(f"frame number {num}, expected {fno}")
        if bcode == 0:
            raise FlacError("reserved block size code")
        if bcode == 6:
            bs = r.bits(8) + 1
        elif bcode == 7:
            bs = r.bits(16) + 1
        else:
            bs = _BS[bcode]
        if rcode == 0:
            raise FlacError("rate from STREAMINFO (not in the subset)")
        if rcode == 15:
            raise FlacError("invalid rate code")
        if rcode == 12:
            hz = r.bits(8) * 1000
        elif rcode == 13:
            hz = r.bits(16)
        elif rcode == 14:
            hz = r.bits(16) * 10
        else:
            hz = _RATES[rcode]
        if hz != rate:
            raise FlacError("frame rate differs from STREAMINFO")
        if bs > 4608:
            raise FlacError("block size above 4608 (subset)")
        hlen = r.pos // 8 - pos
        if crc8(data[pos:pos + hlen]) != r.bits(8):
            raise FlacError("CRC-8")
        s = _subframe(r, bs, info)
        if r.pos % 8:
            if r.bits(8 - r.pos % 8):
                raise FlacError("nonzero padding")
        body = r.pos // 8 - pos
        if body + 2 > len(data) - pos:
            raise FlacError("truncated frame")
        if crc16(data[pos:pos + body]) != int.from_bytes(data[pos + body:pos + body + 2], "big"):
            raise FlacError("CRC-16")
        for x in s:
            if x < -32768 or x > 32767:
                raise FlacError("sample outside 16 bits")
        out.extend(s)
        sizes.append(body + 2)
        if bs != bs_nom and sizes and pos + body + 2 < len(data):
            raise FlacError("a frame other than the last is not block_size long")
        if bs > bs_nom:
            raise FlacError("frame longer than the nominal block size")
        pos += body + 2
        fno += 1
    if len(out) != total:
        raise FlacError(f"total samples {total}, decoded {len(out)}")
    if (min(sizes) if sizes else 0) != min_fs or (max(sizes) if sizes else 0) != max_fs:
        raise FlacError("STREAMINFO frame sizes disagree with the frames")
    info["frames"] = fno
    info["frame_sizes"] = sizes
    return np.array(out, dtype=np.int16), info


def verbatim_frame_bound(n: int, frame: int, hz: int) -> int:
    """Bytes of the VERBATIM frame of n samples (header as the library codes it, subframe, CRC-16)."""
    h = 4 + (1 if frame < 0x80 else 2 if frame < 0x800 else 3 if frame < 0x10000 else 4 if frame < 0x200000 else 5
             if frame < 0x4000000 else 6)
    if n not in (192, 576, 1152, 2304, 4608) and not (n >= 256 and n & (n - 1) == 0):
        h += 1 if n <= 256 else 2
    if hz not in _RATES.values():
        h += 1 if hz % 1000 == 0 and hz // 1000 <= 255 else 2
    return h + 1 + 1 + 2 * n + 2
