"""The metadata of a FLAC stream with an MD5 or a SEEKTABLE (include/jbonsai_amd.h "FLAC"), taken apart for the tests.

tests/flac_ref.py::decode is strict about the plain contract: it rejects a non-zero MD5 and a STREAMINFO that is not
the last block.  split(data) reads the metadata blocks of a stream that may carry both -- "fLaC", STREAMINFO, at most
one SEEKTABLE (marked last), frames -- and returns the STREAMINFO fields, the digest, the seek points and the *plain
form*: a 42-byte header, marked last, with a zeroed digest, followed by the frames.  The plain form goes to decode.
Anything else in front of the frames is a FlacError."""
from tests.flac_ref import FlacError, decode


def split(data: bytes):
    data = bytes(data)
    if len(data) < 42 or data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    if data[4] & 0x7F != 0 or data[5:8] != b"\x00\x00\x22":
        raise FlacError("the first block is not a STREAMINFO of 34 bytes")
    si_last = bool(data[4] & 0x80)
    si = data[8:42]
    v = int.from_bytes(si[10:18], "big")
    info = {"streaminfo_last": si_last, "md5": si[18:34], "rate": v >> 44, "total": v & ((1 << 36) - 1),
            "block_size": int.from_bytes(si[0:2], "big"), "min_frame": int.from_bytes(si[4:7], "big"),
            "max_frame": int.from_bytes(si[7:10], "big"), "points": None, "seektable_last": None, "header_bytes": 42}
    pos = 42
    if not si_last:
        if len(data) < 46:
            raise FlacError("STREAMINFO is not last and nothing follows")
        if data[42] & 0x7F != 3:
            raise FlacError(f"block type {data[42] & 0x7F} behind STREAMINFO, expected a SEEKTABLE")
        info["seektable_last"] = bool(data[42] & 0x80)
        if not info["seektable_last"]:
            raise FlacError("the SEEKTABLE is not the last block")
        length = int.from_bytes(data[43:46], "big")
        if length == 0 or length % 18 or 46 + length > len(data):
            raise FlacError("SEEKTABLE length")
        pts = []
        for k in range(length // 18):
            p = data[46 + 18 * k:46 + 18 * k + 18]
            pts.append((int.from_bytes(p[0:8], "big"), int.from_bytes(p[8:16], "big"), int.from_bytes(p[16:18], "big")))
        for a, b in zip(pts, pts[1:]):
            if not a[0] < b[0]:
                raise FlacError("seek points are not ascending")
        if any(p[0] == 0xFFFFFFFFFFFFFFFF for p in pts):
            raise FlacError("placeholder seek point")
        info["points"] = pts
        pos = 46 + length
    info["header_bytes"] = pos
    plain = data[:4] + b"\x80\x00\x00\x22" + si[:18] + bytes(16) + data[pos:]
    return info, plain


def check(data: bytes):
    """(samples, decoder info, metadata info) of a stream: its plain form through the strict decoder, and every seek
    point against the decoded frames -- sample number, offset, sample count, and the frame sync and frame number at
    header_bytes + offset."""
    meta, plain = split(data)
    samples, info = decode(plain)
    if meta["points"] is not None:
        bs, sizes = info["block_size"], info["frame_sizes"]
        starts = [sum(sizes[:f]) for f in range(len(sizes))]
        for (s0, off, cnt) in meta["points"]:
            if s0 % bs or s0 // bs >= len(sizes):
                raise FlacError(f"seek point at sample {s0} is no frame's first sample")
            f = s0 // bs
            if off != starts[f]:
                raise FlacError(f"seek point of frame {f}: offset {off}, the frame starts at {starts[f]}")
            if cnt != min(bs, len(samples) - s0):
                raise FlacError(f"seek point of frame {f}: {cnt} samples")
            at = meta["header_bytes"] + off
            if data[at] != 0xFF or data[at + 1] != 0xF8:
                raise FlacError(f"no frame sync at the offset of frame {f}")
            if _frame_number(data, at + 4) != f:
                raise FlacError(f"the frame at the offset of frame {f} carries another number")
    return samples, info, meta


def _frame_number(data: bytes, pos: int) -> int:
    b = data[pos]
    if b < 0x80:
        return b
    n = 0
    while b & (0x80 >> n):
        n += 1
    v = b & (0x7F >> n)
    for k in range(1, n):
        v = (v << 6) | (data[pos + k] & 0x3F)
    return v
