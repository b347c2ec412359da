"""A reader of AVI files written from the container's published layout alone (RIFF chunks: a fourcc, a little-endian size, the payload,
a pad byte behind an odd size; LIST chunks hold a type and chunks), sharing no code with rayn_amd.image.AviWriter.  read(data) returns
what the file says, every size checked against where the chunks really are.  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import struct


def _chunks(data, at, end):
    """[(fourcc, payload start, payload size)] of the chunks in data[at:end]"""
    out = []
    while at < end:
        assert at + 8 <= end, "a chunk header past its list's end"
        fourcc, size = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        assert at + 8 + size <= end, (fourcc, "payload past its list's end")
        out.append((fourcc, at + 8, size))
        at += 8 + size + (size & 1)
        assert at <= end or (size & 1) == 0, (fourcc, "no pad byte behind an odd chunk")
    assert at == end, "chunks do not fill their list"
    return out


def _list(data, chunk, kind):
    fourcc, at, size = chunk
    assert fourcc == b"LIST" and data[at:at + 4] == kind, (fourcc, data[at:at + 4], kind)
    return _chunks(data, at + 4, at + size)


def read(data):
    """{"avih": 14 words, "strh": dict, "strf": dict, "frames": [bytes], "frame_at": [file offset of each 00dc chunk header], "index":
    [(fourcc, flags, offset, size)], "movi_at": file offset of the movi fourcc}"""
    data = bytes(data)
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI ", "not a RIFF AVI file"
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8, "the RIFF size is not the file's"
    top = _chunks(data, 12, len(data))
    assert [c[0] for c in top] == [b"LIST", b"LIST", b"idx1"], [c[0] for c in top]
    hdrl = _list(data, top[0], b"hdrl")
    assert [c[0] for c in hdrl] == [b"avih", b"LIST"] and hdrl[0][2] == 56
    avih = struct.unpack("<14I", data[hdrl[0][1]:hdrl[0][1] + 56])
    strl = _list(data, hdrl[1], b"strl")
    assert [c[0] for c in strl] == [b"strh", b"strf"] and strl[0][2] == 56 and strl[1][2] == 40
    h = data[strl[0][1]:strl[0][1] + 56]
    names = ("flags", "priority", "language", "initial_frames", "scale", "rate", "start", "length", "buffer", "quality", "sample_size")
    strh = dict(zip(names, struct.unpack("<IHHIIIIIIII", h[8:48])), type=h[:4], handler=h[4:8], frame=struct.unpack("<4h", h[48:56]))
    f = struct.unpack("<IiiHH4sIiiII", data[strl[1][1]:strl[1][1] + 40])
    strf = dict(zip(("size", "width", "height", "planes", "bits", "compression", "image_bytes"), f[:7]))
    movi_at = top[1][1]
    movi = _list(data, top[1], b"movi")
    assert all(c[0] == b"00dc" for c in movi)
    idx = data[top[2][1]:top[2][1] + top[2][2]]
    assert len(idx) % 16 == 0
    index = [(idx[k:k + 4],) + struct.unpack("<III", idx[k + 4:k + 16]) for k in range(0, len(idx), 16)]
    return {"avih": avih, "strh": strh, "strf": strf, "frames": [data[at:at + n] for _, at, n in movi], "frame_at": [at - 8 for _, at, _ in movi],
            "index": index, "movi_at": movi_at}
