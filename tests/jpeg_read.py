"""A reader of the entropy layer of a baseline JPEG file, in plain Python, written from ITU T.81 and from nothing of tests/jpeg_np.py: the
marker segments (B.2: DQT, SOF0, DHT, DRI, SOS), the decoder tables of a DHT (C.2 HUFFSIZE and HUFFCODE, F.2.2.3 MINCODE, MAXCODE, VALPTR),
the byte unstuffing and the RSTm markers (B.1.1.5, F.1.2.3, E.2.4), DECODE, RECEIVE and EXTEND (F.2.2.1 - F.2.2.4), the AC coefficients with
their runs, ZRL and EOB (F.2.2.2), the order of the data units in an MCU (A.2.3) and the DC prediction per component, reset at every
restart interval (F.2.1.3.1).

read(data) turns a file back into its quantised coefficients: (blocks, 64) int32 in zigzag order, the data units in the order of the scan -
what the encoder's entropy half was given.  Pillow cannot show these; with this reader a coefficient-level case is checked by something
other than the restatement that produced its bytes.  It is strict where the format is: a restart marker out of its order, an interval of
the wrong number of MCUs, a code that no table has, padding that is not 1 bits (F.1.2.3) and bytes left over all raise ValueError.
TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import numpy as np


class _Table:
    """F.2.2.3: MINCODE, MAXCODE and VALPTR by code length, from BITS and HUFFVAL"""

    def __init__(self, bits, vals):
        if len(bits) != 16 or sum(bits) != len(vals):
            raise ValueError("DHT: BITS and HUFFVAL disagree")
        self.vals, self.mincode, self.maxcode, self.valptr = list(vals), [0] * 17, [-1] * 17, [0] * 17
        code, at = 0, 0
        for length in range(1, 17):   # C.2: the codes of one length are consecutive, the first of the next length is the next one doubled
            n = bits[length - 1]
            if n:
                self.valptr[length], self.mincode[length], self.maxcode[length] = at, code, code + n - 1
                code, at = code + n, at + n
                if code > (1 << length):
                    raise ValueError("DHT: more codes of a length than there are")
            code <<= 1


class _BitSource:
    """the bits of one unstuffed interval, most significant first"""

    def __init__(self, data):
        self.data, self.at = data, 0

    def bit(self):
        if self.at >= 8 * len(self.data):
            raise ValueError("the entropy-coded segment ends inside a code")
        b = (self.data[self.at >> 3] >> (7 - (self.at & 7))) & 1
        self.at += 1
        return b

    def receive(self, n):   # F.2.2.4
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def decode(self, t):    # F.2.2.3
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if t.maxcode[length] >= 0 and t.mincode[length] <= code <= t.maxcode[length]:
                return t.vals[t.valptr[length] + code - t.mincode[length]]
        raise ValueError("a code of more than 16 bits")

    def finish(self):
        """Behind the last MCU of an interval: fewer than eight bits, all 1 (F.1.2.3)"""
        left = 8 * len(self.data) - self.at
        if left >= 8:
            raise ValueError("%d whole bytes behind the interval's last MCU" % (left // 8))
        if self.receive(left) != (1 << left) - 1:
            raise ValueError("padding bits that are not 1")
        return left


def _extend(v, t):          # F.2.2.1
    return v if t == 0 or v >= (1 << (t - 1)) else v - (1 << t) + 1


def _data_unit(src, dc, ac, pred):
    zz = [0] * 64
    t = src.decode(dc)
    if t > 11:
        raise ValueError("DC category above 11")
    zz[0] = pred + _extend(src.receive(t), t)
    k = 1
    while k < 64:           # F.2.2.2
        rs = src.decode(ac)
        r, s = rs >> 4, rs & 15
        if s == 0:
            if r == 15:
                k += 16     # ZRL
                continue
            if r:
                raise ValueError("an end-of-band run in a baseline scan")
            break           # EOB
        k += r
        if k > 63:
            raise ValueError("a run past the block's end")
        if s > 10:
            raise ValueError("AC size above 10")
        zz[k] = _extend(src.receive(s), s)
        k += 1
    else:
        if k > 64:
            raise ValueError("a ZRL past the block's end")
    return zz


def _intervals(data, at):
    """The entropy-coded segments from byte `at` to EOI, unstuffed, with the RSTm numbers between them"""
    out, markers, cur = [], [], bytearray()
    while True:
        if at >= len(data):
            raise ValueError("no EOI")
        b = data[at]
        if b != 0xFF:
            cur.append(b)
            at += 1
            continue
        if at + 1 >= len(data):
            raise ValueError("the file ends in FF")
        m = data[at + 1]
        if m == 0x00:
            cur.append(0xFF)
        elif 0xD0 <= m <= 0xD7:
            out.append(bytes(cur))
            markers.append(m - 0xD0)
            cur = bytearray()
        elif m == 0xD9:
            out.append(bytes(cur))
            if at + 2 != len(data):
                raise ValueError("bytes behind EOI")
            return out, markers
        else:
            raise ValueError("marker FF%02X inside the scan" % m)
        at += 2


def read(data):
    """{"coef": (blocks, 64) int32, "comp": (blocks,) the component index of every data unit, "width", "height", "components": [(id, H, V,
    Tq, Td, Ta)], "ri", "intervals", "pad_bits": per interval, "quant": {Tq: 64 entries in zigzag order}}"""
    data = bytes(data)
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    at, quant, huff, ri, frame, scan = 2, {}, {}, 0, None, None
    while scan is None:
        if data[at] != 0xFF:
            raise ValueError("no marker at byte %d" % at)
        m, n = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        seg = data[at + 4:at + 2 + n]
        at += 2 + n
        if m == 0xDB:
            p = 0
            while p < len(seg):
                if seg[p] >> 4:
                    raise ValueError("16-bit quantisation table in a baseline file")
                quant[seg[p] & 15] = list(seg[p + 1:p + 65])
                p += 65
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                bits = list(seg[p + 1:p + 17])
                huff[(seg[p] >> 4, seg[p] & 15)] = _Table(bits, seg[p + 17:p + 17 + sum(bits)])
                p += 17 + sum(bits)
        elif m == 0xC0:
            if seg[0] != 8:
                raise ValueError("sample precision is not 8")
            height, width, nf = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big"), seg[5]
            frame = (width, height, [(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]) for i in range(nf)])
        elif m == 0xDD:
            ri = int.from_bytes(seg[:2], "big")
        elif m == 0xDA:
            ns = seg[0]
            scan = [(seg[1 + 2 * i], seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15) for i in range(ns)]
            if tuple(seg[1 + 2 * ns:4 + 2 * ns]) != (0, 63, 0):
                raise ValueError("Ss, Se, Ah, Al of a baseline scan are 0, 63, 0, 0")
        elif 0xC1 <= m <= 0xCF and m != 0xC8 and m != 0xCC:
            raise ValueError("SOF%d: not a baseline file" % (m - 0xC0))
        elif not (0xE0 <= m <= 0xEF or m == 0xFE):
            raise ValueError("unexpected marker FF%02X" % m)
    if frame is None:
        raise ValueError("SOS in front of SOF0")
    width, height, comps = frame
    if [c[0] for c in comps] != [s[0] for s in scan]:
        raise ValueError("the scan does not hold the frame's components in order")
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    if len(comps) == 1:     # A.2.2: a non-interleaved scan's MCU is one data unit, whatever the sampling factors say
        units = [(0, 1)]
        mcus = -(-width // 8) * -(-height // 8)
    else:
        units = [(i, c[1] * c[2]) for i, c in enumerate(comps)]
        mcus = -(-width // (8 * hmax)) * -(-height // (8 * vmax))
    tables = []
    for (_, td, ta), c in zip(scan, comps):
        if (0, td) not in huff or (1, ta) not in huff or c[3] not in quant:
            raise ValueError("a table the scan names was never defined")
        tables.append((huff[(0, td)], huff[(1, ta)]))
    intervals, markers = _intervals(data, at)
    per = ri if ri else mcus
    if len(intervals) != -(-mcus // per):
        raise ValueError("%d intervals for %d MCUs at Ri %d" % (len(intervals), mcus, ri))
    if markers != [k % 8 for k in range(len(markers))]:
        raise ValueError("restart markers out of order: %r" % (markers,))
    coef, comp, pads, done = [], [], [], 0
    for raw in intervals:
        src, pred = _BitSource(raw), [0] * len(comps)
        for _ in range(min(per, mcus - done)):
            for i, n in units:
                for _ in range(n):
                    zz = _data_unit(src, tables[i][0], tables[i][1], pred[i])
                    pred[i] = zz[0]
                    coef.append(zz)
                    comp.append(i)
        done += min(per, mcus - done)
        pads.append(src.finish())
    return {"coef": np.array(coef, np.int32).reshape(-1, 64), "comp": np.array(comp), "width": width, "height": height,
            "components": [c + s[1:] for c, s in zip(comps, scan)], "ri": ri, "intervals": len(intervals), "pad_bits": pads, "quant": quant}
