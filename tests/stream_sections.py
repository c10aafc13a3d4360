"""The plane sections of a picture packet as symbol lists, for the model of tests/entropy_cases.py: which planes of a real stream the GPU
entropy coder would hand to the host (flag 1).

A picture packet ends with its three plane sections, each a 32-bit length and that many bytes, the last of them 0x55 (hzcc.c:586-613);
what stands in front (header, side information) is not parsed here: the sections are found from the packet's end, as the one offset
from which three length fields chain exactly to the last byte.  A section is then parsed the way hzcc_dec does (hzcc.c:451-583), into
the quantised value at every scan position -- which, placed in a plane, is the lossless plane with the same symbol list."""
import numpy as np

import dsvabi as A
import entropy_cases as E


def find_sections(packet):
    """[(offset of the length field, length)] of the three sections, or None where no offset chains to the packet's end"""
    n = len(packet)
    for x in range(n - 27, 0, -1):  # (three empty sections take 3 * 13 bytes; the first fit from the back is taken)
        pos, out = x, []
        for _ in range(3):
            if pos + 4 > n:
                break
            plen = int.from_bytes(packet[pos:pos + 4], "big")
            if plen < 5 or pos + 4 + plen > n or packet[pos + 4 + plen - 1] != 0x55:
                break
            out.append((pos, plen))
            pos += 4 + plen
        if len(out) == 3 and pos == n:
            return out
    return None


class _Bits:
    def __init__(self, data):
        self.b = np.unpackbits(np.frombuffer(data, dtype=np.uint8)).tolist()
        self.p = 0

    def bit(self):
        self.p += 1
        return self.b[self.p - 1]

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def align(self):
        self.p = (self.p + 7) & ~7

    def ueg(self):
        v = 1
        while not self.bit():
            v = (v << 1) | self.bit()
        return v - 1


def parse_section(section, scan):
    """the dense scan values (position 0: the DC) of a section without its length field"""
    r = _Bits(section)
    sv = np.zeros(scan.total, dtype=np.int32)
    ll = r.ueg()
    if ll and r.bit():
        ll = -ll
    sv[0] = ll
    r.align()
    runs = r.bits(24)
    r.align()
    cur, vk, seg = 0, 0, 0
    for _ in range(runs):
        p = cur + r.ueg()
        assert 0 < p < scan.total, "a run that leaves the plane"
        while p >= scan.base[seg + 1]:
            seg += 1
        if seg == 0:
            v = r.ueg() + 1
            if r.bit():
                v = -v
        else:
            k = vk >> (3 + (seg - 1) // 3)
            q = 0
            while not r.bit():
                q += 1
            vk += 1 if q else (-1 if vk > 0 else 0)
            u = ((q << k) | r.bits(k)) + 1
            v = (u >> 1) ^ -(u & 1)
        sv[p] = v
        cur = p + 1
    r.align()
    assert r.bits(8) == 0x55
    return sv


def plane_models(packet, w, h, subsamp):
    """the model of each plane's symbol list, or None for a packet that holds no picture"""
    secs = find_sections(packet)
    if secs is None:
        return None
    out = []
    for (pos, plen), (cw, ch) in zip(secs, A.coef_dims(subsamp, w, h)):
        scan = E.Scan(cw, ch)
        sv = parse_section(packet[pos + 4:pos + 4 + plen], scan)
        assert scan.total == cw * ch, "a plane whose scanned regions overlap has no plane of its scan values"
        out.append(E.Model(scan, scan.plane_of(sv)))
    return out


def plane_flags(packet, w, h, subsamp):
    ms = plane_models(packet, w, h, subsamp)
    return None if ms is None else [(m.n, int(m.met.max()), max(m.chain_states(), default=0), m.flags() & 1) for m in ms]


# ---- the stream whose planes reach flag 1 inside the packet bound, and a neighbour that does not --------------------------------------
# Searched with the reference at 352 x 288, 4:2:0, two identical pictures: the 0/255 checkerboard codes lossless into an I picture of
# 80 783 bytes, 0.40 of the packet bound, and at qp 99 / 98 / 97 into 104 278 / 99 964 / 99 067 (0.51 / 0.49 / 0.49); the model gives
# flag 1 for all three planes of each (state 320 lossless, 384 / 352 / 352 luma and 288 chroma at the three qualities).  0/255 noise
# reaches it too (state 289) but its lossless picture takes 189 846 bytes, 0.94 of the bound, and at qp 99 the reference outgrows it;
# three impulses stay at states of 68 - 93.
FLAG1_W, FLAG1_H = 352, 288


def stream_dict(frames, cfg, seed=0):
    """a stream in the form tests/mixed_steps.py's Runner takes"""
    import mixed_steps as M
    sp = M.spec(seed, len(frames), cfg, w=FLAG1_W, h=FLAG1_H)
    return dict(frames=list(frames), meta_kw=dict(w=FLAG1_W, h=FLAG1_H, subsamp=A.SUBSAMP_420), cfg=dict(sp.cfg), spec=sp, rgb=None)


def flag1_stream():
    from edge_cases import content_planes
    fb = b"".join(p.tobytes() for p in content_planes("checker", A.SUBSAMP_420, FLAG1_W, FLAG1_H))
    return stream_dict([fb, fb], dict(qp=100, gop=4))


def neighbour_stream():
    import mixed_steps as M
    return M.build(M.spec(31, 2, dict(qp=60, gop=4), w=FLAG1_W, h=FLAG1_H))


def reference_of(st):
    """(packets, stats, pictures the model gives flag 1) of the reference's encode of a stream"""
    from codec_run import encode_stream
    pk, stats = encode_stream(A.load_ref(), st["frames"], FLAG1_W, FLAG1_H, A.SUBSAMP_420, eos=False, meta=A.mk_meta(**st["meta_kw"]), **st["cfg"])
    flagged = 0
    for p in pk:
        if p[5] & 4:  # a picture packet (dsv.h: DSV_PT_PIC)
            flagged += any(m.flags() & 1 for m in plane_models(p, FLAG1_W, FLAG1_H, A.SUBSAMP_420))
    return pk, stats, flagged
