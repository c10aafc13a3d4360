"""Crafted lossless coefficient planes for the GPU entropy coder (csrc/entropy_gpu.hip) and the device parser (csrc/dec_parse_dev.hip),
and a pure-Python model of the coder that says what each plane exercises.

In lossless mode the reference codes a coefficient plane as it stands (hzcc.c:268-306): every nonzero coefficient, in scan order, is
one symbol.  So a plane built by placing values at scan positions IS a symbol list, and the reference's dsv_encode_plane /
dsv_decode_plane judge what the library makes of it bit for bit.

The model restates, per symbol: the run code (UEG, bs.c:132), the value code (NEG in the LL region, bs.c:206; adaptive Rice behind
it, bs.c:237-251, with the state vk and k = vk >> (3 + level)), and on top of that what only the GPU coder has: chunks of 1024
symbols counted from the plane's first symbol, the state at every chunk start, where the 256 trajectories of a chunk have joined
and at which look the kernel sees it (k_ent_tables), and the flags the coder must raise.  tests/test_entropy_cases_ref.py holds
the model against the reference and asserts every label below from it; tests/test_gpu_entropy_stage.py runs the cases on the GPU.

Two kinds of label.  What the codes are -- lengths, states, bit counts -- restates the reference, and the CPU module holds it against
the reference's bytes.  What the GPU coder makes of them -- the look schedule of join(), the walk over zero padding in
chain_states(), handover() -- restates the kernels, not the reference: it says which decision of the kernels a case puts to the
test and which flags to expect, and the only judge of the kernels is the reference's bytes and the flag counters on the GPU.

|v| <= 2^20 everywhere (the reference's int arithmetic stays defined), never INT_MIN."""
import ctypes as C
import functools

import numpy as np

import dsvabi as A
from edge_cases import plane_bitstream_bytes

CHUNK = 1024          # kEntChunk
STATES = 256          # kStates: start states k_ent_chain tabulates
MIRROR = 1 << 20      # kEntMirrorBytes
ABSURD_BITS = 1 << 24  # a chunk of this many bits raises flag 4
VMAX = 1 << 20


# ---- scan geometry (hzcc.c:40-57, :264-342; csrc/scan.cpp) --------------------------------------------------------------------------
def _up(x, s):
    return (x + (1 << s) - 1) >> s


class Scan:
    """seg 0 = the LL region, seg 1 + 3 * level + (sub - 1) the subbands, level 0 the coarsest; base[seg] = its first scan position"""

    def __init__(self, w, h):
        self.w, self.h = w, h
        self.off, self.sw, self.sh = [0], [_up(w, 3)], [_up(h, 3)]
        for lvl in range(3):
            for s in (1, 2, 3):
                self.off.append((_up(w, 3 - lvl) if s & 1 else 0) + (_up(h, 3 - lvl) * w if s & 2 else 0))
                self.sw.append(_up(w, 3 - lvl))
                self.sh.append(_up(h, 3 - lvl))
        self.base = [0]
        for k in range(10):
            self.base.append(self.base[k] + self.sw[k] * self.sh[k])
        self.total = self.base[10]
        # address in the plane of every scan position (odd sizes: regions of adjacent levels overlap, a coefficient is scanned twice)
        self.addr = np.concatenate([(self.off[k] + np.arange(self.sh[k])[:, None] * w + np.arange(self.sw[k])[None, :]).ravel()
                                    for k in range(10)])

    def plane_of(self, scanvals):
        """the coefficient plane that holds scanvals[p] at scan position p (position 0 is the DC, sent apart)"""
        plane = np.zeros(self.w * self.h, dtype=np.int32)
        plane[self.addr] = scanvals
        return plane

    def scan_of(self, plane):
        return plane[self.addr]


def ent_out_bytes(nscan):
    """the seam's section buffer: codec_dev.cpp ent_out_bytes with lists that hold every scan position"""
    return max(4 << 20, (nscan // 2 + 65535) & ~65535)


# ---- the codes ----------------------------------------------------------------------------------------------------------------------
def ueg_len(v):
    return 2 * ((v + 1).bit_length() - 1) + 1


def s2u(v):
    return (2 * v) ^ (-1 if v < 0 else 0)


def seg_len(v):
    return ueg_len(abs(v)) + (1 if v else 0)


class Model:
    """everything the labels need, from the plane's dense scan values"""

    def __init__(self, scan, plane, offset=0):
        sv = scan.scan_of(plane).astype(np.int64)
        self.scan = scan
        self.ll = int(plane[0])
        pos = np.flatnonzero(sv[1:]) + 1
        self.pos, self.val = pos, sv[pos]
        self.seg = np.searchsorted(np.asarray(scan.base[1:10]), pos, side="right")
        n = self.n = len(pos)
        self.nskip = int(np.count_nonzero(self.seg == 0))
        self.run_len = np.zeros(n, dtype=np.int64)   # bits of the run code in front of the symbol
        self.val_len = np.zeros(n, dtype=np.int64)   # bits of its value code (unary part included)
        self.met = np.full(n + 1, -1, dtype=np.int64)  # state before symbol i (met[n]: behind the last)
        self.k = np.full(n, -1, dtype=np.int64)
        self.thr = np.zeros(n, dtype=np.int64)       # T: the state moves up iff vk < T
        vk, prev_end = 0, 0
        for i in range(n):
            p, v, s = int(pos[i]), int(self.val[i]), int(self.seg[i])
            assert v != 0 and abs(v) <= VMAX
            self.run_len[i] = ueg_len(p - prev_end)
            prev_end = p + 1
            self.met[i] = vk
            if s == 0:
                self.val_len[i] = ueg_len(abs(v) - 1) + 1
            else:
                damp = 3 + (s - 1) // 3
                u = s2u(v) - 1
                k = vk >> damp
                q = u >> k
                self.k[i], self.thr[i] = k, u.bit_length() << damp
                self.val_len[i] = q + 1 + k
                vk += 1 if q else (-1 if vk > 0 else 0)
        self.met[n] = vk
        self.value_bits = int(self.val_len.sum())
        self.bits = self.value_bits + int(self.run_len.sum())
        head = 4 + (seg_len(self.ll) + 7) // 8 + 3
        self.section_bytes = head + (self.bits + 7) // 8 + 1
        # bit position, counted from the buffer's start, of every symbol's run code when the section starts at byte `offset`
        self.code_at = (offset + head) * 8 + np.concatenate([[0], np.cumsum(self.run_len + self.val_len)])
        # ---- what only the GPU coder has
        self.nch = (n + CHUNK - 1) // CHUNK
        self.chunk_bits = [int((self.run_len[c * CHUNK:(c + 1) * CHUNK] + self.val_len[c * CHUNK:(c + 1) * CHUNK]).sum()) for c in range(self.nch)]
        self.chunk_start = [int(self.met[c * CHUNK]) for c in range(self.nch)]

    # -- the join of a chunk's 256 trajectories (k_ent_tables) --
    @functools.lru_cache(maxsize=None)
    def join(self, c):
        """(true, look): `true` = Rice symbols of chunk c after which all 256 start states sit on two neighbouring values for the
        first time, or None; `look` = the symbol index in the chunk at which the kernel sees it (it looks where 4 * q - nskip >= 128,
        every 16 groups of 4 from the group that holds the prefix's end, and never at the chunk's end), or None: kNotJoined"""
        first, cnt = c * CHUNK, min(CHUNK, self.n - c * CHUNK)
        nskip = int(np.count_nonzero(self.seg[first:first + cnt] == 0))
        looks, q, qend = set(), nskip >> 2, (cnt + 3) >> 2
        while q < qend:
            q = min(qend, q + 16)
            if q < qend and 4 * q - nskip >= 128:
                looks.add(4 * q)
        vk = np.arange(STATES, dtype=np.int64)
        true, look = None, None
        for s in range(nskip, cnt):
            if s in looks and look is None and vk.max() - vk.min() <= 1:
                look = s
            t = self.thr[first + s]
            vk = np.where(vk < t, vk + 1, np.maximum(vk - 1, 0))
            if true is None and vk.max() - vk.min() <= 1:
                true = s + 1 - nskip
            if true is not None and (look is not None or s + 1 > max(looks, default=0)):
                break
        return true, look

    def handover(self, c, join_range=1, swap=False):
        """The state chunk c hands to chunk c + 1 the way the kernels work it out: all 256 start states walked to the first look at
        which they span join_range or less (k_ent_tables), the pair (m, m + 1) walked on from there (k_ent_pair), and the chunk's true
        start state given the end of the pair member it stood on (k_ent_chain) -- of the other one with `swap`.  With join_range = 1
        and no swap that is the true state, met[(c + 1) * 1024]; a case is only a test of the join where the others give another."""
        first, cnt = c * CHUNK, min(CHUNK, self.n - c * CHUNK)
        assert cnt == CHUNK, "a chunk that hands a state on is a full one"
        nskip = int(np.count_nonzero(self.seg[first:first + cnt] == 0))
        looks, q = set(), nskip >> 2
        while q < CHUNK // 4:
            q = min(CHUNK // 4, q + 16)
            if q < CHUNK // 4 and 4 * q - nskip >= 128:
                looks.add(4 * q)
        vk, pair, m = np.arange(STATES, dtype=np.int64), None, 0
        for s in range(nskip, cnt):
            if pair is None and s in looks and vk.max() - vk.min() <= join_range:
                m = int(vk.min())
                pair = np.array([m, m + 1], dtype=np.int64)
            t = self.thr[first + s]
            if pair is None:
                vk = np.where(vk < t, vk + 1, np.maximum(vk - 1, 0))
            else:
                pair = np.where(pair < t, pair + 1, np.maximum(pair - 1, 0))
        at = int(vk[self.chunk_start[c]])
        if pair is None:
            return at
        return int(pair[0] if (at == m) != swap else pair[1])

    def chain_states(self):
        """the state k_ent_chain sees behind every chunk: the true one -- but a last, partial chunk whose trajectories the kernel saw
        join is walked on over its zero padding (k_ent_pair), every step of which moves the state down"""
        out = []
        for c in range(self.nch):
            end = min((c + 1) * CHUNK, self.n)
            st = int(self.met[end])
            if end - c * CHUNK < CHUNK and self.join(c)[1] is not None:
                st = max(st - (CHUNK - (end - c * CHUNK)), 0)
            out.append(st)
        return out

    def flags(self):
        """the flags the GPU coder must raise for this plane, coded as plane `cur_plane` beside two empty planes (9 bytes each)"""
        f = 0
        levels = np.maximum(self.seg - 1, 0) // 3
        if any(s >= STATES for s in self.chain_states()) or bool(np.any((self.seg > 0) & ((self.met[:-1] >> 3 >> levels) >= 32))):
            f |= 1
        kept = sum(b for b in self.chunk_bits if b < ABSURD_BITS)
        if kept != self.bits:
            f |= 4
        total = 18 + self.section_bytes - (self.bits + 7) // 8 + (kept + 7) // 8
        if total + 16 > ent_out_bytes(self.scan.total):
            f |= 2
        elif total > MIRROR:
            f |= 8
        return f

    def longest_flip_run(self, level):
        """most consecutive symbols of `level` that meet vk on a multiple of 2^damp or one below it, k changing from each to the next"""
        best = cur = 0
        for i in range(1, self.n):
            s0, s1 = int(self.seg[i - 1]), int(self.seg[i])
            if s0 and s1 and (s0 - 1) // 3 == level == (s1 - 1) // 3 and self.k[i] != self.k[i - 1]:
                cur += 1
                best = max(best, cur)
            else:
                cur = 0
        return best

    def straddles(self, span=2048 * 8):
        """symbols whose run + value code holds a bit position that is a multiple of `span` bits of the buffer (the parser's window)"""
        a, b = self.code_at[:-1], self.code_at[1:] - 1
        return int(np.count_nonzero(a // span != b // span))

    def codes_in_tail(self, bits=256):
        """symbols whose codes start within the last `bits` bits of the codes"""
        return int(np.count_nonzero(self.code_at[:-1] >= self.code_at[-1] - bits))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
class Case:
    """name, plane size, a builder of the dense scan values, and the labels: what the CPU module asserts from the model"""

    def __init__(self, name, w, h, build, ll=0, **labels):
        self.name, self.w, self.h, self._build, self.ll, self.labels = name, w, h, build, ll, labels

    @functools.lru_cache(maxsize=None)
    def scan(self):
        return Scan(self.w, self.h)

    @functools.lru_cache(maxsize=None)
    def plane(self):
        sc = self.scan()
        sv = np.zeros(sc.total, dtype=np.int32)
        self._build(sc, sv)
        sv[0] = self.ll
        plane = sc.plane_of(sv)
        plane.setflags(write=False)
        return plane

    @functools.lru_cache(maxsize=None)
    def model(self):
        return Model(self.scan(), self.plane())

    def __repr__(self):
        return self.name


def _first(n, value=-1, start=1):
    """n symbols at the scan positions from `start` on"""
    def build(sc, sv):
        sv[start:start + n] = value
    return build


def _at(seg, idx, values):
    """values from position idx of subband seg on (running on into the next subbands)"""
    def build(sc, sv):
        v = np.asarray(values, dtype=np.int32)
        sv[sc.base[seg] + idx:sc.base[seg] + idx + len(v)] = v
    return build


def _all(*builders):
    def build(sc, sv):
        for b in builders:
            b(sc, sv)
    return build


def _alt(n, a, b):
    v = np.empty(n, dtype=np.int32)
    v[0::2], v[1::2] = a, b
    return v[:n]


def _laplace(n, seed, scale=1.6):
    r = np.random.RandomState(seed)
    v = np.rint(r.laplace(0.0, scale, size=n)).astype(np.int32)
    v[v == 0] = np.where(r.randint(0, 2, size=int(np.count_nonzero(v == 0))) == 0, -1, 1)
    return v


def _dense(seed, scale=1.6):
    def build(sc, sv):
        sv[:] = _laplace(sc.total, seed, scale)
    return build


def _prefix(n_ll, n_rice, value=3):
    """n_ll symbols in the LL region (from position 1), then n_rice symbols from the first subband on"""
    def build(sc, sv):
        assert n_ll < sc.base[1]
        sv[1:1 + n_ll] = _alt(n_ll, 2, -3)
        sv[sc.base[1]:sc.base[1] + n_rice] = _laplace(n_rice, 7 + n_ll, 2.5)
    return build


def _joined(pattern):
    """three chunks: one symbol of level 1 and 1023 of |v| = 128 at the finest level (the state ends on 255), the 1024 symbols of
    `pattern` at the finest level, 1024 symbols of +1"""
    assert len(pattern) == CHUNK
    return _all(_at(4, 0, [-1]), _at(7, 0, [128] * 1023 + list(pattern) + [1] * CHUNK))


def _big(values_at):
    def build(sc, sv):
        for p, v in values_at:
            sv[p] = v
    return build


def _eight_absurd(sc, sv):
    """8 x (40 symbols of -1, then 2^20) from the finest level's first position on: one chunk of 2^24 bits and more"""
    p = sc.base[7]
    for _ in range(8):
        sv[p:p + 40] = -1
        sv[p + 40] = VMAX
        p += 41


def _over_mirror(sc, sv):
    """five symbols of 2^20 at the finest level, each in a chunk of its own (1024 symbols of -1 between them): no chunk reaches 2^24
    bits, the section is 1.3 MB"""
    p = sc.base[7]
    for _ in range(5):
        sv[p] = VMAX
        sv[p + 1:p + 1 + CHUNK] = -1
        p += 1 + CHUNK


F = 7  # first subband of the finest level (damp 5); 4: of level 1 (damp 4); 1: of level 0 (damp 3)

CASES = [
    # ---- state range: flag 1 ----
    Case("dense-200-finest", 128, 128, _at(F, 0, _alt(4096, 200, -200)), flags=1, end_state=288, nch=4),
    Case("dense-64-finest", 128, 128, _at(F, 0, _alt(4096, 64, -64)), flags=0, nch=4, peak=224),  # the neighbour: bitlen(u) = 7, T = 224
    Case("dense-65-finest", 128, 128, _at(F, 0, _alt(4096, 65, -65)), flags=1, nch=4, peak=256),  # bitlen(u) = 8, T = 256: 255 / 256
    # |v| = 128 at the finest level: T = 256, the state alternates 255 / 256 from its 256th symbol on; two resp. one symbol of level 1 in
    # front of it move the chunk boundaries by one symbol: the state at symbol 1024 is 256 (flag, host) or 255 (no flag, GPU) ...
    Case("dense-128-shift2", 64, 64, _all(_at(4, 0, [-1, -1]), _at(F, 0, [128] * 2047)), flags=1, chunk_start={1: 256}, peak=256),
    Case("dense-128-shift1", 64, 64, _all(_at(4, 0, [-1]), _at(F, 0, [128] * 2047)), flags=0, chunk_start={1: 255}, peak=256),
    # ... and the state behind the plane's last chunk is looked at as well (the state's parity is that of the symbols that moved it, so
    # behind a full chunk it is what it was at the chunk's start; behind a last chunk too short for a look it is the true one):
    # 1025 symbols end on 256, 1026 on 255
    Case("dense-128-end256", 64, 64, _all(_at(4, 0, [-1]), _at(F, 0, [128] * 1024)), flags=1, chunk_start={1: 255}, end_state=256, n=1025),
    Case("dense-128-end255", 64, 64, _all(_at(4, 0, [-1]), _at(F, 0, [128] * 1025)), flags=0, chunk_start={1: 255}, end_state=255, n=1026),
    # level 1: T >= 256 needs bitlen(u) >= 16: v >= 16385 or v <= -16385 (flag 1 by k >= 32 would need vk >= 256 at level 0, T = bitlen(u) << 3 > 256:
    # bitlen(u) > 32 -- not inside |v| <= 2^20, whose bitlen(u) is 22 at most)
    Case("dense-16385-level1", 256, 128, _at(4, 0, [16385] * 1300), flags=1, chunk_start={1: 256}),
    Case("dense-16384-level1", 256, 128, _at(4, 0, [16384] * 1300), flags=0, chunk_start={1: 240}),
    # ---- join ----
    # A chunk's join only shows in the bytes of the chunks behind it: the walk that codes a chunk starts again from the state the chain
    # hands it.  So the join chunk is chunk 1, between a chunk 0 that leaves it the highest of the 256 start states (255: the one
    # trajectory a join test of hi - lo <= 2 puts on the wrong pair member) and a chunk 2 of +1 at the finest level, whose state sits
    # on 31 / 32 and whose every code therefore changes with the parity of the state it was handed.
    # (3000, -1) alternating from state 0: never joined in 1024 symbols, 3 072 512 value bits, state 0 handed on by the table alone;
    # (129, -1) the same as chunk 1, from 255
    Case("alt-3000-m1", 256, 256, _at(F, 0, list(_alt(1024, 3000, -1)) + [1] * CHUNK), flags=0, chunk_start={1: 0}, join={0: (None, None)},
         hands_on={0: ()}, chunk_value_bits={0: 3072512}),
    Case("alt-129-m1-from-255", 64, 64, _joined(_alt(1024, 129, -1)), flags=0, chunk_start={1: 255, 2: 255}, join={1: (None, None)},
         hands_on={1: ()}),
    Case("laplace-one-chunk", 64, 64, _joined(_laplace(1024, 3)), flags=0, chunk_start={1: 255}, join={1: (330, 384)},
         hands_on={1: ("swap",)}),  # small values: seen at the fifth look
    # |v| = 5 at the finest level: T = 128, every state walks towards 127 / 128; one symbol in front moves the join by one
    Case("join-at-first-look", 64, 64, _joined([-1] + [5] * 1023), flags=0, chunk_start={1: 255}, join={1: (128, 128)}, hands_on={1: ("swap",)}),
    Case("join-one-before-look", 64, 64, _joined([5] * 1024), flags=0, chunk_start={1: 255}, join={1: (127, 128)}, hands_on={1: ("swap",)}),
    Case("join-one-after-look", 64, 64, _joined([200] + [5] * 1023), flags=0, chunk_start={1: 255}, join={1: (129, 192)},
         hands_on={1: ("swap", "range2")}),
    # (129, -1) alternating keeps the 256 states apart, 156 symbols of 5 then join them at symbol 995: behind the last look (960)
    Case("join-in-last-64", 64, 64, _joined(list(_alt(868, 129, -1)) + [5] * 156), flags=0, chunk_start={1: 255}, join={1: (995, None)},
         hands_on={1: ()}),
    # 74 Rice symbols behind 950 of the LL region in chunk 0: never looked at, its table alone hands the state on
    Case("short-rice-chunk", 320, 240, _prefix(950, 1500), flags=0, join={0: (None, None)}, nskip=950, hands_on={0: ()}),
    # ---- chunk and prefix geometry ----
    Case("n0", 64, 64, _first(0), ll=-77, n=0, flags=0),
    Case("n1", 64, 64, _first(1, 5, start=70), ll=1, n=1, flags=0),
    Case("n1023", 64, 64, _first(1023, -2), n=1023, nch=1, flags=0),
    Case("n1024", 64, 64, _first(1024, -2), n=1024, nch=1, flags=0),
    Case("n1025", 64, 64, _first(1025, -2), n=1025, nch=2, flags=0),
    Case("n2048", 64, 64, _first(2048, 3), ll=300, n=2048, nch=2, flags=0),
    Case("ll-only", 64, 64, _first(63, -9), n=63, nskip=63, flags=0),
    Case("prefix-16", 64, 64, _prefix(16, 1500), nskip=16, flags=0),   # = 0 mod 4 and mod 16
    Case("prefix-17", 64, 64, _prefix(17, 1500), nskip=17, flags=0),
    Case("prefix-18", 64, 64, _prefix(18, 1500), nskip=18, flags=0),
    Case("prefix-19", 64, 64, _prefix(19, 1500), nskip=19, flags=0),
    Case("prefix-15", 64, 64, _prefix(15, 1500), nskip=15, flags=0),   # = 15 mod 16
    Case("prefix-1024", 320, 240, _prefix(1024, 1500), nskip=1024, flags=0),
    Case("prefix-1100", 320, 240, _prefix(1100, 1500), nskip=1100, flags=0),
    Case("last-position", 64, 64, _big([(64 * 64 - 1, -4)]), n=1, run_len={0: 2 * 12 + 1}, flags=0),
    Case("subband-firsts", 64, 64, lambda sc, sv: sv.__setitem__(sc.base[1:10], [3, -1, 7, 1, -2, 40, -1, 1, 2]), n=9, flags=0),
    Case("empty-subband", 64, 64, _all(_at(4, 0, [2] * 256), _at(6, 0, [-3] * 256)), n=512, flags=0),
    Case("odd-50x38", 50, 38, _dense(11), flags=0),
    Case("dense-256x160", 256, 160, _dense(5), flags=0, min_nch=33),
    Case("dense-320x240", 320, 240, _dense(6, 2.2), ll=-1000, flags=0, min_nch=65),
    # ---- code lengths ----
    Case("lone-30000", 64, 64, _at(F, 0, [-1] * 300 + [30000]), flags=0, val_len={300: 59999 + 1}, straddle=1),
    Case("value-40", 64, 64, _at(1, 0, [-1, 20, -1, -1]), flags=0, val_len={1: 40}),
    Case("value-41", 64, 64, _at(1, 0, [-1, -21, -1, -1]), flags=0, val_len={1: 41}),
    Case("value-run-64", 256, 192, _all(_at(F, 0, [-1, -17]), _at(F, 2 + 32767, [-1, -1])), flags=0, val_run_len={1: 64}),
    Case("value-run-65", 256, 192, _all(_at(F, 0, [-1, 17]), _at(F, 2 + 32767, [-1, -1])), flags=0, val_run_len={1: 65}),
    Case("run-1-and-31", 256, 192, _all(_at(F, 0, [2, 2]), _at(F, 2 + 65534 // 2, [2])), flags=0, run_len={1: 1, 2: 31}),
    Case("run-max-640x480", 640, 480, _big([(640 * 480 - 1, 1)]), flags=0, run_len={0: 2 * 18 + 1}),
    Case("flip-k", 64, 64, _all(_at(1, 0, [1] * 192), _at(4, 0, [1] * 768), _at(F, 0, [1] * 3072)), flags=0, flips={0: 150, 1: 700, 2: 3000}),
    Case("flip-k-16", 64, 64, _at(1, 0, [-2] * 192), flags=0, flips={0: 150}),
    Case("floor-0", 64, 64, _at(1, 0, [-1] * 2000), flags=0, peak=0),
    Case("short-codes-in-tail", 64, 64, _at(F, 0, [9] * 200 + [-1] * 400), flags=0, tail=100),
    # ---- big sections ----
    Case("absurd-chunk-640x480", 640, 480, _eight_absurd, flags=4, value_bits=16777536),
    Case("over-mirror-640x480", 640, 480, _over_mirror, flags=8, min_bytes=MIRROR + 1),
    # flag 2 (a section larger than the seam's buffer, ent_out_bytes = 4 MiB for every plane of 8 Mi coefficients or fewer) is out of
    # reach: the reference's decoder refuses a section of cw * ch * 8 bytes or more (hzcc.c:627), 2 457 600 at 640 x 480 -- the buffer
    # is the smaller of the two only from 524 288 coefficients on, and a section above 4 MiB of such a plane is not a test input
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the planes every case runs as: the coder's plane 0, 1 and 2 differ in where their symbols and chunks sit in the job's tables
GEOMETRY_CASES = ["n0", "n1", "n1023", "n1024", "n1025", "n2048", "ll-only", "prefix-16", "prefix-17", "prefix-18", "prefix-19", "prefix-15",
                  "prefix-1024", "prefix-1100", "last-position", "subband-firsts", "empty-subband", "dense-256x160", "dense-320x240",
                  "dense-128-shift2", "join-one-after-look"]
# the byte offsets a section is placed at, with nonzero bytes in front
OFFSETS = [0, 1, 3, 13]
OFFSET_CASES = ["n1", "prefix-19", "lone-30000", "laplace-one-chunk", "short-codes-in-tail", "dense-128-shift2"]


# ---- the stage seam, as both test modules call it (the reference and the library share the signatures) ------------------------------
def _fmeta(case, plane):
    meta = A.mk_meta(case.w, case.h, A.SUBSAMP_444)  # (4:4:4: a plane of any index has the picture's size)
    params = A.mk_params(meta, case.w, case.h, 0, lossless=1)
    nb = params.nblocks_h * params.nblocks_v
    keep = [meta, params, np.zeros(nb, dtype=np.uint8), np.zeros(nb, dtype=A.MV_DTYPE)]
    fm = A.FMETA()
    fm.params = C.pointer(params)
    fm.blockdata = A.np_ptr(keep[2], C.c_uint8)
    fm.mvs = C.cast(keep[3].ctypes.data, C.POINTER(A.MV))
    fm.cur_plane, fm.isP = plane, 0
    return fm, keep


LEAD = 0xC3  # what stands in front of a section that does not start at byte 0


def buffer_bytes(case):
    return plane_bitstream_bytes(case.w, case.h)


def encode_plane(lib, case, plane=0, offset=0):
    """dsv_encode_plane of the case's coefficients at byte `offset` of a zeroed buffer: (the whole buffer, bs.pos, the coefficients behind)"""
    coefs = np.array(case.plane())
    out = np.zeros(buffer_bytes(case), dtype=np.uint8)
    out[:offset] = LEAD
    bs = A.BS(A.np_ptr(out, C.c_uint8), offset * 8)
    cs = A.COEFS(A.np_ptr(coefs, C.c_int32), case.w, case.h)
    fm, keep = _fmeta(case, plane)
    lib.dsv_encode_plane(C.byref(bs), C.byref(cs), 1, C.byref(fm))
    return out, bs.pos, coefs


def decode_plane(lib, buf, case, plane=0, offset=0, fill=0):
    """dsv_decode_plane of the section at byte `offset` of buf into a plane that holds `fill`: (return value, bs.pos, the plane)"""
    buf = np.array(buf)
    coefs = np.full(case.w * case.h, fill, dtype=np.int32)
    bs = A.BS(A.np_ptr(buf, C.c_uint8), offset * 8)
    cs = A.COEFS(A.np_ptr(coefs, C.c_int32), case.w, case.h)
    fm, keep = _fmeta(case, plane)
    ok = lib.dsv_decode_plane(C.byref(bs), C.byref(cs), 1, C.byref(fm))
    return ok, bs.pos, coefs
