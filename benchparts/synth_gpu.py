"""bench.py, the headline's pictures made on the GPU: the same bytes as digital-subband-video-2_amd/synth.py (SynthVideo), in torch.

The package's generator is numpy on the host: about a second per 1080p video for its canvas and 50 ms per frame, i.e. minutes of
host CPU for the headline's 96 videos x 64 frames.  This module repeats its integer arithmetic op for op on the device, so a
plain benchmark run spends its set-up on the encode rather than on making pictures.  tests/test_bench_synth.py holds the two
generators byte-equal.  Every product of two 32-bit values is formed in 16-bit halves, so no int64 intermediate overflows."""
import numpy as np

from conftest import load_pkg

_M32 = 0xFFFFFFFF
_M16 = 0xFFFF


def _mul32(a, c):
    """(a * c) mod 2^32 for int64 tensors a in [0, 2^32) and a Python int c in [0, 2^32)"""
    return ((a & _M16) * c + ((((a >> 16) * c) & _M16) << 16)) & _M32


def _hash_xy(torch, h, w, dev):
    """the coordinate part of synth._hash2d, which every seed shares"""
    y = torch.arange(h, dtype=torch.int64, device=dev)[:, None]
    x = torch.arange(w, dtype=torch.int64, device=dev)[None, :]
    return _mul32(x, 73856093) ^ _mul32(y, 19349663)


def _hash_seed(v, seed):
    """synth._hash2d from its coordinate part v; seed = an int, or an int64 tensor that broadcasts against v (one hash per seed)"""
    v = v ^ ((seed * 83492791) & _M32)
    v = (_mul32(v, 1103515245) + 12345) & _M32
    v ^= v >> 15
    v = _mul32(v, 2246822519)
    v ^= v >> 13
    v = _mul32(v, 3266489917)
    v ^= v >> 16
    return v


def _box_blur(torch, a, r):
    """synth._box_blur: (2r+1)^2 box mean with edge clamp, integer, via cumulative sums"""
    h, w = a.shape
    dev = a.device
    iy = torch.arange(-r, h + r, device=dev).clamp_(0, h - 1)
    ix = torch.arange(-r, w + r, device=dev).clamp_(0, w - 1)
    p = a.to(torch.int64)[iy][:, ix]
    c = torch.nn.functional.pad(torch.cumsum(torch.cumsum(p, 0), 1), (1, 0, 1, 0))
    k = 2 * r + 1
    s = c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]
    return torch.div(s, k * k, rounding_mode="floor")


class DeviceVideo:
    """One synthetic video of `nf` frames, made on `dev` when generate() is called; len() is the frame count and P the bytes of
    one frame, as EncodeRun reads them from a list of frames."""

    def __init__(self, width, height, subsamp, seed, nf, dev="cuda"):
        self.w, self.h, self.subsamp, self.seed, self.nf, self.dev = width, height, subsamp, seed, nf, dev
        self.cw = width // 2 if subsamp == "420" else width
        self.ch = height // 2 if subsamp == "420" else height
        self.P = width * height + 2 * self.cw * self.ch

    def __len__(self):
        return self.nf

    def _squares(self):
        """the six squares exactly as SynthVideo.__init__ draws them (a 6 x 8 hash: host numpy)"""
        synth = load_pkg().synth
        w, h = self.w, self.h
        sq = max(16, (96 * h) // 1080 // 2 * 2)
        hs = synth._hash2d(6, 8, self.seed + 77)
        out = []
        for k in range(6):
            x0 = int(hs[k, 0] % np.uint32(max(1, w - sq)))
            y0 = int(hs[k, 1] % np.uint32(max(1, h - sq)))
            vx = int(hs[k, 2] % np.uint32(9)) - 4
            vy = int(hs[k, 3] % np.uint32(7)) - 3
            if vx == 0 and vy == 0:
                vx = 1
            lum = (6, 250, 40 + int(hs[k, 4] % np.uint32(180)))[k % 3]
            cu = 64 + int(hs[k, 5] % np.uint32(128))
            cv = 64 + int(hs[k, 6] % np.uint32(128))
            out.append((x0, y0, vx, vy, lum, cu, cv))
        return sq, out

    def generate(self, torch, out=None, chunk=16):
        """all frames as one (nf, P) uint8 tensor on the device (written into `out` when given); the per-pixel terms of `chunk`
        frames are made at once, the moving squares frame by frame"""
        w, h, cw, ch, dev, pad = self.w, self.h, self.cw, self.ch, self.dev, 256
        assert w % 2 == 0 and h % 2 == 0
        i32, i64 = torch.int32, torch.int64
        n = (_hash_seed(_hash_xy(torch, 2 * h + 2 * pad, 2 * w + 2 * pad, dev), self.seed) >> 24).to(i32)
        lo, mid = _box_blur(torch, n, 6), _box_blur(torch, n, 1)
        canvas = torch.clamp(128 + (lo - 128) * 6 + torch.div(mid - 128, 3, rounding_mode="floor"), 16, 240).to(i32)
        sq, squares = self._squares()
        tri = torch.tensor(load_pkg().synth._TRI, dtype=i32, device=dev)
        hxy = _hash_xy(torch, h, w, dev)
        yy = torch.arange(h, dtype=i32, device=dev)[:, None]
        xx = torch.arange(w, dtype=i32, device=dev)[None, :]
        cyy = torch.arange(ch, dtype=i32, device=dev)[:, None]
        cxx = torch.arange(cw, dtype=i32, device=dev)[None, :]
        sc = w // cw
        sy, sx = h // ch, w // cw
        c0 = canvas[pad:pad + 2 * h, pad:pad + 2 * (w // 4)]
        left = (c0[0::2, 0::2] + c0[0::2, 1::2] + c0[1::2, 0::2] + c0[1::2, 1::2] + 2) >> 2
        sinus_left = tri[(((xx[:, :w // 4] * 3 + yy) >> 2) & 63).long()]
        u_y = tri[(((cyy * sc) >> 4) & 63).long()]
        v_x = tri[(((cxx * sc) >> 4) & 63).long()]
        if out is None:
            out = torch.empty((self.nf, self.P), dtype=torch.uint8, device=dev)
        for t0 in range(0, self.nf, chunk):
            t1 = min(self.nf, t0 + chunk)
            tt = torch.arange(t0, t1, dtype=i64, device=dev)[:, None, None]
            noise = (_hash_seed(hxy, self.seed * 1000 + 17 + tt) % 5).to(i32) - 2
            noise[:, :, :w // 2] = 0
            sinus = tri[(((xx * 3 + yy + 2 * tt.to(i32)) >> 2) & 63).long()]
            sinus[:, :, :w // 4] = sinus_left
            Y = sinus + noise
            U = (128 + tri[(((cxx * sc + 2 * tt.to(i32)) >> 3) & 63).long()] * 2 + u_y).expand(t1 - t0, ch, cw).clone()
            V = (128 + tri[(((cyy * sc + 3 * tt.to(i32)) >> 3) & 63).long()] * 2 - v_x).expand(t1 - t0, ch, cw).clone()
            for t in range(t0, t1):
                j = t - t0
                ox, oy = pad + (3 * t) % pad, pad + (2 * t) % pad
                c = canvas[oy:oy + 2 * h, ox:ox + 2 * w]
                tex = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2
                tex[:, :w // 4] = left
                Y[j] += tex
                for (x0, y0, vx, vy, lum, cu, cv) in squares:
                    span_x, span_y = w - sq, h - sq
                    px = (x0 + vx * t) % (2 * span_x) if span_x > 0 else 0
                    py = (y0 + vy * t) % (2 * span_y) if span_y > 0 else 0
                    if px >= span_x:
                        px = 2 * span_x - px
                    if py >= span_y:
                        py = 2 * span_y - py
                    Y[j, py:py + sq, px:px + sq] = lum + (noise[j, py:py + sq, px:px + sq] >> 1)
                    U[j, py // sy:(py + sq) // sy, px // sx:(px + sq) // sx] = cu
                    V[j, py // sy:(py + sq) // sy, px // sx:(px + sq) // sx] = cv
            rows = out[t0:t1]
            rows[:, :w * h].view(t1 - t0, h, w).copy_(Y.clamp_(0, 255))
            rows[:, w * h:w * h + cw * ch].view(t1 - t0, ch, cw).copy_(U.clamp_(0, 255))
            rows[:, w * h + cw * ch:].view(t1 - t0, ch, cw).copy_(V.clamp_(0, 255))
        return out
