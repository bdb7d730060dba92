"""A FLAC reader written from the specification (RFC 9639), for the tests: mono, 16-bit, fixed-blocksize streams as the encoder writes them.

It parses STREAMINFO and every frame, checks each frame header's CRC-8 and each frame's CRC-16, checks the streamable-subset limits the
encoder promises (block size <= 4608 and 4096 here, LPC order <= 12, Rice partition order <= 8, rate and bit depth coded in the frame header),
and decodes CONSTANT, VERBATIM, FIXED and LPC subframes with Rice-coded partitioned residuals; the bits between a subframe's end and the
byte boundary must be zero (RFC 9639, 9.3).  numpy + Python only."""
import numpy as np

RATE_CODES = {8000: 0b0100, 16000: 0b0101, 22050: 0b0110, 24000: 0b0111, 32000: 0b1000, 44100: 0b1001, 48000: 0b1010}
CODE_RATES = {v: k for k, v in RATE_CODES.items()}


class FlacError(ValueError):
    pass


def crc8(data) -> int:
    """CRC-8 of the frame header: polynomial 0x07, init 0, MSB first."""
    c = 0
    for b in bytes(data):
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


_POW16 = [1]


def _x_pow_mod(n):
    """x^j mod (x^16 + x^15 + x^2 + 1) for j < n, as an int array."""
    while len(_POW16) < n:
        v = _POW16[-1] << 1
        if v & 0x10000:
            v ^= 0x18005
        _POW16.append(v)
    return np.asarray(_POW16[:n], np.int64)


def crc16(data) -> int:
    """CRC-16 of a frame: polynomial 0x8005, init 0, MSB first, i.e. M(x) x^16 mod P(x): the xor of x^(16 + j) mod P over the set bits of
    the message, j counted from its last bit."""
    bits = np.unpackbits(np.frombuffer(bytes(data), np.uint8))
    if bits.size == 0:
        return 0
    pw = _x_pow_mod(bits.size + 16)
    j = bits.size - 1 - np.flatnonzero(bits) + 16
    return int(np.bitwise_xor.reduce(pw[j])) if j.size else 0


class _Bits:
    def __init__(self, data: bytes, pos_bits: int = 0):
        self.b = np.unpackbits(np.frombuffer(data, np.uint8))
        self.ones = np.flatnonzero(self.b)
        self.pos = pos_bits

    def u(self, n):
        if self.pos + n > self.b.size:
            raise FlacError("read past the end of the stream")
        v = 0
        for bit in self.b[self.pos:self.pos + n].tolist():
            v = (v << 1) | bit
        self.pos += n
        return v

    def s(self, n):
        v = self.u(n)
        return v - (1 << n) if v >> (n - 1) else v

    def unary(self):
        i = int(np.searchsorted(self.ones, self.pos))
        if i >= self.ones.size:
            raise FlacError("unterminated unary code")
        q = int(self.ones[i]) - self.pos
        self.pos += q + 1
        return q


FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def _utf8(r: _Bits):
    b0 = r.u(8)
    if b0 < 0x80:
        return b0
    n = 0
    while b0 & (0x80 >> n):
        n += 1
    if n < 2 or n > 7:
        raise FlacError("bad UTF-8 frame number")
    v = b0 & (0xFF >> (n + 1))
    for _ in range(n - 1):
        c = r.u(8)
        if c >> 6 != 0b10:
            raise FlacError("bad UTF-8 continuation byte")
        v = (v << 6) | (c & 0x3F)
    return v


def _residual(r: _Bits, n, order, info):
    method = r.u(2)
    if method != 0:
        raise FlacError(f"residual coding method {method} (the encoder writes 0: 4-bit Rice parameters)")
    p = r.u(4)
    if p > 8:
        raise FlacError(f"partition order {p} > 8 (streamable subset)")
    if n % (1 << p) or (n >> p) <= order:
        raise FlacError(f"invalid partition order {p} for block {n}, order {order}")
    info["p"] = p
    res, ks = [], []
    for part in range(1 << p):
        k = r.u(4)
        if k == 15:
            raise FlacError("escaped partition (the encoder never writes one)")
        ks.append(k)
        for _ in range((n >> p) - (order if part == 0 else 0)):
            q = r.unary()
            u = (q << k) | r.u(k) if k else q
            res.append((u >> 1) ^ -(u & 1))
    info["k"] = ks
    info["res"] = np.asarray(res, np.int64)
    return res


def _subframe(r: _Bits, n):
    if r.u(1):
        raise FlacError("subframe padding bit set")
    t = r.u(6)
    if r.u(1):
        raise FlacError("wasted bits (the encoder never writes them)")
    info = {}
    if t == 0:
        info["type"] = "CONSTANT"
        return [r.s(16)] * n, info
    if t == 1:
        info["type"] = "VERBATIM"
        return [r.s(16) for _ in range(n)], info
    if 8 <= t <= 12:
        order = t - 8
        info.update(type="FIXED", order=order)
        x = [r.s(16) for _ in range(order)]
        coef, shift = FIXED[order], 0
    elif t >= 32:
        order = t - 31
        if order > 12:
            raise FlacError(f"LPC order {order} > 12 (streamable subset)")
        x = [r.s(16) for _ in range(order)]
        prec = r.u(4) + 1
        if prec == 16:
            raise FlacError("invalid coefficient precision")
        shift = r.s(5)
        if shift < 0:
            raise FlacError("negative LPC shift")
        coef = [r.s(prec) for _ in range(order)]
        info.update(type="LPC", order=order, precision=prec, shift=shift, coef=coef)
    else:
        raise FlacError(f"reserved subframe type {t}")
    res = _residual(r, n, order, info)
    # x[i] = e[i] + (sum_j coef[j] x[i - 1 - j]) >> shift, coef[0] multiplying the sample right before x[i]
    for i, e in enumerate(res, start=order):
        acc = 0
        for j, c in enumerate(coef):
            acc += c * x[i - 1 - j]
        x.append(e + (acc >> shift))
    return x, info


def read(data: bytes):
    """-> dict(rate, total, min_block, max_block, min_frame, max_frame, md5, samples (int16), frames = [dict(size, n, number, header, type,
    bits = the subframe's length in bits from its first bit to the end of its last residual code; FIXED and LPC: order, p, k = [per
    partition], res = the decoded residuals (int64 array); LPC: precision, shift, coef)])."""
    data = bytes(data)
    if data[:4] != b"fLaC":
        raise FlacError("no fLaC marker")
    if data[4] != 0x80 or int.from_bytes(data[5:8], "big") != 34:
        raise FlacError("expected exactly one metadata block: a last STREAMINFO of 34 bytes")
    si = data[8:42]
    out = dict(min_block=int.from_bytes(si[0:2], "big"), max_block=int.from_bytes(si[2:4], "big"), min_frame=int.from_bytes(si[4:7], "big"),
               max_frame=int.from_bytes(si[7:10], "big"), md5=si[18:34])
    v = int.from_bytes(si[10:18], "big")
    out["rate"], ch, bps, out["total"] = v >> 44, (v >> 41) & 7, ((v >> 36) & 31) + 1, v & ((1 << 36) - 1)
    if ch != 0 or bps != 16:
        raise FlacError(f"not mono 16-bit: channels {ch + 1}, bits {bps}")
    if out["max_block"] > 4608:
        raise FlacError("block size beyond the streamable subset")
    pos, samples, frames = 42, [], []
    r = _Bits(data)
    while pos < len(data):
        r.pos = 8 * pos
        if r.u(16) != 0xFFF8:
            raise FlacError(f"no fixed-blocksize frame sync at byte {pos}")
        bs, rc = r.u(4), r.u(4)
        chan, size, res = r.u(4), r.u(3), r.u(1)
        if chan != 0 or size != 0b100 or res:
            raise FlacError("frame header: not mono 16-bit, or reserved bit set")
        if rc not in CODE_RATES or CODE_RATES[rc] != out["rate"]:
            raise FlacError(f"frame rate code {rc:04b} does not code the stream's rate {out['rate']} in the header")
        number = _utf8(r)
        if bs == 0b1100:
            n = 4096
        elif bs == 0b0110:
            n = r.u(8) + 1
        elif bs == 0b0111:
            n = r.u(16) + 1
        else:
            raise FlacError(f"unexpected block size code {bs:04b}")
        hlen = r.pos // 8 - pos
        if crc8(data[pos:pos + hlen]) != r.u(8):
            raise FlacError(f"frame {number}: header CRC-8 mismatch")
        sub = r.pos
        x, info = _subframe(r, n)
        info["bits"] = r.pos - sub
        if r.u(-r.pos % 8):
            raise FlacError(f"frame {number}: a padding bit before the byte boundary is set")
        end = r.pos // 8
        if end + 2 > len(data):
            raise FlacError("truncated frame")
        if crc16(data[pos:end]) != int.from_bytes(data[end:end + 2], "big"):
            raise FlacError(f"frame {number}: CRC-16 mismatch")
        info.update(size=end + 2 - pos, n=n, number=number, header=hlen + 1)
        if number != len(frames):
            raise FlacError(f"frame number {number}, expected {len(frames)}")
        frames.append(info)
        samples.extend(x)
        pos = end + 2
    out["frames"] = frames
    s = np.asarray(samples, np.int64)
    if s.size and (s.min() < -32768 or s.max() > 32767):
        raise FlacError("decoded samples outside 16 bits")
    out["samples"] = s.astype(np.int16)
    if out["total"] != s.size:
        raise FlacError(f"STREAMINFO total {out['total']} != decoded {s.size}")
    return out
