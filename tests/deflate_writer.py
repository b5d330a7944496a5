"""A deflate / zlib / PNG writer under the test's control (RFC 1950, RFC 1951, PNG 9.2), and the corpus built with it.

zlib and libpng write one dialect of deflate; the PNG decoder on the device has only ever been shown that dialect.  This
writer emits a bit stream exactly as told: stored, fixed and dynamic blocks from explicit token lists, explicit code
lengths, an explicit run-length coding of a dynamic header, and escape hatches for the streams that must be refused.
It reports where every block header and every token starts, and the bytes the stream expands to, so that the tests
can assert what a stream covers instead of hoping.

Nothing here is fast or clever: plain Python, one bit field at a time.
"""
import struct
import zlib

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def len_symbol(n, prefer=None):
    """(symbol, extra value) for match length n; `prefer` picks between the two ways to write 258 (285, or 284 + 31)."""
    if prefer is not None:
        c = prefer - 257
        assert 0 <= n - LEN_BASE[c] < (1 << LEN_EXTRA[c]), (n, prefer)
        return prefer, n - LEN_BASE[c]
    if n == 258:
        return 285, 0
    c = max(i for i in range(28) if LEN_BASE[i] <= n)
    return 257 + c, n - LEN_BASE[c]


def dist_symbol(d):
    c = max(i for i in range(30) if DIST_BASE[i] <= d)
    return c, d - DIST_BASE[c]


def canonical(lens):
    """Canonical codes (RFC 1951 3.2.2) of a length array; an over-subscribed array still gets codes (masked to their
    length) so that invalid headers can be followed by data."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l:
            out.append(nxt[l] & ((1 << l) - 1))
            nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft(lens):
    """Sum of 2^-len in units of 2^-15: 32768 is a complete code."""
    return sum(1 << (15 - l) for l in lens if l)


def complete_lengths(rng, n, maxbits=15):
    """n code lengths of a complete prefix code: random leaf splits of the one-leaf tree."""
    if n == 1:
        return [1]
    leaves = [1, 1]
    while len(leaves) < n:
        can = [i for i, l in enumerate(leaves) if l < maxbits]
        i = can[int(rng.integers(len(can)))]
        l = leaves.pop(i)
        leaves += [l + 1, l + 1]
    rng.shuffle(leaves)
    return [int(l) for l in leaves]


def rle_lengths(lens):
    """A plain run-length coding of a code-length array into code-length symbols (sym, repeat count or None)."""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            take = min(run, 138)
            out.append((18, take) if take >= 11 else (17, take))
            i += take
        elif v and run >= 4:
            out.append((v, None))
            take = min(run - 1, 6)
            out.append((16, take))
            i += 1 + take
        else:
            out.append((v, None))
            i += 1
    return out


def cl_lengths_for(cl_syms):
    """Lengths (<= 7 bits) of a complete code-length code for the symbols in use; a second symbol is added when only one is
    in use, since zlib wants this code complete."""
    used = sorted({s for s, _ in cl_syms})
    if len(used) == 1:
        used.append(0 if used[0] else 1)
    k = len(used)
    b = max(1, (k - 1).bit_length())
    short = (1 << b) - k
    freq = {s: sum(1 for t, _ in cl_syms if t == s) for s in used}
    order = sorted(used, key=lambda s: -freq[s])
    lens = [0] * 19
    for i, s in enumerate(order):
        lens[s] = b - 1 if i < short else b
    return lens


class Bits:
    def __init__(self):
        self.out, self.acc, self.cnt = bytearray(), 0, 0

    @property
    def pos(self):
        return len(self.out) * 8 + self.cnt

    def put(self, v, n):
        """n bits of v, least significant first (header fields and extra bits)."""
        self.acc |= (v & ((1 << n) - 1)) << self.cnt
        self.cnt += n
        while self.cnt >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.cnt -= 8

    def code(self, c, n):
        """A Huffman code of n bits, most significant first."""
        r = 0
        for _ in range(n):
            r = r << 1 | (c & 1)
            c >>= 1
        self.put(r, n)

    def align(self, ones=False):
        if self.cnt:
            n = 8 - self.cnt
            self.put((1 << n) - 1 if ones else 0, n)

    def raw(self, b):
        assert self.cnt == 0
        self.out += b


class Sym:
    """A literal/length symbol written as is, with the bits that follow it: the low-level token (what the others become)."""
    def __init__(self, ll, ll_extra=0, d=None, d_extra=0):
        self.ll, self.ll_extra, self.d, self.d_extra = ll, ll_extra, d, d_extra


class RawBits:
    """Bits put into a block's data as they stand: [(value, nbits), ...], least significant first."""
    def __init__(self, fields):
        self.fields = fields


class Stream:
    """One zlib stream.  Positions in the report are bit positions in the zlib stream (the deflate data begins at 16)."""

    def __init__(self, cmf=0x78, flg=0x01):
        self.b = Bits()
        self.b.raw(bytes([cmf, flg]))
        self.out = bytearray()       # what a decoder produces
        self.blocks = []             # {kind, bit, sym_bit, end_bit, out0, final, tokens: [(bit, nbits, ll symbol, d symbol, out position behind it, len, dist)]}
        self.bad_distance = False

    # -- tokens ------------------------------------------------------------------------------------------------------
    def _tokens(self, blk, tokens, ll_lens, d_lens, eob):
        ll_codes, d_codes = canonical(ll_lens), canonical(d_lens)
        b, out = self.b, self.out
        for t in tokens:
            if isinstance(t, RawBits):
                for v, n in t.fields:
                    b.put(v, n)
                continue
            if isinstance(t, int):
                t = Sym(t)
            elif isinstance(t, tuple):
                ls, lx = len_symbol(t[0], t[2] if len(t) > 2 else None)
                ds, dx = dist_symbol(t[1])
                t = Sym(ls, lx, ds, dx)
            p0, n, dist = b.pos, 0, 0
            assert ll_lens[t.ll], ("symbol without a code", t.ll)
            b.code(ll_codes[t.ll], ll_lens[t.ll])
            if t.ll < 256:
                out.append(t.ll)
            elif t.ll > 256:
                c = t.ll - 257
                if c < 29:
                    b.put(t.ll_extra, LEN_EXTRA[c])
                    n = LEN_BASE[c] + t.ll_extra
                if t.d is not None:
                    assert d_lens[t.d], ("distance without a code", t.d)
                    b.code(d_codes[t.d], d_lens[t.d])
                    if t.d < 30 and c < 29:
                        b.put(t.d_extra, DIST_EXTRA[t.d])
                        dist = DIST_BASE[t.d] + t.d_extra
                        if dist > len(out):
                            self.bad_distance = True
                        elif dist >= n:
                            out += out[len(out) - dist:len(out) - dist + n]
                        else:
                            for _ in range(n):
                                out.append(out[-dist])
            blk["tokens"].append((p0, b.pos - p0, t.ll, t.d, len(out), n, dist))
        if eob:
            blk["eob_bit"] = b.pos
            b.code(ll_codes[256], ll_lens[256])
        blk["end_bit"] = b.pos

    def _open(self, kind, final, btype):
        blk = {"kind": kind, "bit": self.b.pos, "out0": len(self.out), "final": final, "tokens": []}
        self.blocks.append(blk)
        self.b.put(1 if final else 0, 1)
        self.b.put(btype, 2)
        return blk

    # -- blocks ------------------------------------------------------------------------------------------------------
    def stored(self, data, final=False, pad_ones=False, len_field=None, nlen_field=None, btype=0):
        blk = self._open("stored", final, btype)
        self.b.align(pad_ones)
        n = len(data) if len_field is None else len_field
        self.b.raw(struct.pack("<HH", n, (n ^ 0xffff) if nlen_field is None else nlen_field))
        blk["sym_bit"] = self.b.pos
        self.b.raw(bytes(data))
        self.out += data
        blk["end_bit"] = self.b.pos
        return blk

    def fixed(self, tokens, final=False, eob=True, btype=1):
        blk = self._open("fixed", final, btype)
        blk["sym_bit"] = self.b.pos
        self._tokens(blk, tokens, FIXED_LL, FIXED_D, eob)
        return blk

    def dynamic(self, tokens, ll_lens, d_lens, final=False, eob=True, btype=2, hlit=None, hdist=None, hclen=None, cl_lens=None,
                cl_syms=None, hlit_field=None, hdist_field=None):
        """ll_lens / d_lens: {symbol: length} or arrays.  hlit / hdist: how many lengths the header carries (default: up to the
        last one in use); cl_syms: the header's code-length symbols [(0..15, None) | (16 | 17 | 18, repeat)]; cl_lens: the 19
        lengths of the code-length code; hclen: how many of them are sent; *_field: the raw 5-bit header fields."""
        def arr(x, n):
            if isinstance(x, dict):
                a = [0] * n
                for s, l in x.items():
                    a[s] = l
                return a
            return list(x) + [0] * (n - len(x))
        ll, dd = arr(ll_lens, 288), arr(d_lens, 32)
        if hlit is None:
            hlit = max(257, max((i + 1 for i in range(288) if ll[i]), default=257))
        if hdist is None:
            hdist = max(1, max((i + 1 for i in range(32) if dd[i]), default=1))
        if cl_syms is None:
            cl_syms = rle_lengths(ll[:hlit] + dd[:hdist])
        if cl_lens is None:
            cl_lens = cl_lengths_for(cl_syms)
        if hclen is None:
            hclen = max(4, max(i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]))
        blk = self._open("dynamic", final, btype)
        b = self.b
        b.put((hlit - 257) if hlit_field is None else hlit_field, 5)
        b.put((hdist - 1) if hdist_field is None else hdist_field, 5)
        b.put(hclen - 4, 4)
        for i in range(hclen):
            b.put(cl_lens[CL_ORDER[i]], 3)
        cl_codes = canonical(cl_lens)
        for s, rep in cl_syms:
            assert cl_lens[s], ("code-length symbol without a code", s)
            b.code(cl_codes[s], cl_lens[s])
            if s == 16:
                b.put(rep - 3, 2)
            elif s == 17:
                b.put(rep - 3, 3)
            elif s == 18:
                b.put(rep - 11, 7)
        blk.update(sym_bit=b.pos, hlit=hlit, hdist=hdist, hclen=hclen, cl_syms=list(cl_syms), cl_lens=list(cl_lens), ll=ll, dd=dd)
        self._tokens(blk, tokens, ll, dd, eob)
        return blk

    def bits(self, fields):
        for v, n in fields:
            self.b.put(v, n)

    # -- the end -----------------------------------------------------------------------------------------------------
    def finish(self, adler=None, trailer=True):
        """-> the zlib stream.  adler: a value to write instead of the right one; trailer=False: none at all."""
        self.end_bit = self.b.pos
        self.b.align()
        if trailer:
            self.b.raw(struct.pack(">I", zlib.adler32(bytes(self.out)) if adler is None else adler))
        return bytes(self.b.out)


# ---- PNG --------------------------------------------------------------------------------------------------------------
def chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))


def png_file(z, w, h, ctype, plte=None, idat_split=None):
    """An 8-bit PNG of colour type ctype (0 grey, 2 RGB, 3 palette, 4 grey + alpha, 6 RGBA) around a zlib stream."""
    parts = [z] if not idat_split else [z[i:i + idat_split] for i in range(0, len(z), idat_split)]
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, ctype, 0, 0, 0)) +
            (chunk(b"PLTE", bytes(plte)) if plte is not None else b"") + b"".join(chunk(b"IDAT", p) for p in parts) +
            chunk(b"IEND", b""))


def _predict(ft, cur_a, up, c):
    if ft == 0:
        return 0
    if ft == 1:
        return cur_a
    if ft == 2:
        return up
    if ft == 3:
        return (cur_a + up) >> 1
    p = cur_a + up - c
    pa, pb, pc = abs(p - cur_a), abs(p - up), abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), cur_a, np.where(pb <= pc, up, c))


def filter_rows(img, bpp, ftypes):
    """img: [h, row bytes] integers; ftypes: the filter type of every row.  -> the filtered bytes (PNG 9.2)."""
    img = np.asarray(img).astype(np.int32)
    rows = []
    for y in range(img.shape[0]):
        ft = ftypes[y]
        cur, up = img[y], (img[y - 1] if y else np.zeros_like(img[0]))
        a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if len(cur) > bpp else np.zeros_like(cur)
        c = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]]) if len(cur) > bpp else np.zeros_like(cur)
        rows.append(bytes([ft]) + ((cur - _predict(ft, a, up, c)) & 255).astype(np.uint8).tobytes())
    return b"".join(rows)


def unfilter(raw, h, row, bpp):
    """The integer model of PNG 9.2 reconstruction: filtered bytes (h rows of 1 + row) -> [h, row] uint8, or None where a
    filter type is not 0..4.  Average and Paeth run along the row, so this one is a loop per byte."""
    raw = np.frombuffer(bytes(raw), np.uint8).reshape(h, row + 1)
    out = np.zeros((h, row), np.int32)
    zero = np.zeros(row, np.int32)
    for y in range(h):
        ft = int(raw[y, 0])
        x = raw[y, 1:].astype(np.int32)
        up = out[y - 1] if y else zero
        if ft > 4:
            return None
        if ft == 0:
            out[y] = x
        elif ft == 2:
            out[y] = (x + up) & 255
        elif ft == 1:
            cur = x.reshape(-1, bpp).copy() if row % bpp == 0 else None
            out[y] = (np.cumsum(cur, axis=0) & 255).reshape(-1)
        else:
            cur = [0] * row
            upl = up.tolist()
            xl = x.tolist()
            for i in range(row):
                a = cur[i - bpp] if i >= bpp else 0
                b = upl[i]
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    c = upl[i - bpp] if i >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (xl[i] + pred) & 255
            out[y] = cur
    return out.astype(np.uint8)


# ---- the corpus ---------------------------------------------------------------------------------------------------------
# GRAY8 255 x 256: a row is 256 filtered bytes (filter type + 255 pixels), raw_n = 65 536 -- the smallest image that holds a
# 65 535-byte stored block and a 32 768-byte distance.  RGB8 85 x 128 has the same 256-byte rows.  Whatever a stream expands to
# is the filtered image, so every 256th byte must be a filter type 0 .. 4: generators either keep to the alphabet 0 .. 4 or cut
# a match short where it would put another byte there.
ROW = 256
GRAY = dict(w=255, h=256, ctype=0, fmt=0, bpp=1)
RGB = dict(w=85, h=128, ctype=2, fmt=1, bpp=3)
RAW_N = ROW * 256
OK, NEEDS_HOST, BAD = 0, 1, -1


class Case:
    def __init__(self, name, family, z, status, geom=GRAY, stream=None, raw=None, why=None, info=None):
        self.name, self.family, self.z, self.status, self.geom, self.stream = name, family, z, status, geom, stream
        self.w, self.h, self.fmt = geom["w"], geom["h"], geom["fmt"]
        self.png = png_file(z, geom["w"], geom["h"], geom["ctype"], idat_split=8192 if family == "F2" else None)
        self.raw = bytes(stream.out) if (raw is None and stream is not None) else raw
        self.why = why                 # invalid cases: "refused" (zlib raises) or "length" (a sound stream of the wrong length)
        self.info = info or {}
        self.pixels = None
        if status == OK:
            px = unfilter(self.raw, geom["h"], ROW - 1, geom["bpp"])
            assert px is not None and len(self.raw) == ROW * geom["h"], name
            self.pixels = px if geom["bpp"] == 1 else px.reshape(geom["h"], geom["w"], geom["bpp"])

    def light(self):
        """What a child process needs (no writer report)."""
        return dict(name=self.name, family=self.family, png=self.png, status=self.status, w=self.w, h=self.h, fmt=self.fmt,
                    pixels=self.pixels)


class Sim:
    """Token list in the making, with the bytes it expands to."""
    def __init__(self, rng, raw_n=RAW_N, small=False):
        self.rng, self.raw_n, self.small = rng, raw_n, small
        self.out, self.toks = bytearray(), []

    @property
    def pos(self):
        return len(self.out)

    def lit(self, v=None):
        if v is None:
            v = int(self.rng.integers(0, 5 if (self.small or self.pos % ROW == 0) else 256))
        assert v < 5 or self.pos % ROW, "a filter byte must be 0..4"
        self.toks.append(v)
        self.out.append(v)

    def lits(self, n, v=None):
        for _ in range(n):
            self.lit(v)

    def expand(self, n, d):
        o = self.out
        if d >= n:
            return o[len(o) - d:len(o) - d + n]
        r = bytearray(o[len(o) - d:])
        while len(r) < n:
            r += r[:n - len(r)]
        return r[:n]

    def match(self, n, d, prefer=None, safe=False):
        """safe: cut the match short of a filter byte > 4 and of the image's end; False when nothing of it is left."""
        assert 1 <= d <= self.pos
        n = min(n, self.raw_n - self.pos) if safe else n
        if n < 3:
            return False
        e = self.expand(n, d)
        first = (-self.pos) % ROW
        for k in range(first, n, ROW):
            if e[k] > 4:
                assert safe, "a filter byte must be 0..4"
                n, e = k, e[:k]
                break
        if n < 3:
            return False
        self.toks.append((n, d) if prefer is None else (n, d, prefer))
        self.out += e
        return True

    def take(self):
        t, self.toks = self.toks, []
        return t

    def fill(self, upto=None):
        """Row copies (len 258, dist 256) up to `upto`: cheap in bits, filter bytes copy filter bytes."""
        upto = self.raw_n if upto is None else upto
        assert self.pos >= ROW
        while self.pos < upto:
            rem = upto - self.pos
            n = min(258, rem)
            if 0 < rem - n < 3:
                n = rem - 3
            if n < 3:
                self.lits(rem, int(self.out[-ROW]))
            else:
                self.match(n, ROW)


def auto_code(rng, tokens, extra_ll=0, extra_d=0, maxbits=15):
    """A random complete code pair for the symbols a token list uses (+ 256, + a few unused ones).  A lone end-of-block code and a
    lone distance code get one bit, which every inflater takes; no distance code at all when there is no match."""
    ll_used, d_used = {256}, set()
    for t in tokens:
        if isinstance(t, int):
            ll_used.add(t)
        elif isinstance(t, tuple):
            ll_used.add(len_symbol(t[0], t[2] if len(t) > 2 else None)[0])
            d_used.add(dist_symbol(t[1])[0])
        elif isinstance(t, Sym):
            ll_used.add(t.ll)
            if t.d is not None:
                d_used.add(t.d)
    for _ in range(extra_ll):
        ll_used.add(int(rng.integers(0, 286)))
    for _ in range(extra_d):
        d_used.add(int(rng.integers(0, 30)))
    ll_s, d_s = sorted(ll_used), sorted(d_used)
    ll = dict(zip(ll_s, complete_lengths(rng, len(ll_s), maxbits)))
    dd = dict(zip(d_s, complete_lengths(rng, len(d_s), maxbits))) if d_s else {}
    return ll, dd


def _rng(*key):
    return np.random.default_rng([0xDEF1A7E, *key])


# ---- F1: long codes and wide symbols ---------------------------------------------------------------------------------------
F1_LITS_LONG = [0, 1, 2, 3, 128, 255]
F1_LITS_REST = [4, 7, 200]
F1_LENS_LONG = [257, 264, 265, 284, 285, 270]
F1_D_LONG = [0, 3, 4, 28, 29, 1]
F1_D_REST = [2, 5, 6, 8, 10, 12, 16, 20, 24, 26]


def _ladder(rng, long_syms, rest_syms):
    """Lengths 1, 2, ..., 14, 15, 15 over 16 symbols: 11 .. 15, 15 on long_syms, 1 .. 10 on the rest."""
    long_l, rest_l = [11, 12, 13, 14, 15, 15], list(range(1, 11))
    rng.shuffle(long_l)
    rng.shuffle(rest_l)
    assert len(long_syms) == 6 and len(rest_syms) == 10
    return {**dict(zip(long_syms, map(int, long_l))), **dict(zip(rest_syms, map(int, rest_l)))}


def f1_ladder(k, geom=GRAY):
    rng = _rng(1, k, geom["fmt"])
    raw_n = ROW * geom["h"]
    if k & 1:
        ll = _ladder(rng, F1_LENS_LONG, F1_LITS_LONG + F1_LITS_REST + [256])
    else:
        ll = _ladder(rng, F1_LITS_LONG, F1_LENS_LONG + F1_LITS_REST + [256])
    dd = _ladder(rng, F1_D_LONG, F1_D_REST) if k & 2 else _ladder(rng, F1_D_REST[:6], F1_D_LONG + F1_D_REST[6:])
    sim = Sim(rng, raw_n)
    syms = [s for s in ll if s != 256]
    forced = False
    while sim.pos < raw_n:
        if not forced and sim.pos >= 32768 and raw_n - sim.pos > 600:
            sim.match(258, 32768, prefer=284)                   # 258 as 284 + 31, and as 285; distance 32 768 exactly
            sim.match(258, 32768)
            forced = True
            continue
        for _ in range(30):
            s = syms[int(rng.integers(len(syms)))]
            if s < 256:
                if s > 4 and sim.pos % ROW == 0:
                    continue
                sim.lit(s)
                break
            c = s - 257
            n = LEN_BASE[c] + int(rng.integers(0, 1 << LEN_EXTRA[c]))
            ds = [d for d in dd if DIST_BASE[d] <= sim.pos]
            if not ds or sim.pos + n > raw_n:
                continue
            d = ds[int(rng.integers(len(ds)))]
            dist = DIST_BASE[d] + int(rng.integers(0, min(1 << DIST_EXTRA[d], sim.pos - DIST_BASE[d] + 1)))
            e = sim.expand(n, dist)
            if any(e[q] > 4 for q in range((-sim.pos) % ROW, n, ROW)):
                continue
            sim.match(n, dist, prefer=s)
            break
        else:
            sim.lit(int(rng.integers(0, 4)))
    S = Stream()
    S.dynamic(sim.take(), ll, dd, final=True)
    return Case(f"f1_ladder_{k}_{'rgb' if geom is RGB else 'grey'}", "F1", S.finish(), OK, geom, S, info=dict(ll=ll, dd=dd))


def f1_wide():
    """A stored block of 24 577 bytes, then one dynamic block that is almost all 43- to 48-bit symbols."""
    rng = _rng(1, 99)
    sim = Sim(rng, small=True)
    sim.lits(24577)
    head = bytes(sim.out)
    sim.take()
    ll = {0: 1, 256: 2, 285: 3, 1: 4, 2: 5, 3: 6, 4: 7, 258: 8, 259: 9, 260: 10, 261: 11, 262: 12, 263: 13, 265: 14, 257: 15, 284: 15}
    dd = {**{s: s + 1 for s in range(14)}, 28: 15, 29: 15}
    # A 43-bit symbol: a 15-bit code for length 3, a 15-bit distance code, 13 extra bits.  A 48-bit one: 284 with its 5 extra bits;
    # it costs some 240 bytes of the image, so there are 16 of them beside the forced 284 + 31, each placed where the block's bit
    # position is an even residue mod 32 that no 48-bit symbol has had yet: the widest symbol meets 16 evenly spaced bit phases.
    i, bit, forced, long_at = 0, 0, False, set()
    while RAW_N - sim.pos >= 3:
        i += 1
        far = int(rng.integers(16385, min(sim.pos, 32768) + 1))
        if not forced and sim.pos >= 32768:
            sim.match(258, 32768, prefer=284)                   # (258 as 284 + 31, the distance 32 768 exactly)
            bit += 48
            forced = True
        elif i % 32 == 0:
            sim.lit(0)
            bit += 1
        elif len(long_at) < 16 and i >= 600 * (len(long_at) + 1) and bit % 2 == 0 and bit % 32 not in long_at and RAW_N - sim.pos >= 300:
            sim.match(227 + int(rng.integers(0, 8)), far, prefer=284)
            long_at.add(bit % 32)
            bit += 48
        else:
            sim.match(3, far)
            bit += 43
    sim.lits(RAW_N - sim.pos, 0)
    S = Stream()
    S.stored(head)
    S.dynamic(sim.take(), ll, dd, final=True)
    return Case("f1_wide", "F1", S.finish(), OK, GRAY, S)


# ---- F2: block seams and headers -------------------------------------------------------------------------------------------
def _random_tokens(sim, n):
    rng = sim.rng
    for _ in range(n):
        if sim.pos >= sim.raw_n:
            break
        if sim.pos < 8 or rng.random() < 0.4:
            sim.lit()
            continue
        ln = int((3, 4, 5, 8, 9, 17, 64, 130, 258, 258)[int(rng.integers(10))])
        r = rng.random()
        d = 1 + int(rng.integers(0, 8)) if r < 0.2 else ROW * int(rng.integers(1, 129)) if r < 0.5 else 1 + int(rng.integers(0, 32768))
        if not sim.match(ln, min(d, sim.pos), safe=True):
            sim.lit()


def _empty(S, kind, final=False):
    blk = S.stored(b"", final=final) if kind == 0 else S.fixed([], final=final) if kind == 1 else S.dynamic([], {256: 1}, {}, final=final)
    blk["empty_run"] = True
    return blk


def f2_seams(seed, geom=GRAY):
    """Hundreds of blocks of 0 .. 40 tokens in random alternation, runs of empty blocks in between."""
    rng = _rng(2, seed, geom["fmt"])
    raw_n = ROW * geom["h"]
    sim, S = Sim(rng, raw_n), Stream()
    nblk = 0
    while sim.pos < raw_n:
        nblk += 1
        if nblk % 5 == 0:
            for _ in range(int(rng.integers(1, 41))):
                _empty(S, int(rng.integers(3)))
            continue
        kind = int(rng.integers(3))
        n = int(rng.integers(0, 41))
        if kind == 0:
            sim.lits(min(n, raw_n - sim.pos))
            sim.take()
            S.stored(bytes(sim.out[len(S.out):]), pad_ones=bool(rng.integers(2)))
        else:
            _random_tokens(sim, n)
            t = sim.take()
            if kind == 1:
                S.fixed(t)
            else:
                ll, dd = auto_code(rng, t, extra_ll=int(rng.integers(0, 4)), extra_d=int(rng.integers(0, 3)) if any(isinstance(x, tuple) for x in t) else 0)
                S.dynamic(t, ll, dd)
    for kind in (0, 1, 2, 2, 1, 0):                    # empty non-final blocks behind the last output byte, then an empty final one
        _empty(S, kind)
    _empty(S, seed % 3, final=True)
    return Case(f"f2_seams_{seed}_{'rgb' if geom is RGB else 'grey'}", "F2", S.finish(), OK, geom, S)


def f2_phases():
    """An empty block of each kind with its header at each bit phase 0 .. 31: a fixed block of m nine-bit literals in front of it
    ends 10 + 9 m bits on, and 9 m runs through every residue mod 32."""
    rng = _rng(2, 66)
    sim, S = Sim(rng), Stream()
    sim.lits(ROW)
    S.fixed(sim.take())
    for kind in range(3):
        for target in range(32):
            while sim.pos % ROW == 0 or sim.pos % ROW > ROW - 34:
                sim.lit(0)
            S.fixed(sim.take())
            m = ((target - S.b.pos - 10) * 25) % 32            # 9 * 25 = 1 mod 32
            for _ in range(m):
                sim.lit(144 + int(rng.integers(0, 112)))
            S.fixed(sim.take())
            assert S.b.pos % 32 == target
            _empty(S, kind)
    sim.fill()
    S.fixed(sim.take(), final=True)
    return Case("f2_phases", "F2", S.finish(), OK, GRAY, S)


def f2_stored_sizes():
    """Stored blocks of 1, 2, 3 and 65 535 bytes; a stored block after a Huffman block that ends at each of the 8 bit phases."""
    rng = _rng(2, 77)
    sim, S = Sim(rng), Stream()

    def stored(n, **kw):
        sim.lits(n)
        sim.take()
        return S.stored(bytes(sim.out[len(S.out):]), **kw)
    sim.lit()
    S.fixed(sim.take())
    stored(65535 - 300)
    # behind a stored block the stream is byte-aligned: a fixed block of k 8-bit and m 9-bit literals ends at phase (2 + m) % 8
    for m in range(8):
        while sim.pos % ROW > ROW - 12 or sim.pos % ROW == 0:
            sim.lit(0)
        for _ in range(m):
            sim.lit(144 + int(rng.integers(0, 112)))
        blk = S.fixed(sim.take())
        st = stored((1, 2, 3)[m % 3], pad_ones=bool(m & 1))
        st["after_phase"], st["pad_ones"] = blk["end_bit"] % 8, bool(m & 1)
    _random_tokens(sim, 5)
    S.fixed(sim.take())
    stored(RAW_N - sim.pos, final=True)
    a = Case("f2_stored_small", "F2", S.finish(), OK, GRAY, S)
    sim, S = Sim(rng), Stream()
    sim.lit()
    S.fixed(sim.take())
    sim.lits(65535)
    S.stored(bytes(sim.out[1:]), final=True)
    return [a, Case("f2_stored_65535", "F2", S.finish(), OK, GRAY, S)]


def f2_headers():
    """Dynamic headers zlib never writes, each in a block of its own; the blocks are tagged in the report."""
    rng = _rng(2, 88)
    sim, S = Sim(rng, small=True), Stream()
    sim.lits(ROW)
    S.fixed(sim.take())
    # (a) a code 16 that repeats the last literal/length length on into the distance lengths
    sim.lits(6, 0)
    sim.lit(1)
    sim.match(3, 4)
    sim.match(3, 1)
    sim.match(3, 2)
    sim.match(3, 3)
    ll, dd = {0: 2, 1: 2, 256: 2, 257: 2}, {0: 2, 1: 2, 2: 2, 3: 2}
    cl = [(2, None), (2, None), (18, 138), (18, 116), (2, None), (16, 5)]
    S.dynamic(sim.take(), ll, dd, hlit=258, hdist=4, cl_syms=cl)["tag"] = "rep16_crosses"
    # (b) an 18 of 138, and a 17 of 3 that ends exactly on HLIT + HDIST
    sim.lits(5, 2)
    sim.match(4, 2)
    ll, dd = {2: 1, 256: 2, 258: 2}, {1: 1}
    cl = [(0, None), (0, None), (1, None), (18, 138), (18, 115), (2, None), (0, None), (2, None), (0, None), (1, None), (17, 3)]
    S.dynamic(sim.take(), ll, dd, hlit=259, hdist=5, cl_syms=cl)["tag"] = "rep18_138_rep17_ends"
    # (c) HLIT = 286 with symbol 285 in use, HDIST = 30 with symbol 29 in use -- needs 24 577 bytes behind it: see below
    # (d) HCLEN = 19 with 7-bit code-length codes
    for _ in range(200):
        cl_lens = complete_lengths(rng, 19, 7)
        if max(cl_lens) == 7:
            break
    sim.lits(9)
    sim.match(5, 3)
    sim.match(30, 7)
    sim.lits(3)
    t = sim.take()
    ll, dd = auto_code(rng, t, extra_ll=6, extra_d=3)
    lens = [ll.get(i, 0) for i in range(286)] + [dd.get(i, 0) for i in range(30)]
    S.dynamic(t, ll, dd, hlit=286, hdist=30, cl_lens=cl_lens, cl_syms=[(v, None) for v in lens])["tag"] = "hclen19"
    # (e) HCLEN as small as the lengths in use allow (8 and 0 only: five code-length-code lengths), no distance code at all
    sim.lits(40)
    ll = {**{s: 8 for s in range(255)}, 256: 8}
    S.dynamic(sim.take(), ll, {})["tag"] = "hclen_min_no_dist"
    # (f) one distance code of one bit
    sim.lits(4)
    sim.match(10, 4)
    sim.match(3, 4)
    t = sim.take()
    ll, _ = auto_code(rng, t)
    S.dynamic(t, ll, {3: 1})["tag"] = "one_dist_code"
    sim.fill(25000)
    S.fixed(sim.take())
    sim.match(258, 24577 + 7)
    sim.lits(3)
    sim.match(258, 1)
    t = sim.take()
    ll, dd = auto_code(rng, t, extra_ll=3)
    S.dynamic(t, ll, dd, hlit=286, hdist=30)["tag"] = "hlit286_hdist30"
    sim.fill()
    S.fixed(sim.take(), final=True)
    return Case("f2_headers", "F2", S.finish(), OK, GRAY, S)


# ---- F3: window and match-list geometry ------------------------------------------------------------------------------------
F3_LENS = [3, 4, 5, 8, 9, 10, 64, 65, 258]
F3_SMALL = [1, 2, 3, 4, 5, 7, 8, 9]
kWindow, kRoundBytes, kLaneWords, kRoundWords = 2048, 8192, 32, 2048


def match_path(n, d):
    """Which of resolve_matches' paths a match takes: certain for these classes whatever the rounds (a source is 'far' when it
    lies below round start - 2048, and a round adds at most 8192 bytes)."""
    if n > 8 or d < n:
        return "coop"
    if d <= kWindow:
        return "window"
    if d > kWindow + kRoundBytes + 3:
        return "far"
    return "window_or_far"


def f3_geometry():
    rng = _rng(3, 1)
    sim, S = Sim(rng, small=True), Stream()
    sim.lits(64)
    for n in (3, 9, 64, 258):
        sim.match(n, sim.pos)                           # exactly the bytes produced so far: reaches byte 0
        sim.lits(2)
    placed, c = [], 0

    def place(n, d):
        nonlocal c
        sim.lits((int(rng.integers(4)) - sim.pos) % 4)  # destinations (and with them sources) at every alignment
        c += 1
        placed.append((n, d, sim.pos))
        sim.match(n, d)
    for n in F3_LENS:
        for d in sorted(set(F3_SMALL + [n - 1, n, n + 1])):
            place(n, d)
    S.fixed(sim.take())
    for lo, hi, upto in ((2040, 2056, 2100), (8184, 8200, 8300), (32767, 32768, 32800)):
        while sim.pos < upto:
            sim.lit()
        sim.take()
        S.stored(bytes(sim.out[len(S.out):]))
        for rep in range(4 if lo == 32767 else 1):      # (far sources: four rounds, so that both alignments see every value)
            for n in F3_LENS:
                for d in range(lo, hi + 1):
                    place(n, d)
                    if sim.pos > RAW_N - 600:
                        break
        t = sim.take()
        ll, dd = auto_code(rng, t, extra_ll=2)
        S.dynamic(t, ll, dd)
    sim.fill()
    S.fixed(sim.take(), final=True)
    return Case("f3_geometry", "F3", S.finish(), OK, GRAY, S, info=dict(placed=placed))


def f3_runs(k):
    """k leading literals, 2014 stored bytes, then: 40 matches of 258 with alternating distances (never merged: 16 to a lane, two
    lanes pass a round's 8192 bytes), runs of 2, 16, 17 and 100 matches with one distance (merged per lane).  With k = 0 .. 33 every
    match's two token words fall on every place of the 32-word lane seam and of the 2048-word round seam."""
    rng = _rng(3, 2)                                   # (the same tail for every k)
    sim, S = Sim(rng, small=True), Stream()
    if k:
        sim.lits(k, 0)
        S.fixed(sim.take())
    sim.lits(2014)
    sim.take()
    S.stored(bytes(sim.out[len(S.out):]))
    for i in range(40):
        sim.match(258, (256, 512)[i & 1])
    for run in (2, 16, 17, 100):
        for n, d in ((3, 3), (258, 1), (4, 256)):
            sim.lit()
            for _ in range(run):
                sim.match(n, d)
    S.fixed(sim.take())
    sim.fill()
    S.fixed(sim.take(), final=True)
    return Case(f"f3_runs_{k}", "F3", S.finish(), OK, GRAY, S)


def f3_two_bit():
    """A zero image as two-bit matches: a one-bit code for 285 and a one-bit distance code."""
    S = Stream()
    S.dynamic([0] + [(258, 1)] * 254 + [(3, 1)], {285: 1, 0: 2, 256: 3, 257: 3}, {0: 1}, final=True)
    return Case("f3_two_bit", "F3", S.finish(), OK, GRAY, S)


def token_words(stream):
    """Word index (16-bit token words of the two-pass form: 1 per literal or stored byte, 2 per match) of every match head."""
    heads, w = [], 0
    for blk in stream.blocks:
        if blk["kind"] == "stored":
            w += (blk["end_bit"] - blk["sym_bit"]) // 8
        for _, _, ll, *_ in blk["tokens"]:
            if ll < 256:
                w += 1
            else:
                heads.append(w)
                w += 2
    return heads


# ---- F4: invalid streams: a valid stream with one field changed ------------------------------------------------------------
def f4_cases():
    out = []

    def add(name, build, status=BAD, why="refused", **fin):
        rng = _rng(4, len(out))
        sim, S = Sim(rng), Stream()
        build(rng, sim, S)
        out.append(Case("f4_" + name, "F4" if status != OK else "F4twin", S.finish(**fin), status, GRAY, S, why=None if status == OK else why))

    def row0(sim, S, **kw):
        sim.lits(ROW)
        S.fixed(sim.take(), **kw)

    def rest(sim, S, **kw):
        sim.fill()
        S.fixed(sim.take(), final=True, **kw)

    def simple(mid=None, **restkw):
        def b(rng, sim, S):
            row0(sim, S)
            if mid:
                mid(rng, sim, S)
            rest(sim, S, **restkw)
        return b
    # header and block structure
    add("btype3", simple(btype=3))

    def nlen(rng, sim, S):
        sim.lits(ROW)
        sim.take()
        S.stored(bytes(sim.out), nlen_field=(ROW ^ 0xffff) ^ 0x0100)
        rest(sim, S)
    add("len_nlen", nlen)

    def beyond(rng, sim, S):
        row0(sim, S)
        sim.fill(RAW_N - 100)
        S.fixed(sim.take())
        S.stored(bytes(10), final=True, len_field=100)
    add("stored_len_beyond_input", beyond, trailer=False)

    def dyn_header(**kw):
        def mid(rng, sim, S):
            sim.lits(20)
            sim.match(5, 7)
            t = sim.take()
            ll, dd = auto_code(rng, t)
            S.dynamic(t, ll, dd, **kw)
        return simple(mid)
    add("hlit_field_30", dyn_header(hlit_field=30))
    add("hlit_field_31", dyn_header(hlit_field=31))
    add("hdist_31", dyn_header(hdist_field=30))
    add("hdist_32", dyn_header(hdist_field=31))

    # code-length coding
    def cl_case(change):
        def mid(rng, sim, S):
            sim.lits(20)
            sim.match(5, 7)
            t = sim.take()
            ll, dd = auto_code(rng, t)
            hlit, hdist = max(ll) + 1, max(dd) + 4               # (three zero lengths at the end, for the overrun)
            lens = [ll.get(i, 0) for i in range(hlit)] + [dd.get(i, 0) for i in range(hdist)]
            cl_syms, cl_lens = rle_lengths(lens), None
            if change == "incomplete":
                cl_lens = cl_lengths_for(cl_syms)
                cl_lens[max(range(19), key=lambda s: cl_lens[s])] += 1
            elif change == "over":
                cl_lens = cl_lengths_for(cl_syms)
                cl_lens[min((s for s in range(19) if cl_lens[s]), key=lambda s: -cl_lens[s])] -= 1
            elif change == "first16":
                cl_syms = [(16, 3)] + rle_lengths(lens[3:])
            elif change == "overrun":
                cl_syms = rle_lengths(lens[:-3]) + [(17, 4)]
            S.dynamic(t, ll, dd, hlit=hlit, hdist=hdist, cl_syms=cl_syms, cl_lens=cl_lens)
        return simple(mid)
    for ch in ("incomplete", "over", "first16", "overrun"):
        add("cl_" + ch, cl_case(ch))

    # the two main codes
    def no_eob(rng, sim, S):
        sim.lits(16, 0)
        sim.lits(16, 1)
        S.dynamic(sim.take(), {0: 1, 1: 1}, {}, eob=False)
    add("no_eob_code", simple(no_eob))

    def main_code(which, change):
        def mid(rng, sim, S):
            sim.lits(20)
            sim.match(5, 7)
            sim.match(3, 1)
            sim.match(4, 20)
            t = sim.take()
            ll, dd = auto_code(rng, t, maxbits=14)
            c = ll if which == "ll" else dd
            s = max(c, key=lambda q: c[q])
            c[s] += 1 if change == "incomplete" else -1
            assert sum(1 for q in c if c[q]) >= 2
            S.dynamic(t, ll, dd)
        return simple(mid)
    for which in ("ll", "dist"):
        add(which + "_over_subscribed", main_code(which, "over"))
        add(which + "_incomplete_two_codes", main_code(which, "incomplete"))

    # codes used in the data
    def unassigned_dist(rng, sim, S):
        sim.lits(8)
        S.dynamic(sim.take() + [Sym(257, 0), RawBits([(1, 1)])], {**{s: 8 for s in range(254)}, 256: 8, 257: 8}, {0: 1})
    add("unassigned_code_lone_dist", simple(unassigned_dist))

    def unassigned_ll(rng, sim, S):
        S.dynamic([RawBits([(1, 1)])], {256: 1}, {}, eob=False)
    add("unassigned_code_lone_ll", simple(unassigned_ll))

    def no_dist_match(rng, sim, S):
        sim.lits(8)
        S.dynamic(sim.take() + [Sym(257, 0), RawBits([(0, 5)])], {**{s: 8 for s in range(254)}, 256: 8, 257: 8}, {})
    add("match_without_dist_codes", simple(no_dist_match))
    for name, sym in (("sym286", Sym(286)), ("sym287", Sym(287)), ("dist30", Sym(257, 0, 30, 0)), ("dist31", Sym(257, 0, 31, 0))):
        def fx(rng, sim, S, sym=sym):
            sim.lits(5)
            S.fixed(sim.take() + [sym])
        add("fixed_" + name, simple(fx))

    # distances
    def too_far(k):
        def b(rng, sim, S):
            sim.lits(k, 0)
            S.fixed(sim.take() + [Sym(*len_symbol(3), *dist_symbol(k + 1))])
            sim.lits(ROW)
            S.fixed(sim.take())
            rest(sim, S)
        return b
    add("dist_beyond_start_first", too_far(0))
    add("dist_beyond_start_after5", too_far(5))

    # output length and stream end
    def longer(extra):
        def b(rng, sim, S):
            row0(sim, S)
            sim.raw_n = RAW_N * 3
            if extra == 257:
                sim.fill(RAW_N - 1)
                sim.match(258, ROW)
            else:
                sim.fill(RAW_N + extra - 1 if extra > 0 else RAW_N - 4)
                sim.lits(1 if extra > 0 else 3, 0)
            S.fixed(sim.take(), final=True)
        return b
    add("inflates_to_raw_n_plus_1", longer(1), why="length")
    add("inflates_to_raw_n_plus_257", longer(257), why="length")
    add("inflates_to_3_raw_n", longer(2 * RAW_N), why="length")
    add("inflates_to_raw_n_minus_1", longer(-1), why="length")
    lad = f1_ladder(0)
    tk = [t for t in lad.stream.blocks[0]["tokens"] if t[0] // 8 != (t[0] + t[1] - 1) // 8 and t[0] % 8]
    cut = (tk[len(tk) // 2][0] + 7) // 8                 # a byte boundary strictly inside a symbol
    out.append(Case("f4_ends_mid_symbol", "F4", lad.z[:cut], BAD, GRAY, raw=b"", why="refused"))

    def non_final(rng, sim, S):
        row0(sim, S)
        sim.fill()
        S.fixed(sim.take())
    add("ends_after_non_final_block", non_final, trailer=False)

    # lone incomplete codes: one bit is what every inflater takes; any other length zlib refuses and others take -> the host decides
    for bits in (1, 2, 15):
        def lone_ll(rng, sim, S, bits=bits):
            S.dynamic([], {256: bits}, {})
        add(f"lone_ll_code_{bits}_bit", simple(lone_ll), status=OK if bits == 1 else NEEDS_HOST)

        def lone_d(rng, sim, S, bits=bits):
            sim.lits(8, 1)
            sim.match(9, 1)
            t = sim.take()
            ll, _ = auto_code(rng, t)
            S.dynamic(t, ll, {0: bits})
        add(f"lone_dist_code_{bits}_bit", simple(lone_d), status=OK if bits == 1 else NEEDS_HOST)

    # damage in front of a lone code stays damage, in both inflate forms as in the oracle, which meet the distance first
    def far_then_lone(rng, sim, S):
        sim.lits(5, 0)
        S.fixed(sim.take() + [Sym(*len_symbol(3), *dist_symbol(6))])
        S.dynamic([], {256: 2}, {})
        row0(sim, S)
        rest(sim, S)
    add("dist_beyond_start_then_lone_code", far_then_lone)
    return out


# ---- F5: filter rows libpng does not choose -------------------------------------------------------------------------------
F5_SIZES = [1, 2, 63, 64, 65, 129]
F5_LAYOUTS = [("grey", 0, 1, 0), ("grey_alpha", 4, 2, 0), ("rgb", 2, 3, 1), ("rgba", 6, 4, 2), ("palette", 3, 1, 1)]   # name, ctype, bpp, pixfmt


class FilterCase:
    def __init__(self, name, layout, w, h, ftypes, rng, status=OK):
        lname, ctype, bpp, fmt = layout
        self.name, self.family, self.status, self.w, self.h, self.fmt, self.ftypes, self.layout = name, "F5", status, w, h, fmt, ftypes, lname
        row = w * bpp
        raw = rng.integers(0, 256, (h, row + 1), dtype=np.uint8)       # random FILTERED bytes: arbitrary residuals, Paeth ties
        raw[:, 0] = ftypes
        self.raw = raw.tobytes()
        plte = rng.integers(0, 256, 3 * 37, dtype=np.uint8) if ctype == 3 else None       # a short palette: entries 37 .. are black
        self.z = zlib.compress(self.raw, 1)
        self.png = png_file(self.z, w, h, ctype, plte=plte)
        self.pixels = None
        if status == OK:
            px = unfilter(self.raw, h, row, bpp)
            if ctype == 3:
                pal = np.zeros((256, 3), np.uint8)
                pal[:37] = plte.reshape(37, 3)
                px = pal[px]
            elif ctype == 4:
                px = px[:, 0::2]
            elif bpp > 1:
                px = px.reshape(h, w, bpp)
            self.pixels = np.ascontiguousarray(px)

    light = Case.light


def f5_cases():
    out = []
    for li, layout in enumerate(F5_LAYOUTS):
        rng = _rng(5, li)
        for shift in (0, li + 1):
            for i, h in enumerate(F5_SIZES):
                w = F5_SIZES[(i + shift) % 6]
                out.append(FilterCase(f"f5_{layout[0]}_{w}x{h}_random", layout, w, h, rng.integers(0, 5, h), rng))
        for t in range(5):
            ft = rng.integers(0, 5, 129)
            ft[[0, 63, 64, 65, 127, 128]] = t
            out.append(FilterCase(f"f5_{layout[0]}_65x129_type{t}_on_seam_rows", layout, 65, 129, ft, rng))
            out.append(FilterCase(f"f5_{layout[0]}_64x129_all_type{t}", layout, 64, 129, np.full(129, t), rng))
    rng = _rng(5, 99)
    for bad in (5, 255):
        for r in (0, 1, 70, 128):
            ft = rng.integers(0, 5, 129)
            ft[r] = bad
            out.append(FilterCase(f"f5_grey_65x129_filter{bad}_row{r}", F5_LAYOUTS[0], 65, 129, ft, rng, status=BAD))
    return out


# ---- all of it ------------------------------------------------------------------------------------------------------------
_corpus = None


def corpus():
    """Every case, built once per process: F1 .. F4 (Case) and F5 (FilterCase)."""
    global _corpus
    if _corpus is None:
        c = [f1_ladder(k) for k in range(4)] + [f1_ladder(1, RGB), f1_ladder(2, RGB), f1_wide()]
        c += [f2_seams(0), f2_seams(1), f2_seams(2, RGB)] + [f2_phases()] + f2_stored_sizes() + [f2_headers()]
        c += [f3_geometry()] + [f3_runs(k) for k in range(34)] + [f3_two_bit()]
        c += f4_cases()
        c += f5_cases()
        _corpus = c
    return _corpus


def batches(cases):
    """The cases as decode batches of one geometry each, {(w, h, fmt): [case, ...]}: every case that must be refused (or handed to
    the host) sits between two valid files of different content, whose pixels are checked like everyone's."""
    groups = {}
    for c in cases:
        groups.setdefault((c["w"], c["h"], c["fmt"]), []).append(c)
    out = {}
    for key, g in groups.items():
        good, bad = [c for c in g if c["status"] == OK], [c for c in g if c["status"] != OK]
        order, gi = [], 0
        if bad:
            assert len(good) >= 2, key
        for b in bad:
            order += [good[gi % len(good)], b]
            gi += 1
        order += [good[(gi + j) % len(good)] for j in range(len(good))]
        out[key] = order
    return out


def check(image, ctx, cases, tile=None):
    """Decodes the cases (dicts of Case.light()) batch by batch through image.decode_pngs and compares status and pixels bit for bit.
    tile: repeat the largest batch's files up to that many.  -> the list of mismatches (empty: all well)."""
    wrong = []
    for (w, h, fmt), order in batches(cases).items():
        if tile:
            if (w, h, fmt) != (GRAY["w"], GRAY["h"], GRAY["fmt"]):
                continue
            order = [order[i % len(order)] for i in range(tile)]
        fr, st = image.decode_pngs([c["png"] for c in order], w, h, fmt, ctx=ctx)
        for i, c in enumerate(order):
            if int(st[i]) != c["status"]:
                wrong.append((c["name"], i, "status", int(st[i]), c["status"]))
            elif c["status"] == OK and not np.array_equal(fr[i], c["pixels"]):
                wrong.append((c["name"], i, "pixels", int((fr[i] != c["pixels"]).sum()), 0))
    return wrong


def child_main(path, tiles):
    """Entry of the child processes (one per setting of the decoder's switches, which are read once per process)."""
    import pickle
    from ucfp_amd import _lib, image
    with open(path, "rb") as f:
        cases = pickle.load(f)
    ctx = _lib.default_context(0)
    wrong = check(image, ctx, cases)
    for t in tiles:
        wrong += check(image, ctx, cases, tile=t)
    print("wrong", wrong[:20])
    print("ok" if not wrong else "FAILED")
