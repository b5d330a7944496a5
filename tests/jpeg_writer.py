"""A coefficient-level baseline JPEG WRITER for the tests (T.81 sequential Huffman; plain numpy, nothing of any decoder).

The decoders under test (oracle/ucfp_oracle_jpeg.c, ucfp_amd/csrc/jpeg.hip) otherwise only ever see what Pillow's libjpeg
encoder emits: luma 1x1 / 2x1 / 2x2 against chroma 1x1, table ids 0 and 1, SOF0 + JFIF, Annex-K or libjpeg-optimised
codes.  This writer takes the QUANTISED COEFFICIENTS themselves -- no forward DCT: the caller owns every coefficient --
and any frame / scan / table layout T.81 allows (and a few it does not: the tests need files libjpeg refuses too).

    f = write_jpeg(coefs, w, h, samp=((4, 1), (1, 1), (1, 1)), restart=3)
    f.data                 the file
    f.blocks_per_mcu ...   what the tests need to know to say which decoder path the file takes (see `Jpeg`)

coefs: one int array [blocks down, blocks across, 64] per component, NATURAL order (row-major 8 x 8), padded to whole MCUs
(`comp_blocks`).  A one-component file is not interleaved: one block per MCU whatever sampling it declares (T.81 A.2.2).
"""
from dataclasses import dataclass, field

import numpy as np

# zigzag index -> natural index (T.81 figure A.6)
ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48,
               41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


@dataclass
class Jpeg:
    data: bytes = field(repr=False)
    w: int
    h: int
    ncomp: int
    blocks_per_mcu: int       # blocks of one MCU of the scan (1 for a one-component file)
    n_mcu: int
    restart: int              # MCUs per restart interval as written in DRI (0: no DRI segment)
    n_seg: int                # restart intervals in the scan = RSTn markers + 1
    clean_len: int            # bytes of entropy-coded data once the stuffing and the RSTn markers are taken out
    scan_off: int             # file offset of the first scan byte
    scan_len: int             # bytes from there to EOI's FF (stuffing and RSTn markers included)
    stuffed_ff: np.ndarray    # offsets (from the first scan byte) of every data FF, each followed by a stuffed 00
    rst: np.ndarray           # offsets (from the first scan byte) of the FF of every RSTn marker
    code_len_hist: np.ndarray = field(repr=False, default=None)   # [17]: coded Huffman symbols by code length


def _ceil_div(a, b):
    return -(-a // b)


def scan_geometry(w, h, samp):
    """-> (MCUs across, MCUs down, sampling factors as the SCAN uses them)."""
    if len(samp) == 1:
        return _ceil_div(w, 8), _ceil_div(h, 8), ((1, 1),)
    hmax, vmax = max(s[0] for s in samp), max(s[1] for s in samp)
    return _ceil_div(w, 8 * hmax), _ceil_div(h, 8 * vmax), tuple(tuple(s) for s in samp)


def comp_blocks(w, h, samp):
    """Blocks (down, across) of every component's coefficient array: whole MCUs."""
    mx, my, eff = scan_geometry(w, h, samp)
    return [(my * v, mx * hh) for hh, v in eff]


def _to_mcu_order(a, mx, my, hs, vs):
    """[my * vs, mx * hs, ...] -> [MCU, block of the component within the MCU, ...] (rows of the MCU first)."""
    rest = a.shape[2:]
    return a.reshape((my, vs, mx, hs) + rest).transpose((0, 2, 1, 3) + tuple(range(4, 4 + len(rest)))).reshape(
        (my * mx, vs * hs) + rest)


def _from_mcu_order(a, mx, my, hs, vs):
    rest = a.shape[2:]
    return a.reshape((my, mx, vs, hs) + rest).transpose((0, 2, 1, 3) + tuple(range(4, 4 + len(rest)))).reshape(
        (my * vs, mx * hs) + rest)


def rand_coefs(rng, w, h, samp, density, amp):
    """Random quantised coefficients for a w x h file of sampling `samp`.  DC: a walk IN CODING ORDER with steps within
    +-30, reflected into +-100.  AC: coefficient k (zigzag) is non-zero with probability density * 8 / (8 + k) and then
    uniform in +-max(1, amp * 8 / (8 + k)): thinning out and shrinking towards the high frequencies, as pictures do."""
    mx, my, eff = scan_geometry(w, h, samp)
    k = np.arange(1, 64)
    p = np.minimum(1.0, density * 8.0 / (8.0 + k))
    a = np.maximum(1, np.floor(amp * 8.0 / (8.0 + k))).astype(np.int64)
    out = []
    for hs, vs in eff:
        n = mx * my * hs * vs
        walk = np.cumsum(rng.integers(-30, 31, n))
        dc = 100 - np.abs((walk + 100) % 400 - 200)                   # triangular fold: steps keep their size
        mag = (rng.random((n, 63)) * a).astype(np.int64) + 1          # 1 .. a
        ac = np.where(rng.random((n, 63)) < p, mag * rng.choice((-1, 1), (n, 63)), 0)
        zz = np.concatenate([dc[:, None], ac], axis=1)
        nat = np.zeros((n, 64), np.int64)
        nat[:, ZZ] = zz
        out.append(_from_mcu_order(nat.reshape(mx * my, hs * vs, 64), mx, my, hs, vs))
    return out


def default_quant(tid):
    """A quantisation table (natural order) with every entry in 1 .. 8, another one for every table id."""
    i = np.arange(64)
    return 1 + (i * (3 + 2 * tid) + 5 * tid + i // 8) % 8


# ---- Huffman tables ----

def optimal_table(freq):
    """Symbol statistics [256] -> (BITS [16], HUFFVAL): T.81 K.2 -- Huffman's procedure with one more symbol reserved so that
    no code is all ones, code lengths limited to 16 (figure K.3)."""
    f = [int(x) for x in freq] + [1]
    codesize = [0] * 257
    others = [-1] * 257
    while True:
        c1 = c2 = -1
        for i in range(257):                       # least frequent, of ties the largest symbol
            if f[i] and (c1 < 0 or f[i] <= f[c1]):
                c1 = i
        for i in range(257):
            if f[i] and i != c1 and (c2 < 0 or f[i] <= f[c2]):
                c2 = i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                   # the reserved symbol had the longest code
    # (after the length limit the lengths are handed out afresh, by code size, as K.2's figure K.4 does)
    vals = [s for _, s in sorted((codesize[s], s) for s in range(256) if codesize[s])]
    assert sum(bits[1:17]) == len(vals)
    return bits[1:17], vals


def comb_table(symbols, mids):
    """An explicit "comb": `symbols` (most frequent FIRST) get, from the front, codes of 16 bits -- as many as are left once
    the others are placed -- then one code of each length in `mids` (a subset of 10 .. 15, longest first), and the last nine
    one code of each length 9 .. 1.  So the common symbols take the canonical search for long codes, and every length of the
    9-bit look-ahead table is in use.  -> (BITS [16], HUFFVAL).  Raises if the all-ones code would be needed."""
    mids = sorted(mids, reverse=True)
    n16 = len(symbols) - 9 - len(mids)
    if n16 < 1:
        raise ValueError("a comb table needs at least %d symbols" % (10 + len(mids)))
    lengths = [16] * n16 + mids + list(range(9, 0, -1))
    budget = (1 << 16) - 1 - sum(1 << (16 - l) for l in lengths)       # Kraft, with the all-ones code left free
    if budget < 0:
        raise ValueError("%d symbols do not fit a comb with middle lengths %s" % (len(symbols), mids))
    bits = [lengths.count(l) for l in range(1, 17)]
    return bits, list(reversed(symbols))


def _codes(bits, vals):
    """Canonical codes (T.81 annex C) -> (code [256], length [256]; length 0: the symbol has no code)."""
    code = np.zeros(256, np.int64)
    length = np.zeros(256, np.int64)
    c, k = 0, 0
    for l in range(1, 17):
        for _ in range(bits[l - 1]):
            code[vals[k]] = c
            length[vals[k]] = l
            c += 1
            k += 1
        assert c <= (1 << l), "over-subscribed Huffman table"
        c <<= 1
    return code, length


def _bitlen(v):
    return np.frexp(np.abs(v).astype(np.float64))[1].astype(np.int64)       # 0 -> 0, else floor(log2) + 1


def _seg(marker, payload, fills):
    n = len(payload) + 2
    assert n <= 65535
    return (b"\xff\xff" if fills else b"") + bytes([0xFF, marker, n >> 8, n & 255]) + payload


def write_jpeg(coefs, w, h, samp, *, restart=0, cids=None, jfif=True, adobe=None, sof=0xC0, tq=None, quant=None,
               huff=None, td=None, ta=None, one_dht=False, one_dqt=False, fills=False, dri_first=False, com=()):
    """Write a sequential-Huffman JPEG of ONE interleaved scan.

    samp       (h, v) per component, 1 or 3 of them
    restart    MCUs per restart interval, 0: none (no DRI segment)
    cids       component ids (default 1, 2, 3); ints or one-character strings
    jfif       write the JFIF APP0 segment;  adobe: None, or the transform byte of an Adobe APP14 segment
    sof        0xC0 or 0xC1
    tq         quantisation table id per component (default 0, 1, 1); quant: {id: 64 values, natural order}
               (default: `default_quant(id)`)
    td, ta     DC / AC Huffman table id per component (default 0, 1, 1)
    huff       {(cls, id): (BITS, HUFFVAL)} explicit tables (cls 0: DC, 1: AC), or a callable (cls, id, freq [256]) ->
               (BITS, HUFFVAL); tables not given are built from the file's own symbol statistics (`optimal_table`)
    one_dht / one_dqt   all tables in one segment (else one segment each)
    fills      FF FF in front of every marker of the HEADERS (after SOI, up to and including SOS; fill bytes inside the
               entropy-coded data are not what decoders agree on)
    dri_first  the DRI segment in front of SOF (else right in front of SOS)
    com        extra segments: (where, marker, payload length) with where = "pre_sof" or "pre_sos" (between DHT and SOS);
               the payload is made of bytes that look like markers
    """
    nc = len(samp)
    assert nc in (1, 3) and len(coefs) == nc
    mx, my, eff = scan_geometry(w, h, samp)
    n_mcu = mx * my
    cids = list(cids) if cids is not None else [1, 2, 3][:nc]
    cids = [ord(c) if isinstance(c, str) else int(c) for c in cids]
    tq = list(tq) if tq is not None else [0, 1, 1][:nc]
    td = list(td) if td is not None else [0, 1, 1][:nc]
    ta = list(ta) if ta is not None else [0, 1, 1][:nc]
    quant = dict(quant or {})
    for t in tq:
        quant.setdefault(t, default_quant(t))

    # ---- blocks in coding order, zigzag ----
    per_comp, comp_of = [], []
    for c, (hs, vs) in enumerate(eff):
        a = np.asarray(coefs[c], np.int64)
        assert a.shape == (my * vs, mx * hs, 64), (a.shape, (my * vs, mx * hs, 64))
        per_comp.append(_to_mcu_order(a, mx, my, hs, vs))
        comp_of += [c] * (hs * vs)
    B = len(comp_of)
    comp_of = np.array(comp_of)
    blocks = np.concatenate(per_comp, axis=1)[:, :, ZZ]                # [MCU, B, 64]
    ivl_of_mcu = np.arange(n_mcu) // restart if restart else np.zeros(n_mcu, np.int64)
    n_seg = int(ivl_of_mcu[-1]) + 1
    # DC differences: the predictor of a component restarts at 0 with every interval
    diff = np.zeros((n_mcu, B), np.int64)
    for c in range(nc):
        cols = np.nonzero(comp_of == c)[0]
        seq = blocks[:, cols, 0]
        prev = np.concatenate([[0], seq.reshape(-1)[:-1]]).reshape(seq.shape)
        first = np.concatenate([[True], ivl_of_mcu[1:] != ivl_of_mcu[:-1]])
        prev[first, 0] = 0
        diff[:, cols] = seq - prev
    nb = n_mcu * B
    zz = blocks.reshape(nb, 64)
    blk_comp = np.tile(comp_of, n_mcu)
    blk_ivl = np.repeat(ivl_of_mcu, B)
    diff = diff.reshape(nb)

    # ---- tokens: (table, symbol, extra bits) in coding order ----
    eb, ek = np.nonzero(zz[:, 1:])                                     # AC coefficients, block by block
    ek = ek + 1
    ev = zz[eb, ek]
    prevk = np.zeros(ek.size, np.int64)                                # the block's previous non-zero coefficient (0: the DC)
    prevk[1:] = np.where(eb[1:] == eb[:-1], ek[:-1], 0)
    run = ek - prevk - 1
    nzrl = run >> 4
    grp = nzrl + 1                                                     # tokens of this coefficient: its ZRLs and itself
    per_blk = np.bincount(eb, weights=grp, minlength=nb).astype(np.int64)
    lastk = np.zeros(nb, np.int64)
    lastk[eb] = ek                                                     # (ascending within a block: the last write wins)
    eob = lastk < 63
    ntok = 1 + per_blk + eob
    bs = np.concatenate([[0], np.cumsum(ntok)])                        # first token of every block
    T = int(bs[-1])
    g = np.concatenate([[0], np.cumsum(grp)])[:-1]
    gb = np.concatenate([[0], np.cumsum(per_blk)])[:-1]
    pos = bs[eb] + 1 + g - gb[eb] + nzrl                               # where the coefficient's own token goes
    tab_td, tab_ta = np.array(td), 4 + np.array(ta)
    t_tab = np.repeat(tab_ta[blk_comp], ntok)
    t_sym = np.full(T, 0xF0, np.int64)                                 # what is not set below is a ZRL
    t_ext = np.zeros(T, np.int64)
    t_nx = np.zeros(T, np.int64)
    sz = _bitlen(ev)
    assert sz.size == 0 or sz.max() <= 10, "AC coefficient beyond 10 bits"
    t_sym[pos] = (run & 15) << 4 | sz
    t_ext[pos] = np.where(ev >= 0, ev, ev + (1 << sz) - 1)
    t_nx[pos] = sz
    t_sym[bs[1:][eob] - 1] = 0x00
    dsz = _bitlen(diff)
    assert dsz.max() <= 11, "DC difference beyond 11 bits"
    t_tab[bs[:-1]] = tab_td[blk_comp]
    t_sym[bs[:-1]] = dsz
    t_ext[bs[:-1]] = np.where(diff >= 0, diff, diff + (1 << dsz) - 1)
    t_nx[bs[:-1]] = dsz
    t_ivl = np.repeat(blk_ivl, ntok)

    # ---- code tables ----
    freq = np.bincount(t_tab * 256 + t_sym, minlength=8 * 256).reshape(8, 256)
    tables = {}
    for key in sorted({(0, t) for t in td} | {(1, t) for t in ta}):
        if isinstance(huff, dict) and key in huff:
            tables[key] = huff[key]
        elif callable(huff):
            tables[key] = huff(key[0], key[1], freq[key[0] * 4 + key[1]])
        else:
            tables[key] = optimal_table(freq[key[0] * 4 + key[1]])
    code = np.zeros((8, 256), np.int64)
    length = np.zeros((8, 256), np.int64)
    for (cls, t), (bits, vals) in tables.items():
        code[cls * 4 + t], length[cls * 4 + t] = _codes(bits, vals)
    t_len = length[t_tab, t_sym]
    assert t_len.min() > 0, "a coded symbol has no code in its table"
    val = code[t_tab, t_sym] << t_nx | t_ext
    nbits = t_len + t_nx

    # ---- bits -> bytes: every interval padded with ones to a whole byte ----
    ivl_bits = np.bincount(t_ivl, weights=nbits, minlength=n_seg).astype(np.int64)
    pad = (-ivl_bits) % 8
    ends = np.cumsum(np.bincount(t_ivl, minlength=n_seg))
    val = np.insert(val, ends, (1 << pad) - 1)
    nbits = np.insert(nbits, ends, pad)
    sh = nbits[:, None] - 1 - np.arange(27)
    stream = ((val[:, None] >> np.maximum(sh, 0)) & 1)[sh >= 0].astype(np.uint8)
    clean = np.packbits(stream)
    ivl_bytes = (ivl_bits + pad) // 8
    assert clean.size == ivl_bytes.sum() and ivl_bytes.min() > 0
    # ---- stuffing and RSTn markers ----
    is_ff = clean == 0xFF
    byte_ivl = np.repeat(np.arange(n_seg), ivl_bytes)
    at = np.arange(clean.size) + np.concatenate([[0], np.cumsum(is_ff)[:-1]]) + 2 * byte_ivl
    scan = np.zeros(clean.size + int(is_ff.sum()) + 2 * (n_seg - 1), np.uint8)
    scan[at] = clean
    starts = at[np.concatenate([[0], np.cumsum(ivl_bytes)[:-1]])[1:]]  # first byte of intervals 1 ..
    scan[starts - 2] = 0xFF
    scan[starts - 1] = 0xD0 + np.arange(n_seg - 1) % 8

    # ---- headers ----
    def seg(marker, payload):
        return _seg(marker, payload, fills)

    def extra(where):
        out = b""
        for wh, marker, n in com:
            assert wh in ("pre_sof", "pre_sos")
            if wh == where:
                out += seg(marker, (b"\xff\xda\x00\x0c\xff\xc4\xff\xd9\xff\xc0\xff\xd8" * (n // 12 + 1))[:n])
        return out

    out = b"\xff\xd8"
    if jfif:
        out += seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    if adobe is not None:
        out += seg(0xEE, b"Adobe\0\x64\0\0\0\0" + bytes([adobe]))
    dqt = [bytes([t]) + bytes(int(x) for x in np.asarray(quant[t])[ZZ]) for t in sorted(set(tq))]
    out += seg(0xDB, b"".join(dqt)) if one_dqt else b"".join(seg(0xDB, d) for d in dqt)
    dri = seg(0xDD, bytes([restart >> 8, restart & 255])) if restart else b""
    out += extra("pre_sof")
    if dri_first:
        out += dri
    out += seg(sof, bytes([8, h >> 8, h & 255, w >> 8, w & 255, nc]) +
               b"".join(bytes([cids[c], samp[c][0] << 4 | samp[c][1], tq[c]]) for c in range(nc)))
    dht = [bytes([cls << 4 | t]) + bytes(bits) + bytes(vals) for (cls, t), (bits, vals) in tables.items()]
    out += seg(0xC4, b"".join(dht)) if one_dht else b"".join(seg(0xC4, d) for d in dht)
    out += extra("pre_sos")
    if not dri_first:
        out += dri
    out += seg(0xDA, bytes([nc]) + b"".join(bytes([cids[c], td[c] << 4 | ta[c]]) for c in range(nc)) + b"\0\x3f\0")
    scan_off = len(out)
    out += scan.tobytes() + b"\xff\xd9"
    return Jpeg(data=out, w=w, h=h, ncomp=nc, blocks_per_mcu=B, n_mcu=n_mcu, restart=restart, n_seg=n_seg,
                clean_len=int(clean.size), scan_off=scan_off, scan_len=int(scan.size), stuffed_ff=at[is_ff],
                rst=starts - 2, code_len_hist=np.bincount(t_len, minlength=17))
