"""Plain-Python restatement of the STREAMING form of text mode RAW_UTF8 ("UTF-8 streams"): what one
slot of a UTF-8 stream set does with the chunks of a document, without a device.

    CanonStream().push(chunk: bytes, final: bool) -> (piece: bytes, status)

The pieces of a stream, concatenated, are the canonical token string `text_canon_ref.canon_bytes` gives for the whole
document, however the document was cut.  The rules a non-final push follows:
  - the trailing bytes of an incomplete UTF-8 sequence (at most 3) are HELD raw and prefixed to the next chunk;
  - the last canonical code point produced so far stays UNDECIDED: the boundary before x[i] needs x[i + 1] (U4);
  - Cf code points produce nothing, so a trailing run of them is consumed, not held;
  - an open segment that already has an alphanumeric is a token: its bytes so far are emitted now;
  - an open segment without one is PROVISIONAL: its canonical bytes (the separator in front included) stay in the
    state, at most OPEN_SEGMENT_BYTES of them -- more at a push boundary and the stream is handed back (NEEDS_HOST,
    sticky), the one place where a stream refuses what the offline call hashes.
A final push decides everything with "no code point" as the right neighbour and closes the open segment; a sequence
still incomplete then is malformed.
"""
from typing import Tuple

import text_canon_ref as ref

NEEDS_HOST = ref.NEEDS_HOST
OPEN_SEGMENT_BYTES = 256            # UCFP_TEXT_STREAM_OPEN_SEGMENT_BYTES
NONE = (0x1FFFF, 15)                # "no code point": class 15 is in no class set, no apostrophe, no flags


def incomplete_tail(v: bytes) -> int:
    """Bytes at the end of `v` that begin a UTF-8 sequence and do not finish it: the last byte >= 0xC0 among the last
    three, when the sequence its value announces reaches past the end.  Whether the sequence is VALID is not decided
    here: it is decoded, strictly, once it is whole (or at the final push)."""
    for back in (1, 2, 3):
        if back > len(v):
            break
        b = v[-back]
        if b < 0x80:
            return 0
        if b >= 0xC0:
            need = 4 if b >= 0xF0 else 3 if b >= 0xE0 else 2
            return back if back < need else 0
    return 0


class CanonStream:
    def __init__(self):
        self.held = b""             # raw bytes of an incomplete sequence
        self.ctx = [NONE, NONE]     # the last two decided canonical code points
        self.pend = None            # the undecided one
        self.seg_alnum = False      # the open segment has an alphanumeric
        self.prov = b""             # the open segment's bytes while it has none
        self.emitted = False        # a piece byte went out: the stream is (' ' token)*, the string lacks the first ' '
        self.bad = False

    def push(self, chunk: bytes, final: bool) -> Tuple[bytes, int]:
        if self.bad:
            return b"", NEEDS_HOST
        v = self.held + bytes(chunk)
        nh = 0 if final else incomplete_tail(v)
        self.held, v = v[len(v) - nh:], v[:len(v) - nh]
        try:
            s = v.decode("utf-8", "strict")
        except UnicodeDecodeError:
            return self._fail()
        new = ref.canonical(map(ord, s))
        if new is None:
            return self._fail()
        x = self.ctx + ([self.pend] if self.pend is not None else []) + new
        ndec = len(x) if final else max(2, len(x) - 1)
        out, seg_start = bytearray(self.prov), 0
        for i in range(2, ndec):
            if not ref._joined([x[i - 2], x[i - 1], x[i], x[i + 1] if i + 1 < len(x) else NONE], 2):
                if not self.seg_alnum:
                    del out[seg_start:]                  # closed without an alphanumeric: it leaves nothing
                seg_start, self.seg_alnum = len(out), False
                out += b" "
            out += chr(x[i][0]).encode("utf-8")
            self.seg_alnum = self.seg_alnum or bool(x[i][1] & 16)
        self.ctx = x[ndec - 2:ndec]
        self.pend = x[ndec] if ndec < len(x) else None
        if final:
            if not self.seg_alnum:
                del out[seg_start:]
            self.prov = b""
        elif self.seg_alnum:
            self.prov = b""
        else:
            self.prov = bytes(out[seg_start:])
            del out[seg_start:]
            if len(self.prov) > OPEN_SEGMENT_BYTES:
                return self._fail()
        piece = bytes(out)
        if piece and not self.emitted:
            self.emitted, piece = True, piece[1:]
        return piece, 0

    def _fail(self):
        self.bad = True
        self.prov = self.held = b""
        return b"", NEEDS_HOST


def stream_canon(doc: bytes, cuts) -> Tuple[bytes, int]:
    """The document pushed as doc[0:c0], doc[c0:c1], ... and a final push of the rest -> (pieces joined, final status);
    b"" under NEEDS_HOST, as the offline call."""
    st, out, at = CanonStream(), bytearray(), 0
    for c in list(cuts) + [None]:
        piece, status = st.push(doc[at:] if c is None else doc[at:c], c is None)
        out += piece
        at = c
    return (b"", NEEDS_HOST) if status else (bytes(out), 0)
