"""Schema types mirroring src/core/mod.rs of the reference (Record :33-72, Hit :107-131,
Query :152-189, Modality :19-26). Field names and meaning are kept 1:1 so the parity tests read
like the reference's own."""
from dataclasses import dataclass, field
from enum import IntEnum
from typing import List, Optional


class Modality(IntEnum):
    # catalog discriminants: src/index/embedded/mod.rs:106,411-414
    Audio = 0
    Image = 1
    Text = 2


class HitSource:
    Vector = "vector"
    Bm25 = "bm25"
    Fused = "fused"
    Hamming = "hamming"   # new capability behind /v1/query; not in the reference
    Landmark = "landmark"  # audio identification over Wang landmarks (DESIGN A10); not in the reference
    Haitsma = "haitsma"    # audio identification over Haitsma sub-fingerprints (DESIGN A12); not in the reference
    Tlsh = "tlsh"          # nearest `tlsh-128-1` records by TLSH distance (DESIGN A15); not in the reference
    ImageMatch = "image-match"   # image records by global and block hashes together (DESIGN A16); not in the reference
    MinHash = "minhash"    # MinHash-128 records by the number of equal slots (DESIGN A17); not in the reference


@dataclass
class Record:
    tenant_id: int
    record_id: int
    modality: Modality
    format_version: int
    algorithm: str
    config_hash: int
    fingerprint: bytes
    embedding: Optional[List[float]] = None
    model_id: Optional[str] = None
    metadata: bytes = b""
    text: Optional[str] = None


@dataclass
class TermHit:
    """One matched query term of a BM25 hit (src/core/mod.rs:191-205): filled when the query asks to explain."""
    term: str
    idf: float
    tf: int
    contribution: float


@dataclass
class Hit:
    tenant_id: int
    record_id: int
    score: float                      # higher is better (src/core/mod.rs:113-115)
    source: str = HitSource.Vector
    vector_score: Optional[float] = None
    bm25_score: Optional[float] = None
    vector_rank: Optional[int] = None
    bm25_rank: Optional[int] = None
    term_hits: list = field(default_factory=list)
    distance: Optional[int] = None    # Hamming distance when source == "hamming"; bit errors of the block when "haitsma"; TLSH distance when "tlsh"; 128 - agree when "minhash"
    votes: Optional[int] = None       # offset-consistent landmark matches when source == "landmark"
    offset: Optional[int] = None      # where the query's frame 0 lies in the record (frames) when source == "landmark" / "haitsma"
    scale: Optional[float] = None     # record frames per query frame, from the (scale, offset) vote over Panako triplets (DESIGN A14)


FORMAT_VERSION = 1  # src/lib.rs:62


# ---- /v1/query wire types (src/server/dto.rs:74-116, handlers.rs:143-187) -----------------------------
# The reference's request needs `vector`; the Hamming search adds ONE additive, backward-compatible field
# (SURVEY 8b / 8f N3): `hash` (u64, or 8 little-endian bytes) with `algorithm` naming the hash space.  Audio
# identification adds `landmarks` (DESIGN A10): Wang landmark bytes (8 per landmark) or a list of [hash, t] pairs; with
# `algorithm` = "audiofp-panako-v1" they are the (hash, t_anchor) pairs of Panako triplets and search that index (A13).
# Keyword search adds `terms` (the reference's Query::terms, src/core/mod.rs:163-164; BM25, DESIGN A11) and `explain`
# (the reference's `?explain=1`, handlers.rs:133-140): terms alone give a BM25 query, vector + terms the hybrid one.
# `triplets` (DESIGN A14) are whole Panako records, 16 bytes per triplet or a list of [hash, t_a, t_b, t_c], and with
# `algorithm` = "audiofp-panako-v1" go to the (scale, offset) vote, which also finds a time-stretched copy; its hits carry
# `scale`.  `resampled`: true next to `triplets` (DESIGN A22) asks the same vote with the bins following the scale, which
# finds a copy played at another speed through a resampler (times and frequencies both change); it is a JSON bool, left
# out when false, and valid only with `triplets`.
# Identification by bit-error rate adds `subfingerprints` (DESIGN A12): Haitsma frames as bytes (4 per frame, u32 LE) or a
# list of integers.
# TLSH-distance search adds `tlsh` (DESIGN A15): the digest string a `tlsh-128-1` record stores ("T1" + 70 hex digits; the
# prefix may be left out) or the 35 digest bytes (bytes, or a list of 35 integers); valid with `algorithm` = "tlsh-128-1" or none.
# Image search over whole records adds `image_record` (DESIGN A16): the 168 bytes of a single-algorithm record or the 536 of
# the bundle, as a list of integers, a hex string or bytes; `algorithm`, when given, must name the tag that goes with the
# length.  `multi_hash` is the reference's MultiHashConfigDto object (kebab-case keys, dto.rs:462-480) and `min_score` a
# number; both are optional and are checked when the query runs.
# MinHash search adds `minhash` (DESIGN A17): the bytes of a MinHash record (8 + 8 H; 1032 at the default H = 128) as a hex
# string, a list of integers or bytes -- its length tells H, and records of that H are searched (DESIGN T10); `algorithm`, when given, names the tag of the records searched ("minhash-h128" or
# "minhash-lsh-h128").  `min_similarity` in (0, 1] is optional and valid only with `minhash`: hits need that Jaccard estimate.
# A body the reference accepts parses to the same query here.

DEFAULT_K = 10   # dto.rs:85-87


@dataclass
class QueryRequest:
    tenant_id: int
    modality: Modality
    k: int = DEFAULT_K
    vector: Optional[List[float]] = None
    hash: Optional[int] = None
    algorithm: Optional[str] = None
    landmarks: Optional[bytes] = None   # 8 bytes per landmark: u32 LE hash, u32 LE t
    subfingerprints: Optional[bytes] = None   # 4 bytes per frame: u32 LE (an audiofp-haitsma-v1 block)
    triplets: Optional[bytes] = None    # 16 bytes per Panako triplet: u32 LE hash, t_a, t_b, t_c (DESIGN A14)
    resampled: bool = False             # a `triplets` query whose bins follow the scale (DESIGN A22)
    tlsh: Optional[bytes] = None        # the 35 bytes of a TLSH digest (DESIGN A15)
    image_record: Optional[bytes] = None   # a whole image record, 168 or 536 bytes (DESIGN A16)
    multi_hash: Optional[dict] = None   # MultiHashConfigDto of an `image_record` query (dto.rs:462-480)
    min_score: Optional[float] = None   # hits of an `image_record` query need at least this score
    minhash: Optional[bytes] = None     # the 8 + 8 H bytes of a MinHash record (DESIGN A17, T10)
    min_similarity: Optional[float] = None   # hits of a `minhash` query need agree / H >= this, in (0, 1]
    terms: List[str] = field(default_factory=list)
    explain: bool = False
    filter: Optional[bytes] = None      # Query.filter (src/core/mod.rs:165-167): a serialized Roaring treemap of record ids (DESIGN F1)

    @classmethod
    def from_json(cls, body: dict) -> "QueryRequest":
        from .errors import InvalidArgument
        try:
            tenant_id = int(body["tenant_id"])
            modality = Modality[body["modality"]]          # "Image" | "Audio" | "Text" (tests.rs:60,199)
        except (KeyError, TypeError, ValueError) as e:
            raise InvalidArgument(f"bad query body: {e}") from None
        k = int(body.get("k", DEFAULT_K))
        vector, h, lm = body.get("vector"), body.get("hash"), body.get("landmarks")
        sub, tri, tl = body.get("subfingerprints"), body.get("triplets"), body.get("tlsh")
        img, mh, ms = body.get("image_record"), body.get("multi_hash"), body.get("min_score")
        mhr, sim = body.get("minhash"), body.get("min_similarity")
        terms = body.get("terms") or []
        if not isinstance(terms, list) or not all(isinstance(t, str) for t in terms):
            raise InvalidArgument("`terms` must be a list of strings")
        if (vector is None and h is None and lm is None and sub is None and tri is None and tl is None and img is None
                and mhr is None and not terms):
            raise InvalidArgument("query needs `vector` (dto.rs:80-82), `terms`, `hash`, `landmarks` or `subfingerprints`")
        if img is not None:
            img = _image_record_bytes(img, body.get("algorithm"))
            if mh is not None and not isinstance(mh, dict):
                raise InvalidArgument("`multi_hash` must be an object")
            if ms is not None and (isinstance(ms, bool) or not isinstance(ms, (int, float))):
                raise InvalidArgument("`min_score` must be a number")
        else:
            mh = ms = None      # they belong to an `image_record` query
        if sim is not None:
            if mhr is None:
                raise InvalidArgument("`min_similarity` goes with `minhash`")
            if isinstance(sim, bool) or not isinstance(sim, (int, float)) or not 0.0 < float(sim) <= 1.0:
                raise InvalidArgument("`min_similarity` must be a number in (0, 1]")
        if mhr is not None:
            mhr = _minhash_bytes(mhr)
            if body.get("algorithm") not in (None,) + _MINHASH_TAGS:
                raise InvalidArgument(f"`minhash` goes with `algorithm` in {list(_MINHASH_TAGS)} or none")
        if tl is not None:
            tl = _tlsh_bytes(tl)
            if body.get("algorithm") not in (None, "tlsh-128-1"):
                raise InvalidArgument("`tlsh` goes with `algorithm` = \"tlsh-128-1\" or none")
        filt = body.get("filter")
        if filt is not None:
            filt = _filter_bytes(filt)
        resampled = body.get("resampled", False)
        if not isinstance(resampled, bool):
            raise InvalidArgument("`resampled` must be true or false")
        if resampled and tri is None:
            raise InvalidArgument("`resampled` goes with `triplets`")
        if tri is not None:
            tri = _triplet_bytes(tri)
        if sub is not None:
            sub = _subfingerprint_bytes(sub)
        if lm is not None:
            lm = _landmark_bytes(lm)
        if isinstance(h, (list, bytes, bytearray)):
            if len(h) != 8:
                raise InvalidArgument("`hash` bytes must be 8 little-endian bytes")
            h = int.from_bytes(bytes(h), "little")
        if h is not None and not 0 <= int(h) < 1 << 64:
            raise InvalidArgument("`hash` must be a u64")
        return cls(tenant_id=tenant_id, modality=modality, k=max(k, 1),       # handlers.rs:153: k.max(1)
                   vector=[float(x) for x in vector] if vector is not None else None,
                   hash=int(h) if h is not None else None, algorithm=body.get("algorithm"), landmarks=lm, subfingerprints=sub,
                   triplets=tri, resampled=resampled, tlsh=tl, image_record=img, multi_hash=dict(mh) if mh is not None else None,
                   min_score=float(ms) if ms is not None else None,
                   minhash=mhr, min_similarity=float(sim) if sim is not None else None,
                   terms=list(terms), explain=_flag(body.get("explain", False)), filter=filt)


def _filter_bytes(f) -> bytes:
    """`filter` of a query body: standard base64 of the filter bytes (or the bytes themselves)."""
    from .errors import InvalidArgument
    if isinstance(f, (bytes, bytearray)):
        return bytes(f)
    if not isinstance(f, str):
        raise InvalidArgument("`filter` must be a base64 string")
    import base64
    import binascii
    try:
        return base64.b64decode(f, validate=True)
    except (binascii.Error, ValueError):
        raise InvalidArgument("`filter` is not standard base64") from None


def _flag(v) -> bool:
    """`explain`: a JSON bool, or the reference's query-string forms "1" | "true" | "yes" (handlers.rs:139-141)."""
    if isinstance(v, str):
        return v in ("1", "true", "yes")
    return bool(v)


def _landmark_bytes(lm) -> bytes:
    """`landmarks` of a query body -> 8 bytes per landmark (u32 LE hash, u32 LE t < 2^31)."""
    from .errors import InvalidArgument
    if isinstance(lm, (bytes, bytearray)):
        if len(lm) % 8:
            raise InvalidArgument("`landmarks` bytes must be a multiple of 8 (u32 hash, u32 t per landmark)")
        return bytes(lm)
    if not isinstance(lm, list):
        raise InvalidArgument("`landmarks` must be bytes or a list of [hash, t] pairs")
    out = bytearray()
    for p in lm:
        if not isinstance(p, (list, tuple)) or len(p) != 2 or not all(isinstance(x, int) for x in p):
            raise InvalidArgument("every landmark must be a [hash, t] pair of integers")
        if not 0 <= p[0] < 1 << 32 or not 0 <= p[1] < 1 << 31:
            raise InvalidArgument("a landmark needs 0 <= hash < 2^32 and 0 <= t < 2^31")
        out += int(p[0]).to_bytes(4, "little") + int(p[1]).to_bytes(4, "little")
    return bytes(out)


def _triplet_bytes(tri) -> bytes:
    """`triplets` of a query body -> 16 bytes per Panako triplet (u32 LE hash, t_a, t_b, t_c)."""
    from .errors import InvalidArgument
    if isinstance(tri, (bytes, bytearray)):
        if len(tri) % 16:
            raise InvalidArgument("`triplets` bytes must be a multiple of 16 (u32 hash, t_a, t_b, t_c per triplet)")
        return bytes(tri)
    if not isinstance(tri, list):
        raise InvalidArgument("`triplets` must be bytes or a list of [hash, t_a, t_b, t_c]")
    out = bytearray()
    for p in tri:
        if (not isinstance(p, (list, tuple)) or len(p) != 4
                or not all(isinstance(x, int) and not isinstance(x, bool) and 0 <= x < 1 << 32 for x in p)):
            raise InvalidArgument("every triplet must be [hash, t_a, t_b, t_c], integers below 2^32")
        out += b"".join(int(x).to_bytes(4, "little") for x in p)
    return bytes(out)


def _tlsh_bytes(tl) -> bytes:
    """`tlsh` of a query body -> the 35 digest bytes."""
    from .errors import InvalidArgument
    if isinstance(tl, list):
        if len(tl) != 35 or not all(isinstance(x, int) and not isinstance(x, bool) and 0 <= x < 256 for x in tl):
            raise InvalidArgument("`tlsh` as a list must be 35 integers below 256")
        return bytes(tl)
    if isinstance(tl, (bytes, bytearray)) and len(tl) == 35:
        return bytes(tl)
    if isinstance(tl, (bytes, bytearray)):
        try:
            tl = bytes(tl).decode("ascii")
        except UnicodeDecodeError:
            raise InvalidArgument("`tlsh` bytes must be the 35 digest bytes or the digest string") from None
    if not isinstance(tl, str):
        raise InvalidArgument("`tlsh` must be the digest string or the 35 digest bytes")
    if len(tl) == 72 and tl[:2] in ("T1", "t1"):
        tl = tl[2:]
    try:
        raw = bytes.fromhex(tl) if len(tl) == 70 else b""
    except ValueError:
        raw = b""
    if len(raw) != 35:
        raise InvalidArgument("`tlsh` must be 70 hex digits, with or without the T1 prefix")
    return raw


_MINHASH_TAGS = ("minhash-h128", "minhash-lsh-h128")
_MINHASH_SIZES = tuple(8 + 8 * h for h in range(16, 1025, 16))   # a record of H slots, H a multiple of 16 in [16, 1024] (DESIGN T10)


def _minhash_bytes(rec) -> bytes:
    """`minhash` of a query body -> the record bytes: 8 + 8 H of them (1032 at the default H = 128)."""
    from .errors import InvalidArgument
    if isinstance(rec, list):
        if len(rec) not in _MINHASH_SIZES or not all(isinstance(x, int) and not isinstance(x, bool) and 0 <= x < 256 for x in rec):
            raise InvalidArgument("`minhash` as a list must be 8 + 8 H integers below 256 (1032 at H = 128)")
        return bytes(rec)
    if isinstance(rec, (bytes, bytearray)):
        raw = bytes(rec)
    elif isinstance(rec, str):
        try:
            raw = bytes.fromhex(rec)
        except ValueError:
            raise InvalidArgument("`minhash` as a string must be hexadecimal") from None
    else:
        raise InvalidArgument("`minhash` must be a hex string, a list of integers or bytes")
    if len(raw) not in _MINHASH_SIZES:
        raise InvalidArgument(f"`minhash` must be 8 + 8 H bytes, H a multiple of 16 in [16, 1024] (1032 bytes, 2064 hex digits, at "
                              f"H = 128), not {len(raw)}")
    return raw


_IMAGE_RECORD_TAGS = {168: ("imgfprint-ahash-v1", "imgfprint-phash-v1", "imgfprint-dhash-v1"),
                      536: ("imgfprint-multihash-v1",)}


def _image_record_bytes(rec, algorithm) -> bytes:
    """`image_record` of a query body -> the 168 or 536 record bytes; `algorithm`, when given, must go with the length."""
    from .errors import InvalidArgument
    if isinstance(rec, list):
        if not all(isinstance(x, int) and not isinstance(x, bool) and 0 <= x < 256 for x in rec):
            raise InvalidArgument("`image_record` as a list must be integers below 256")
        raw = bytes(rec)
    elif isinstance(rec, (bytes, bytearray)):
        raw = bytes(rec)
    elif isinstance(rec, str):
        try:
            raw = bytes.fromhex(rec)
        except ValueError:
            raise InvalidArgument("`image_record` as a string must be hexadecimal") from None
    else:
        raise InvalidArgument("`image_record` must be a list of integers, a hex string or bytes")
    if len(raw) not in _IMAGE_RECORD_TAGS:
        raise InvalidArgument(f"`image_record` must be 168 or 536 bytes, not {len(raw)}")
    if algorithm is not None and algorithm not in _IMAGE_RECORD_TAGS[len(raw)]:
        raise InvalidArgument(f"an `image_record` of {len(raw)} bytes goes with `algorithm` in "
                              f"{list(_IMAGE_RECORD_TAGS[len(raw)])} or none, not {algorithm!r}")
    return raw


def _subfingerprint_bytes(sub) -> bytes:
    """`subfingerprints` of a query body -> 4 bytes per frame (u32 LE)."""
    from .errors import InvalidArgument
    if isinstance(sub, (bytes, bytearray)):
        if len(sub) % 4:
            raise InvalidArgument("`subfingerprints` bytes must be a multiple of 4 (one u32 per frame)")
        return bytes(sub)
    if not isinstance(sub, list) or not all(isinstance(x, int) and not isinstance(x, bool) for x in sub):
        raise InvalidArgument("`subfingerprints` must be bytes or a list of integers")
    if not all(0 <= x < 1 << 32 for x in sub):
        raise InvalidArgument("a sub-fingerprint needs 0 <= value < 2^32")
    return b"".join(int(x).to_bytes(4, "little") for x in sub)


def hit_to_json(h: Hit) -> dict:
    """HitOut (dto.rs:94-116); `distance` only appears on Hamming and Haitsma hits, `votes` only on landmark hits and
    `offset` only on landmark and Haitsma hits, so
    vector hits stay byte-stable.  `term_hits` are TermHitOut objects {term, idf, tf, contribution} (dto.rs:118-124)."""
    out = {"tenant_id": h.tenant_id, "record_id": h.record_id, "score": h.score, "source": h.source,
           "vector_score": h.vector_score, "bm25_score": h.bm25_score, "vector_rank": h.vector_rank,
           "bm25_rank": h.bm25_rank,
           "term_hits": [{"term": t.term, "idf": t.idf, "tf": t.tf, "contribution": t.contribution}
                         if isinstance(t, TermHit) else t for t in h.term_hits]}
    if h.distance is not None:
        out["distance"] = h.distance
    if h.source == HitSource.Landmark:
        out["votes"] = h.votes
        out["offset"] = h.offset
        if h.scale is not None:
            out["scale"] = h.scale
    if h.source == HitSource.Haitsma:
        out["offset"] = h.offset
    return out
