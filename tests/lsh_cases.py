"""Case builders for the banded MinHash LSH query tests (DESIGN.md "LSH" L1-L4).  Numpy only, fixed seeds.

Every builder returns `(ids, corpus_slots, query_slots, params, facts)`:
  ids           uint64 [n], distinct
  corpus_slots  uint64 [n, 128]
  query_slots   uint64 [nq, 128]
  params        dict(bands, rows, cand_per_band): how the index is created
  facts         what the case claims about itself (which rows, which band, which list position); the claims are
                proved from the checker alone in test_lsh_cases_spec.py, so test_lsh_edges_gpu.py cannot pass vacuously
`resize_sequence` returns a list of such steps for one handle."""
import zlib

import numpy as np

M64 = (1 << 64) - 1
MAX_CAND = 1024                     # L3: the concatenated candidate list is cut here

# what the GPU tests run and the spec tests prove
SWEEP_SHAPES = [(16, 8), (32, 4), (8, 16), (20, 6), (1, 64), (2, 64), (128, 1), (64, 2), (42, 3), (5, 3), (3, 42),
                (7, 9), (1, 1)]
SWEEP_SIZES = [1, 2, 63, 64, 65, 257, 4097]
RUN_LENGTHS = [1, 63, 64, 65, 127, 128, 129]        # against the 64-row gather groups ...
RUN_CAPS = [1, 63, 64, 65, 127, 128, 200]           # ... and cand_per_band


def records(slots) -> np.ndarray:
    """uint64 [n, 128] -> 1032-byte MinHash records (header: u16 schema = 1, six zero pad bytes)."""
    slots = np.ascontiguousarray(slots, dtype="<u8").reshape(-1, 128)
    n = slots.shape[0]
    rec = np.zeros((n, 1032), np.uint8)
    rec[:, 0] = 1
    rec[:, 8:] = slots.view(np.uint8).reshape(n, 1024)
    return rec


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _slots(rng, n):
    """Random slots over the full range [0, 2^64)."""
    return rng.integers(0, 1 << 64, size=(n, 128), dtype=np.uint64)


def _ids(rng, n, lo=0, hi=1 << 64):
    """n distinct ids in [lo, hi), in random order."""
    out = np.unique(rng.integers(lo, hi, size=n + 16, dtype=np.uint64))
    assert out.size >= n
    return rng.permutation(out)[:n]


def _params(bands, rows, cand_per_band=64):
    return dict(bands=bands, rows=rows, cand_per_band=cand_per_band)


def band_slice(b, rows):
    return slice(b * rows, (b + 1) * rows)


def one_band_matches(bands, rows, n):
    """Random corpus.  Query b (one per band) copies band b of a corpus row and is random in every other slot, so it
    matches that row in band b alone; then up to three queries that equal corpus rows (first, middle, last)."""
    rng = _rng("one_band", bands, rows, n)
    corpus = _slots(rng, n)
    src = rng.integers(0, n, size=bands)
    src[0], src[-1] = n - 1, 0                         # the last and the first row are always somebody's match
    queries = _slots(rng, bands)
    for b in range(bands):
        queries[b, band_slice(b, rows)] = corpus[src[b], band_slice(b, rows)]
    whole = sorted({0, n // 2, n - 1})
    queries = np.concatenate([queries, corpus[whole]])
    facts = dict(band_src=src.tolist(), whole=whole)
    return _ids(rng, n), corpus, queries, _params(bands, rows), facts


def uncovered_slots(bands, rows, n):
    """bands * rows < 128: the slots behind bands * rows take part in the score (L4) and never in candidacy (L3).

    Queries derived from corpus row s (any n >= 1), each random wherever nothing else is said:
      U   copies the uncovered slots of s                          -> no candidate at all
      BA  copies band b of s and all uncovered slots               -> s with agreement rows + u
      BH  copies band b of s and the first u // 2 uncovered slots  -> s with agreement rows + u // 2
      BD  copies band b of s only                                  -> s with agreement rows
      MIX (n >= 2) band b of s, the uncovered slots of another row t -> s alone; t, which agrees in more slots, is absent
    and, where n >= 16, one planted query P with four planted rows: p0 equals P in the uncovered slots only (absent),
    p1 in band 0 and every uncovered slot, p2 in the last band and half the uncovered slots, p3 in band 0 alone; the
    ids ascend from p3 to p1, against the scores."""
    c = bands * rows
    u = 128 - c
    assert u > 0
    rng = _rng("uncovered", bands, rows, n)
    corpus = _slots(rng, n)
    ids = _ids(rng, n, 0, 1 << 63)
    qs, kinds = [], []

    def derived(s, b, n_unc, band=True):
        q = _slots(rng, 1)[0]
        if band:
            q[band_slice(b, rows)] = corpus[s, band_slice(b, rows)]
        q[c:c + n_unc] = corpus[s, c:c + n_unc]
        return q

    planted = None
    if n >= 16:
        p = 2 + rng.choice(n // 2 - 3, size=4, replace=False)       # clear of the rows the derived queries use
        P = _slots(rng, 1)[0]
        corpus[p[0], c:] = P[c:]
        corpus[p[1], band_slice(0, rows)] = P[band_slice(0, rows)]
        corpus[p[1], c:] = P[c:]
        corpus[p[2], band_slice(bands - 1, rows)] = P[band_slice(bands - 1, rows)]
        corpus[p[2], c:c + u // 2] = P[c:c + u // 2]
        corpus[p[3], band_slice(0, rows)] = P[band_slice(0, rows)]
        ids[p[3]], ids[p[2]], ids[p[1]], ids[p[0]] = [np.uint64((1 << 63) + j) for j in range(4)]
        planted = dict(rows=p.tolist(), agree=[u, rows + u, rows + u // 2, rows])
    for s, b in ((0, 0), (n - 1, bands - 1), (n // 2, bands // 2)):
        qs += [derived(s, b, u, band=False), derived(s, b, u), derived(s, b, u // 2), derived(s, b, 0)]
        kinds += [("U", s, 0), ("BA", s, rows + u), ("BH", s, rows + u // 2), ("BD", s, rows)]
        if n >= 2:
            t = (s + 1) % n
            q = derived(s, b, 0)
            q[c:] = corpus[t, c:]
            qs.append(q)
            kinds.append(("MIX", s, rows))
    if planted:
        qs.append(P)
        kinds.append(("P", -1, -1))
    facts = dict(kinds=kinds, planted=planted, uncovered=u)
    return ids, corpus, np.stack(qs), _params(bands, rows), facts


def _band_keys(slots, bands, rows):
    import oracle
    return oracle.lsh_band_keys(records(slots), bands, rows)


POSITIONS = ("first", "last", "middle", "whole_table")


def run_at(position, L, n=None, band=5, bands=16, rows=8, cand_per_band=64):
    """A run of exactly L equal keys in band `band`'s sorted table, at the table's first position, ending at index n
    exactly, around the median, or being the whole table (n = L).  The run's rows are one row of a random corpus (the
    one with the smallest / largest / a median band key) and L - 1 rows appended at the end that carry its band slots.
    Run row j (in row order) agrees with query 0 in the band and in j % 7 slots of the next band, so rows and scores
    are tied together while the ids are shuffled: which rows survive the per-band cap is decided by row, not id.
    Queries: 0 matches the run in that band only; 1 equals the run's last row (found through every other band even
    where the cap cuts it in this one); 2 matches nothing."""
    assert position in POSITIONS and L >= 1
    if position == "whole_table":
        n = L
    elif n is None:
        n = 256 + L
    n0 = n - (L - 1)
    assert n0 >= 1
    rng = _rng("run_at", position, L, n, band, bands, rows)
    base = _slots(rng, n0)
    keys = _band_keys(base, bands, rows)[:, band]
    order = np.argsort(keys, kind="stable")
    head = int(order[{"first": 0, "last": n0 - 1, "middle": n0 // 2, "whole_table": 0}[position]])
    corpus = np.concatenate([base, _slots(rng, L - 1)])
    run_rows = [head] + list(range(n0, n))
    sl, nxt = band_slice(band, rows), band_slice((band + 1) % bands, rows)
    q0 = _slots(rng, 1)[0]
    q0[sl] = base[head, sl]
    for j, r in enumerate(run_rows):
        corpus[r, sl] = base[head, sl]
        if j:
            corpus[r, nxt.start:nxt.start + j % min(7, rows)] = q0[nxt.start:nxt.start + j % min(7, rows)]
    queries = np.stack([q0, corpus[run_rows[-1]], _slots(rng, 1)[0]])
    facts = dict(band=band, run_rows=run_rows, L=L, n=n, position=position)
    return _ids(rng, n), corpus, queries, _params(bands, rows, cand_per_band), facts


CUT_VARIANTS = ("inside", "outside_cut", "outside_cap", "duplicates", "dup_inside", "dup_outside", "b128_cap8",
                "b128_cap64")


def cut_at_1024(variant):
    """The cut of the concatenated candidate list at 1024 entries (L3), to the entry.

    16 x 8, one query q.  For band b a block of `per_band` rows carries q's band-b slots and is random elsewhere; the
    blocks follow each other in row order behind 200 rows of noise.  Row X, the last row of band 15's block, also
    agrees with q in 7 of 8 slots of bands 0..14: agreement 8 + 15 * 7 = 113, everything else scores 8.
      inside       per_band 64, cand_per_band 64: 1024 entries, X is entry 1023 and comes back first (0.8828125)
      outside_cut  per_band 65, cand_per_band 65: 1040 entries cut at 1024, X is absent, the top score is 0.0625
      outside_cap  per_band 70, cand_per_band 64: X is absent through the per-band cap
    Duplicates count toward the cut:
      duplicates   70 rows identical to q, cand_per_band 65: 16 * 65 entries, 65 distinct rows
      dup_inside   63 rows identical to q, then X (band 15 only + 7 of 8 elsewhere), cand_per_band 65: X is entry 1008
      dup_outside  64 rows identical to q, then X: 15 * 64 + 64 entries come first, X would be entry 1024 -- absent
    128 x 1: for each of bands 0..15 a block of 64 rows carries q's slot; X matches q in slot 16 only, the first band
    behind the cut:
      b128_cap8    cand_per_band 8: 16 * 8 entries, then X -- present
      b128_cap64   cand_per_band 64: the list is full after band 15 -- absent"""
    assert variant in CUT_VARIANTS
    rng = _rng("cut", variant.split("_cap")[0] if variant.startswith("b128") else variant)
    q = _slots(rng, 1)[0]
    noise = _slots(rng, 200)
    if variant in ("inside", "outside_cut", "outside_cap"):
        per_band, cap = {"inside": (64, 64), "outside_cut": (65, 65), "outside_cap": (70, 64)}[variant]
        blocks = _slots(rng, 16 * per_band)
        for b in range(16):
            blocks[b * per_band:(b + 1) * per_band, band_slice(b, 8)] = q[band_slice(b, 8)]
        x = 200 + 16 * per_band - 1
        for b in range(15):
            blocks[-1, b * 8:b * 8 + 7] = q[b * 8:b * 8 + 7]
        corpus = np.concatenate([noise, blocks])
        params = _params(16, 8, cap)
        entry = 15 * min(per_band, cap) + per_band - 1 if per_band <= cap else None
        facts = dict(x=x, precut=16 * min(per_band, cap), x_entry=entry, x_agree=113)
    elif variant in ("duplicates", "dup_inside", "dup_outside"):
        ndup = {"duplicates": 70, "dup_inside": 63, "dup_outside": 64}[variant]
        rows_ = [noise, np.repeat(q[None], ndup, axis=0)]
        x = None
        if variant != "duplicates":
            xr = _slots(rng, 1)
            xr[0, band_slice(15, 8)] = q[band_slice(15, 8)]
            for b in range(15):
                xr[0, b * 8:b * 8 + 7] = q[b * 8:b * 8 + 7]
            rows_.append(xr)
            x = 200 + ndup
        corpus = np.concatenate(rows_ + [_slots(rng, 50)])
        params = _params(16, 8, 65)
        take = min(ndup, 65)
        facts = dict(x=x, precut=16 * take + (x is not None), x_entry=16 * take if x is not None else None, x_agree=113)
    else:
        cap = {"b128_cap8": 8, "b128_cap64": 64}[variant]
        blocks = _slots(rng, 16 * 64)
        for b in range(16):
            blocks[b * 64:(b + 1) * 64, b] = q[b]
        xr = _slots(rng, 1)
        xr[0, 16] = q[16]
        corpus = np.concatenate([noise, blocks, xr])
        x = 200 + 16 * 64
        params = _params(128, 1, cap)
        facts = dict(x=x, precut=16 * cap + 1, x_entry=16 * cap, x_agree=1)
    n = corpus.shape[0]
    ids = _ids(rng, n)
    if variant.startswith("b128"):                      # every candidate scores 1/128: X has the smallest id, so it
        lo = int(np.argmin(ids))                        # is first whenever it is a candidate at all
        ids[x], ids[lo] = ids[lo], ids[x]
    return ids, corpus, q[None].copy(), params, facts


ORDERS = ("ascending", "descending", "random")


def graded(order, n_cand=300, mixed_ids=False):
    """The top-k list under pressure.  16 x 8, cand_per_band 1024.  Every candidate carries q's band-0 slots and agrees
    with q in a chosen number of further slots, at random places: the agreement takes every value 8..128 with ties of
    2-4 rows per value (about n_cand rows).  Ids are shuffled and lie at or above 2^63 (`mixed_ids`: every other
    one below 2^63 instead, so that a signed compare orders them wrongly); one id is 2^64 - 2 and one legitimate row has
    id 2^64 - 1, both on rows that equal q.  Corpus row order, which is the order in which the candidates reach the
    top-k list: ascending agreement (every newcomer lands at place 0), descending (every newcomer lands at the end) or
    random.  Behind them 100 rows of noise.
    Query 0 is q.  Query 1 equals q in band 3 only: its candidates (few, all with agreement 8) are ranked by id alone,
    and its unused places tell an id 2^64 - 1 that was found from an id 2^64 - 1 that fills a place."""
    assert order in ORDERS
    rng = _rng("graded", n_cand, mixed_ids)                 # the same rows whatever the order
    q = _slots(rng, 1)[0]
    p3 = min(max((n_cand / 121.0 - 2.0) / 1.6, 0.0), 0.6)   # ties of 2, 3, 4 with mean n_cand / 121
    agree = np.repeat(np.arange(8, 129), rng.choice([2, 3, 4], size=121, p=[1.0 - 1.3 * p3, p3, 0.3 * p3]))
    m = agree.size
    cand = _slots(rng, m)
    for i, a in enumerate(agree.tolist()):
        cand[i, :8] = q[:8]
        extra = 8 + rng.choice(120, size=a - 8, replace=False)
        cand[i, extra] = q[extra]
    ids = _ids(rng, m, 1 << 63, M64 - 1)
    if mixed_ids:
        ids[::2] &= np.uint64((1 << 63) - 1)
        assert np.unique(ids).size == m
    full = np.flatnonzero(agree == 128)
    ids[full[0]], ids[full[1]] = np.uint64(M64), np.uint64(M64 - 1)
    perm = {"ascending": np.arange(m), "descending": np.arange(m)[::-1], "random": _rng("perm").permutation(m)}[order]
    corpus = np.concatenate([cand[perm], _slots(rng, 100)])
    ids = np.concatenate([ids[perm], _ids(rng, 100, 0, 1 << 62) | np.uint64(1 << 63 if not mixed_ids else 0)])
    assert np.unique(ids).size == ids.size
    q1 = _slots(rng, 1)[0]
    q1[band_slice(3, 8)] = q[band_slice(3, 8)]
    facts = dict(agree=agree[perm], n_cand=m, order=order)
    return ids, corpus, np.stack([q, q1]), _params(16, 8, 1024), facts


RESIZE_SIZES = (5000, 10, 70_001, 0, 300)


def resize_sequence(bands=16, rows=8):
    """Corpora of 5000, 10, 70 001, 0 and 300 rows for one handle, pairwise disjoint in rows and ids (step i draws its
    ids from [i * 2^32, (i + 1) * 2^32)).  The queries of a step are rows of its own corpus (first, last, some between)
    and rows of every earlier corpus, the previous one first: the buffers are kept, so what an earlier, larger build
    left behind `n` must never be read.  -> list of (ids, corpus_slots, query_slots, params, facts)."""
    rng = _rng("resize", bands, rows)
    steps, earlier = [], []
    for i, n in enumerate(RESIZE_SIZES):
        corpus = _slots(rng, n)
        ids = _ids(rng, n, i << 32, (i + 1) << 32)
        own = sorted({0, n // 3, n // 2, n - 1}) if n else []
        qs = [corpus[own]] + [c[[0, c.shape[0] // 2, c.shape[0] - 1]] for c in reversed(earlier) if c.shape[0]]
        facts = dict(own=own, n_own=len(own), step=i)
        steps.append((ids, corpus, np.concatenate(qs), _params(bands, rows), facts))
        earlier.append(corpus)
    return steps
