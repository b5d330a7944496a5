"""GPU parity: near-duplicate clusters from the MinHash LSH index (ucfp_lsh_dedup_dev through ucfp_amd.text) vs the
CPU restatement in tests/dedup_ref.py (spec: DESIGN.md "LSH" L5-L7).  Labels, representative ids, keep flags and all
four stats are compared bit for bit."""
import functools

import numpy as np
import pytest

from dedup_ref import SPAN_ALL, dedup_ref, records_of, slots_of

pytestmark = pytest.mark.gpu

SHAPES = [(16, 8), (32, 4), (5, 3), (1, 64), (128, 1)]


def _planted(rng, n_bases, variants, n_noise, keep):
    """Clusters of near-duplicates: each variant keeps a slot of its base with probability `keep` (the corpora of
    test_lsh_gpu.py, same draws in the same order).  Also returns each row's family (-1: noise)."""
    bases = rng.integers(0, 1 << 63, size=(n_bases, 128), dtype=np.uint64)
    rows = [rng.integers(0, 1 << 63, size=(n_noise, 128), dtype=np.uint64)]
    for v in range(variants):
        mask = rng.random((n_bases, 128)) < keep
        rows.append(np.where(mask, bases, rng.integers(0, 1 << 63, size=(n_bases, 128), dtype=np.uint64)))
    corpus = np.concatenate(rows)
    family = np.concatenate([np.full(n_noise, -1)] + [np.arange(n_bases)] * variants)
    perm = rng.permutation(corpus.shape[0])
    return bases, corpus[perm], family[perm]


def _check(res, want):
    labels, rep_ids, keep, stats = want
    assert [res.pairs, res.clusters, res.duplicates, res.largest] == stats.tolist()
    assert res.labels.dtype == np.uint32 and np.array_equal(res.labels, labels)
    assert res.rep_ids.dtype == np.uint64 and np.array_equal(res.rep_ids, rep_ids)
    assert res.keep.dtype == bool and np.array_equal(res.keep, keep)


def _dedup(ids, rec, bands, rows, min_agree, span):
    from ucfp_amd import text
    idx = text.LshIndex(bands, rows)
    try:
        idx.build(ids, rec)
        return idx.dedup(min_agree=min_agree, span=span)
    finally:
        idx.close()


@pytest.mark.parametrize("bands,rows,keep,min_agree", [(16, 8, 0.9, 96), (32, 4, 0.7, 52), (8, 16, 0.95, 110),
                                                       (20, 6, 0.8, 70)])
def test_planted_clusters(gpu_ctx, bands, rows, keep, min_agree):
    rng = np.random.default_rng(1000 + bands)
    _, corpus, family = _planted(rng, n_bases=150, variants=6, n_noise=20000, keep=keep)
    ids = rng.permutation(np.arange(10_000, 10_000 + corpus.shape[0], dtype=np.uint64))
    rec = records_of(corpus)
    res = _dedup(ids, rec, bands, rows, min_agree, 16)
    _check(res, dedup_ref(ids, rec, bands, rows, min_agree, 16))
    # sanity on top of the equality: the planted families are found, and nothing else is
    whole = 0
    for f in range(150):
        lab = res.labels[family == f]
        whole += int((lab == lab[0]).all() and (res.labels == lab[0]).sum() == 6)
    assert whole >= 130
    members = np.flatnonzero(~res.keep | np.isin(np.arange(res.labels.size), res.labels[~res.keep]))
    assert (family[members] >= 0).all()                                             # no noise row in any cluster
    assert np.array_equal(family[members], family[res.labels[members]])             # no cluster mixes two families


def _heavy_corpus():
    rng = np.random.default_rng(7)
    base = rng.integers(0, 1 << 63, size=(1, 128), dtype=np.uint64)
    same = np.repeat(base, 3000, axis=0)
    near = np.repeat(base, 40, axis=0)
    near[np.arange(40), rng.integers(0, 128, 40)] ^= np.uint64(1)
    noise = rng.integers(0, 1 << 63, size=(500, 128), dtype=np.uint64)
    corpus = np.concatenate([noise, near[:20], same, near[20:]])
    ids = rng.permutation(np.arange(corpus.shape[0], dtype=np.uint64)) + np.uint64(1 << 40)
    return ids, records_of(corpus)


@functools.lru_cache(maxsize=None)
def _heavy_ref(span, min_agree):
    ids, rec = _heavy_corpus()
    return dedup_ref(ids, rec, 16, 8, min_agree, span)


@pytest.mark.parametrize("skip", [True, False])
@pytest.mark.parametrize("min_agree", [127, 128])
@pytest.mark.parametrize("span", [1, 16, 5000, SPAN_ALL])
def test_heavy_bucket(gpu_ctx, monkeypatch, span, min_agree, skip):
    """3000 identical rows, 40 one-slot-off copies, 500 noise rows: runs of 3000+ rows in every band.  Same results
    whether or not candidates whose rows already share a root are verified."""
    if skip:
        monkeypatch.delenv("UCFP_LSH_DEDUP_NO_SKIP", raising=False)
    else:
        monkeypatch.setenv("UCFP_LSH_DEDUP_NO_SKIP", "1")
    ids, rec = _heavy_corpus()
    res = _dedup(ids, rec, 16, 8, min_agree, span)
    # j - i never exceeds n - 1, so a span beyond the corpus is the span n: one reference run serves 5000 and SPAN_ALL
    want = _heavy_ref(min(span, rec.shape[0]), min_agree)
    _check(res, want)
    if span >= 5000:
        assert res.largest == (3040 if min_agree == 127 else 3000)
        assert res.pairs > 16 * 3000 * 2999 // 2                      # every pair of the identical rows, in every band


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_edge_sizes_all_rows_distinct(gpu_ctx, n):
    rng = np.random.default_rng(n)
    rec = records_of(rng.integers(0, 1 << 63, size=(n, 128), dtype=np.uint64))
    ids = rng.permutation(np.arange(n, dtype=np.uint64)) + np.uint64(5)
    res = _dedup(ids, rec, 16, 8, 103, 16)
    _check(res, dedup_ref(ids, rec, 16, 8, 103, 16))
    assert res.duplicates == 0 and res.clusters == n and res.largest == 1 and res.pairs == 0
    assert np.array_equal(res.labels, np.arange(n, dtype=np.uint32)) and res.keep.all()
    assert np.array_equal(res.rep_ids, ids)


def test_empty_index(gpu_ctx):
    from ucfp_amd import text
    idx = text.LshIndex()
    for _ in range(2):                                   # never built, then rebuilt to empty
        res = idx.dedup(0.8)
        assert res.labels.shape == (0,) and res.rep_ids.shape == (0,) and res.keep.shape == (0,)
        assert (res.pairs, res.clusters, res.duplicates, res.largest) == (0, 0, 0, 0)
        idx.dedup_dev(103, 16, 0)                        # nothing to write: every output may be NULL
        rng = np.random.default_rng(1)
        idx.build(np.arange(9, dtype=np.uint64), records_of(rng.integers(0, 9, size=(9, 128), dtype=np.uint64)))
        idx.build(np.zeros(0, np.uint64), np.zeros((0, 1032), np.uint8))
    idx.close()


def test_optional_outputs_and_invalid_arguments(gpu_ctx, torch_cuda):
    from ucfp_amd import text
    from ucfp_amd.errors import InvalidArgument
    torch = torch_cuda
    rng = np.random.default_rng(21)
    base = rng.integers(0, 1 << 63, size=(40, 128), dtype=np.uint64)
    corpus = np.concatenate([base, base[:25], base[:10], rng.integers(0, 1 << 63, size=(200, 128), dtype=np.uint64)])
    corpus = corpus[rng.permutation(corpus.shape[0])]
    n = corpus.shape[0]
    ids = rng.permutation(np.arange(n, dtype=np.uint64)) * np.uint64(7)
    rec = records_of(corpus)
    want = dedup_ref(ids, rec, 16, 8, 128, 16)
    idx = text.LshIndex()
    idx.build(ids, rec)
    stream = torch.cuda.current_stream().cuda_stream
    for mask in range(8):
        lab = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        rep = torch.full((n,), -1, dtype=torch.int64, device="cuda")
        keep = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        st = torch.full((4,), -1, dtype=torch.int64, device="cuda")
        idx.dedup_dev(128, 16, lab.data_ptr(), rep.data_ptr() if mask & 1 else 0, keep.data_ptr() if mask & 2 else 0,
                      st.data_ptr() if mask & 4 else 0, stream)
        torch.cuda.synchronize()
        assert np.array_equal(lab.cpu().numpy().view(np.uint32), want[0])
        assert np.array_equal(rep.cpu().numpy().view(np.uint64), want[1] if mask & 1 else np.full(n, 2**64 - 1, np.uint64))
        assert np.array_equal(keep.cpu().numpy(), want[2].astype(np.uint8) if mask & 2 else np.full(n, 9, np.uint8))
        assert np.array_equal(st.cpu().numpy().view(np.uint64), want[3] if mask & 4 else np.full(4, 2**64 - 1, np.uint64))
    for bad in (0, 129):
        with pytest.raises(InvalidArgument):
            idx.dedup(min_agree=bad)
    with pytest.raises(InvalidArgument):
        idx.dedup_dev(103, 16, 0)                        # labels are required once rows exist
    with pytest.raises(InvalidArgument):
        idx.dedup(0.0)
    _check(idx.dedup(1.0), want)                          # threshold 1.0 -> min_agree 128
    idx.close()


def test_rebuild_leaves_no_state_behind(gpu_ctx):
    from ucfp_amd import text
    rng = np.random.default_rng(33)
    one = np.repeat(rng.integers(0, 1 << 63, size=(1, 128), dtype=np.uint64), 700, axis=0)      # one cluster of 700
    base = rng.integers(0, 1 << 63, size=(100, 128), dtype=np.uint64)
    two = np.concatenate([base, base[:30], rng.integers(0, 1 << 63, size=(170, 128), dtype=np.uint64)])
    two = two[rng.permutation(two.shape[0])]                                                    # 300 rows, pairs only
    idx = text.LshIndex()
    for corpus in (one, two, one[:50], two):
        ids = np.arange(corpus.shape[0], dtype=np.uint64) + np.uint64(100)
        rec = records_of(corpus)
        idx.build(ids, rec)
        for span in (16, 2):
            _check(idx.dedup(min_agree=120, span=span), dedup_ref(ids, rec, 16, 8, 120, span))
    idx.close()


def test_candidates_that_are_not_edges(gpu_ctx):
    """Two rows in one run that disagree elsewhere.  A run made by a 64-bit key collision (different slots, equal key)
    cannot be produced through real keys; what it exercises is `same key, low agreement`, which rows that share one
    band's slots exactly and nothing else cover: they are candidates and not an edge."""
    rng = np.random.default_rng(5)
    corpus = rng.integers(0, 1 << 63, size=(300, 128), dtype=np.uint64)
    corpus[17, 24:32] = corpus[200, 24:32]               # band 3 of 16 x 8
    corpus[40, 120:128] = corpus[41, 120:128]            # band 15
    corpus[90] = corpus[7]                               # one true duplicate
    ids = np.arange(300, dtype=np.uint64)
    rec = records_of(corpus)
    res = _dedup(ids, rec, 16, 8, 9, 16)                 # 8 equal slots are not enough
    _check(res, dedup_ref(ids, rec, 16, 8, 9, 16))
    assert (res.pairs, res.clusters, res.duplicates, res.largest) == (2 + 16, 299, 1, 2)
    assert res.labels[200] == 200 and res.labels[41] == 41 and res.labels[90] == 7
    res = _dedup(ids, rec, 16, 8, 8, 16)                 # ... until min_agree says they are
    _check(res, dedup_ref(ids, rec, 16, 8, 8, 16))
    assert res.labels[200] == 17 and res.labels[41] == 40 and res.duplicates == 3


def _random_corpus(seed):
    """n in 1 .. 50 000, a duplicate share of 0-60 % in clusters whose sizes follow a power law up to 500; a cluster's
    rows keep each slot of their base with one probability per cluster (1.0 = exact copies)."""
    rng = np.random.default_rng(77_000 + seed)
    n = int(rng.integers(1, 50_001))
    share = float(rng.uniform(0.0, 0.6))
    sizes = []
    left = int(n * share)
    while left >= 2:
        s = min(left, 500, 1 + int(rng.pareto(1.5) + 1))       # P(size >= s) ~ s^-1.5
        if s >= 2:
            sizes.append(s)
            left -= s
    sizes = np.array(sizes, np.int64)
    cl = np.repeat(np.arange(sizes.size), sizes)
    bases = rng.integers(0, 1 << 63, size=(sizes.size, 128), dtype=np.uint64)
    keep = rng.choice([1.0, 0.98, 0.9, 0.75], size=sizes.size)
    dup = np.where(rng.random((cl.size, 128)) < keep[cl][:, None], bases[cl],
                   rng.integers(0, 1 << 63, size=(cl.size, 128), dtype=np.uint64))
    corpus = np.concatenate([dup, rng.integers(0, 1 << 63, size=(n - cl.size, 128), dtype=np.uint64)])
    corpus = corpus[rng.permutation(n)]
    ids = rng.permutation(np.arange(n, dtype=np.uint64)) + np.uint64(1 << 33)
    bands, rows = SHAPES[int(rng.integers(0, len(SHAPES)))]
    span = int(rng.choice([1, 3, 16, 64]))
    min_agree = int(rng.choice([64, 90, 103, 115, 128]))
    return ids, records_of(corpus), bands, rows, min_agree, span


@pytest.mark.parametrize("seed", range(20))
def test_random_configurations(gpu_ctx, seed):
    ids, rec, bands, rows, min_agree, span = _random_corpus(seed)
    _check(_dedup(ids, rec, bands, rows, min_agree, span), dedup_ref(ids, rec, bands, rows, min_agree, span))


def test_dedup_corpus_on_text(gpu_ctx):
    import random
    from ucfp_amd import text
    rng = random.Random(5)
    vocab = ["w%03d" % i for i in range(500)]

    def doc(words):
        return " ".join(rng.choice(vocab) for _ in range(words))

    originals = [doc(150) for _ in range(12)]
    texts, first = [], {}

    def add(t, of=None):
        texts.append(t)
        if of is not None:
            first.setdefault(of, len(texts) - 1)
        return len(texts) - 1

    for i, t in enumerate(originals):
        add(t, i)
    texts.append("")                                               # no tokens: status != 0
    empty = len(texts) - 1
    exact = [(add(originals[i]), i) for i in (0, 3, 3, 7)]
    cased = [(add(originals[i].upper().replace(" ", "   ")), i) for i in (1, 3, 9)]
    cased.append((add("\t" + originals[5].title() + "\n"), 5))
    edited = []
    for i in (2, 4, 11):
        w = originals[i].split(" ")
        w[60] = "changed"
        edited.append((add(" ".join(w)), i))
    unrelated = [add(doc(150)) for _ in range(6)]
    accent = add("déjà vu " + doc(80))                   # non-ASCII: canonicalised on the host
    accent2 = add("DÉJÀ   VU " + texts[accent][8:].upper())
    keep, labels, status = text.dedup_corpus(texts, threshold=0.8)
    assert keep.dtype == bool and labels.dtype == np.int64 and keep.shape == labels.shape == (len(texts),)
    # the same through the restatement, on the records minhash_batch returns
    rec, st = text.minhash_batch(texts)
    assert np.array_equal(status, st)
    pos = np.flatnonzero(st == 0)
    r_lab, r_rep, r_keep, _ = dedup_ref(pos.astype(np.uint64), rec[pos], 16, 8, text.min_agree_for(0.8), 16)
    want_keep, want_labels = np.ones(len(texts), bool), np.arange(len(texts), dtype=np.int64)
    want_keep[pos], want_labels[pos] = r_keep, r_rep.astype(np.int64)
    assert np.array_equal(keep, want_keep) and np.array_equal(labels, want_labels)
    # what the recipe promises
    assert status[empty] != 0 and keep[empty] and labels[empty] == empty
    assert (np.delete(status, empty) == 0).all()
    for j, i in exact + cased:
        assert labels[j] == first[i] and not keep[j]
        assert np.array_equal(slots_of(rec[j]), slots_of(rec[first[i]]))          # agreement 128
    for j, i in edited:
        assert labels[j] == first[i] and not keep[j]
    for j in unrelated:
        assert keep[j] and labels[j] == j
    assert keep[accent] and labels[accent2] == accent and not keep[accent2]
    assert all(keep[first[i]] and labels[first[i]] == first[i] for i in range(12))
    assert text.dedup_corpus([])[0].shape == (0,)
