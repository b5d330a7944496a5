// panako_index.hip -- GPU index over Panako triplets that votes on (scale, offset) pairs: "which
// recording is this, where in it, and at what tempo?"  The third posting index on postings.h, after landmark.hip (A10)
// and bm25.hip (A11).
//
// Spec (ours; the reference has no audio matcher): A14 in DESIGN.md and the comment in include/ucfp_hip.h.  In short: a
// record and a query are sets of distinct triples (h, a, d) = (hash, t_a, t_c - t_a); a query triple probes the hashes
// that differ from h in the ratio bits r by at most r_slack; a match (query triple, posting) supports the scale
// hypotheses s with |256 d' - s d| <= 256 slack and has the offset a' - ((s a + 128) >> 8) under each; votes(r) is the
// largest number of matches of r that support one s with offsets inside one window of W frames.  The integer pieces
// live in panako_match.h, which the CPU tests compile on their own.
//
// Layout of a tenant after a (lazy) rebuild: postings sorted by (hash, a', d', ordinal), deduplicated, as two arrays --
// hashes u32 [P] and entries u64 [P] (a' << 33 | d' << 23 | ordinal, hence at most 2^23 records per tenant) -- plus a
// directory dir[b] = first posting whose hash >> 14 is >= b and the id of each ordinal (ordinals follow ascending id).
// The rebuild is postings.h's: two stable rocPRIM radix sorts (by entry, then by hash), the compaction with PkHead (a
// new (hash, entry) pair) and PkEmit, and post_directory on hash >> 14.
//
// Query (one launch sequence for a ragged batch):
//   pk_qprep / pk_qkeys   check the offsets, d in 1 ... 1023 and t_a < 2^28; per triple (a << 10 | d) and
//                         (query << 32 | hash)
//   rocPRIM               two stable radix sorts of the batch (by (a, d), then by (query, hash)): equal triples of a
//                         query become neighbours and the queries keep their ranges
//   pk_qruns              one block per query: |Q| and the expanded votes V = sum over matches of supported hypotheses
//   pk_vote               one block per query.  Slots (triple, probe) -> posting runs -> matches (a block scan of the
//                         run lengths) -> votes (ordinal, j, offset), every match as many as the interval of j it
//                         supports (pk_interval: two divisions; a second block scan places them).  A query with
//                         V <= kLdsVotes keeps its votes in LDS: bitonic sort, then every vote takes the number of
//                         votes of its (ordinal, j) inside the window that starts at its offset from a bisection for
//                         the window's end, and folds pk_best(count, rank of j, offset) into the best of its ordinal
//                         with one atomicMax; the qualifying ordinals are sorted by (votes desc, ordinal asc).  A larger
//                         query writes its votes to a global spill buffer instead.
//   spill path            rocPRIM segmented sort of the spilled votes; pk_spill_best: the same window count and fold
//                         into a dense per-(query, ordinal) row; pk_spill_topk scans the row 256 ordinals at a time
//                         into an LDS top-k (topk_offer).
// Both paths sort the same keys and fold the same values, so they agree bit for bit.  The host reads three small arrays
// per query batch (the checked sizes, the input flags, V per query) to size the sorts and the spill buffers.
//
// Scaled mode (bins = 1 in ucfp_panako_match_config_ex) finds resampled copies, whose bins moved with
// their speed: pk_qruns and pk_vote are templates over the mode, and only the walk from a query triple to its matches
// differs (for_each_match).  A triple visits the buckets (k_a', k_b') that some scale hypothesis allows instead of three
// probes, and a posting is tested against the ratio bits, three bin intervals and the d interval (pk_interval_scaled);
// a stopped hash is known by one byte per posting (pk_mark_stopped).  The bins = 0 instantiation is A14's code.

#include <hip/hip_runtime.h>

#include <map>
#include <unordered_map>
#include <vector>

#include "panako_match.h"
#include "postings.h"

namespace {

using ucfp::PkMatch;

constexpr uint32_t kDirBits = 14;                  // hash >> 14 = f_a | f_b
constexpr uint32_t kDirSize = 1u << 18;
constexpr uint32_t kLdsVotes = 2048;               // a query with more expanded votes goes through global memory
constexpr uint32_t kMaxRecords = 1u << ucfp::kPkOrdBits;
constexpr uint32_t kMaxTaRecord = 0x80000000u;     // t_a of a record below 2^31
constexpr uint32_t kMaxTaQuery = 1u << 28;         // t_a of a query below 2^28: every offset fits an int32
constexpr uint64_t kNoSpill = ~0ull;
constexpr uint32_t kErrOffsets = 1, kErrD = 2, kErrTa = 4, kErrCount = 8;

struct Postings {
    const uint32_t* hashes;
    const uint64_t* entries;
    const uint32_t* dir;
    uint32_t max_postings;
    const uint8_t* stop;   // scaled mode with max_postings > 0: stop[i] = posting i belongs to a stopped hash
};

struct Outputs {
    uint64_t* ids;
    uint32_t* votes;
    int32_t* offsets;
    uint32_t* scales;
    float* scores;
    uint32_t* n;
};

// candidate sort key: (votes desc, ordinal asc); kEmpty64 sorts last
__device__ __forceinline__ uint64_t cand_key(uint32_t votes, uint32_t ord) {
    return ((uint64_t)(0xffffffffu - votes) << 32) | ord;
}

// s_rank[j] = preference rank of hypothesis j, s_jof[rank] = j; ends with a barrier
__device__ __forceinline__ void fill_ranks(const PkMatch& m, uint32_t* s_rank, uint32_t* s_jof) {
    if (threadIdx.x < (uint32_t)m.nh) {
        const uint32_t r = ucfp::pk_pref_rank(m, (int32_t)threadIdx.x);
        s_rank[threadIdx.x] = r;
        s_jof[r] = threadIdx.x;
    }
    __syncthreads();
}

// s_key sorted ascending, n entries; one block writes query q's k results; best_of(ordinal) = the packed best
template <class BestOf>
__device__ void write_hits(const uint64_t* s_key, uint32_t n, uint32_t q, uint32_t k, uint32_t qn, const PkMatch& m,
                           const uint32_t* s_jof, const uint64_t* __restrict__ ids, const Outputs& out, BestOf best_of) {
    const uint32_t j = threadIdx.x;   // k <= UCFP_INDEX_MAX_K < kThreads
    const uint64_t sk = j < k && j < n ? s_key[j] : kEmpty64;
    const bool valid = sk != kEmpty64;
    if (j < k) {
        const size_t o = (size_t)q * k + j;
        uint64_t id = kEmpty64;
        uint32_t votes = 0, scale = 0;
        int32_t off = 0;
        if (valid) {
            const uint32_t ord = (uint32_t)sk;
            const uint64_t b = best_of(ord);
            id = ids[ord];
            votes = ucfp::pk_best_count(b);
            off = ucfp::pk_best_delta(b);
            scale = (uint32_t)(m.smin + (int32_t)s_jof[ucfp::pk_best_rank(b)] * m.step);
        }
        out.ids[o] = id;
        out.votes[o] = votes;
        out.offsets[o] = off;
        out.scales[o] = scale;
        out.scores[o] = valid ? (float)votes / (float)qn : -1.0f;
    }
    const int cnt = __syncthreads_count(valid);
    if (threadIdx.x == 0) out.n[q] = (uint32_t)cnt;
}

__device__ __forceinline__ void find_run(const uint32_t* __restrict__ hashes, const uint32_t* __restrict__ dir, uint32_t h,
                                         uint32_t& lo, uint32_t& len) {
    const uint32_t b = h >> kDirBits;
    const uint32_t a = dir[b], e = dir[b + 1];
    uint32_t l = a, r = e;
    while (l < r) {   // first >= h
        const uint32_t m = (l + r) >> 1;
        if (hashes[m] < h) l = m + 1;
        else r = m;
    }
    uint32_t u = l, r2 = e;
    while (u < r2) {  // first > h
        const uint32_t m = (u + r2) >> 1;
        if (hashes[m] <= h) u = m + 1;
        else r2 = m;
    }
    lo = l;
    len = u - l;
}

// first position in (i, e) of the sorted votes that is past the window of vote i (e when none is)
__device__ __forceinline__ uint64_t window_end(const uint64_t* votes, uint64_t i, uint64_t e, uint32_t window) {
    const uint64_t at = votes[i];
    uint64_t l = i + 1, r = e;
    while (l < r) {
        const uint64_t mid = (l + r) >> 1;
        if (ucfp::pk_past_window(votes[mid], at, window)) r = mid;
        else l = mid + 1;
    }
    return l;
}

// The matches of one query, by the whole block: the sorted triples [a, e) of qh (query << 32 | hash) and qad
// (t_a << 10 | d) give three slots each (one per probe; a duplicate of its predecessor and a probe that does not exist
// have an empty run), 256 slots at a time; a block scan of the run lengths lets every lane take the next match.
// f(valid, ordinal, a', a, jlo, jhi) is called by all threads together (it may hold barriers), valid on the lanes that
// carry a match; [jlo, jhi] is the interval of hypotheses the match supports (empty when jlo > jhi).  n_distinct counts
// this lane's distinct triples.
//
// Scaled mode (kBins = 1, A22) has no fixed number of slots per triple: the distinct triples are taken one after the
// other, and a slot is one k_a' that some hypothesis allows, 256 of them at a time.  The hypotheses of that k_a' bound
// k_b' and k_c'; hash >> 14 = k_a' << 9 | k_b' keys the directory, so the buckets of the slot are neighbours and the
// run is everything from (k_a', first k_b', first k_c') to (k_a', last k_b', last k_c', r = 31): every posting at most
// once per triple.  The slots are computed, not stored; most are empty, which two directory reads show, and a chunk
// of empty slots costs one barrier.  The ratio bits, the three bin intervals, the d interval and the stop flag are
// tested per posting (pk_interval_scaled).
template <int kBins, class F>
__device__ __forceinline__ void for_each_match(const uint64_t* __restrict__ qh, const uint64_t* __restrict__ qad, uint64_t a,
                                               uint64_t e, const Postings& P, const PkMatch& m, uint64_t* s_inc,
                                               uint32_t* s_lo, uint64_t* s_qad, uint64_t* s_w, uint64_t& n_distinct, F f) {
    if constexpr (kBins != 0) {
        const uint32_t nt = (uint32_t)(e - a);   // a batch holds fewer than 2^32 / 3 triples
        uint32_t hq = 0;
        uint64_t ad = 0;
        for (uint32_t i = 0; i < nt; i++) {
            const uint32_t hprev = hq;
            const uint64_t adprev = ad;
            hq = (uint32_t)qh[a + i];   // the upper half is the query
            ad = qad[a + i];
            if (i && hprev == hq && adprev == ad) continue;
            if (threadIdx.x == 0) n_distinct++;
            const int32_t ka = (int32_t)(hq >> 23), kb = (int32_t)((hq >> 14) & 511u), kc = (int32_t)((hq >> 5) & 511u);
            int32_t alo, ahi;
            ucfp::pk_bin_range(m, ka, 0, m.nh - 1, &alo, &ahi);
            for (int32_t c = alo; c <= ahi; c += kThreads) {
                const int32_t kap = c + (int32_t)threadIdx.x;
                uint32_t lo = 0, len = 0;
                if (kap <= ahi) {
                    int32_t jlo, jhi, blo, bhi, clo, chi;
                    ucfp::pk_bin_interval(m, ka, kap, m.f_slack, &jlo, &jhi);
                    if (jlo <= jhi) {
                        ucfp::pk_bin_range(m, kb, jlo, jhi, &blo, &bhi);
                        ucfp::pk_bin_range(m, kc, jlo, jhi, &clo, &chi);
                        if (blo <= bhi && clo <= chi) {
                            const uint32_t b0 = ((uint32_t)kap << 9) | (uint32_t)blo, b1 = ((uint32_t)kap << 9) | (uint32_t)bhi;
                            const uint32_t pa = P.dir[b0], pe = P.dir[b1 + 1];   // b1 + 1 <= kDirSize
                            if (pa < pe) {
                                const uint32_t h0 = (b0 << kDirBits) | ((uint32_t)clo << 5);
                                const uint32_t h1 = (b1 << kDirBits) | ((uint32_t)chi << 5) | 31u;
                                uint32_t l = pa, r = pe;
                                while (l < r) {   // first >= h0
                                    const uint32_t mid = (l + r) >> 1;
                                    if (P.hashes[mid] < h0) l = mid + 1;
                                    else r = mid;
                                }
                                uint32_t u = l, r2 = pe;
                                while (u < r2) {  // first > h1
                                    const uint32_t mid = (u + r2) >> 1;
                                    if (P.hashes[mid] <= h1) u = mid + 1;
                                    else r2 = mid;
                                }
                                lo = l;
                                len = u - l;
                            }
                        }
                    }
                }
                if (__syncthreads_count(len != 0) == 0) continue;
                s_inc[threadIdx.x] = block_scan_incl(len, s_w);
                s_lo[threadIdx.x] = lo;
                __syncthreads();
                const uint32_t total = (uint32_t)s_inc[kThreads - 1];   // the runs of a triple are disjoint: below 2^32
                for (uint32_t mb = 0; mb < total; mb += kThreads) {
                    const uint32_t j = mb + threadIdx.x;
                    const bool valid = j < total;
                    uint32_t ord = 0, ap = 0;
                    int32_t jlo = 0, jhi = -1;
                    if (valid) {
                        uint32_t l = 0, r = kThreads - 1;   // first slot x with s_inc[x] > j
                        while (l < r) {
                            const uint32_t mid = (l + r) >> 1;
                            if ((uint32_t)s_inc[mid] > j) r = mid;
                            else l = mid + 1;
                        }
                        const uint32_t excl = l ? (uint32_t)s_inc[l - 1] : 0u;
                        const size_t at = (size_t)s_lo[l] + (j - excl);
                        if (!(P.stop && P.stop[at])) {
                            const uint64_t ent = P.entries[at];
                            ord = ucfp::pk_entry_ord(ent);
                            ap = ucfp::pk_entry_a(ent);
                            ucfp::pk_interval_scaled(m, hq, (int32_t)(ad & 1023u), P.hashes[at], (int32_t)ucfp::pk_entry_d(ent),
                                                     &jlo, &jhi);
                        }
                    }
                    f(valid, ord, ap, (uint32_t)(ad >> 10), jlo, jhi);
                }
                __syncthreads();
            }
        }
        return;
    }
    const uint64_t nslots = 3 * (e - a);
    for (uint64_t c = 0; c < nslots; c += kThreads) {
        const uint64_t s = c + threadIdx.x;
        uint32_t lo = 0, len = 0;
        uint64_t ad = 0;
        if (s < nslots) {
            const uint64_t i = a + s / 3;
            const uint32_t p = (uint32_t)(s % 3);
            const uint64_t hq = qh[i];
            ad = qad[i];
            const bool dup = i > a && qh[i - 1] == hq && qad[i - 1] == ad;
            if (!dup) {
                if (p == 0) n_distinct++;
                uint32_t first, np;
                ucfp::pk_probes((uint32_t)hq, m.r_slack, &first, &np);
                if (p < np) {
                    find_run(P.hashes, P.dir, first + p, lo, len);
                    if (P.max_postings && len > P.max_postings) len = 0;
                }
            }
        }
        s_inc[threadIdx.x] = block_scan_incl(len, s_w);
        s_lo[threadIdx.x] = lo;
        s_qad[threadIdx.x] = ad;
        __syncthreads();
        const uint64_t total = s_inc[kThreads - 1];
        for (uint64_t mb = 0; mb < total; mb += kThreads) {
            const uint64_t j = mb + threadIdx.x;
            const bool valid = j < total;
            uint32_t ord = 0, ap = 0, qa = 0;
            int32_t jlo = 0, jhi = -1;
            if (valid) {
                uint32_t l = 0, r = kThreads - 1;   // first slot x with s_inc[x] > j
                while (l < r) {
                    const uint32_t mid = (l + r) >> 1;
                    if (s_inc[mid] > j) r = mid;
                    else l = mid + 1;
                }
                const uint64_t excl = l ? s_inc[l - 1] : 0;
                const uint64_t ent = P.entries[s_lo[l] + (j - excl)];
                const uint64_t tq = s_qad[l];
                ord = ucfp::pk_entry_ord(ent);
                ap = ucfp::pk_entry_a(ent);
                qa = (uint32_t)(tq >> 10);
                ucfp::pk_interval(m, (int32_t)(tq & 1023u), (int32_t)ucfp::pk_entry_d(ent), &jlo, &jhi);
            }
            f(valid, ord, ap, qa, jlo, jhi);
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- rebuild

// postings sorted by (hash, entry): a head is a new pair -- duplicates of one record are dropped
struct PkHead {
    const uint32_t* hashes;
    const uint64_t* ents;
    __device__ bool operator()(size_t i) const { return i == 0 || hashes[i] != hashes[i - 1] || ents[i] != ents[i - 1]; }
};

struct PkEmit {
    const uint32_t* hashes_in;
    const uint64_t* ents_in;
    uint32_t* hashes;
    uint64_t* entries;
    __device__ void operator()(size_t i, uint64_t o) const {
        hashes[o] = hashes_in[i];
        entries[o] = ents_in[i];
    }
};

// stop[i] = the hash of posting i has more than max_postings postings: the posting max_postings places after the first
// of its hash still carries it (scaled mode meets a posting without looking its hash up, so the flag travels with it)
__global__ void pk_mark_stopped(const uint32_t* __restrict__ hashes, size_t n, uint32_t max_postings, uint8_t* __restrict__ stop) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = hashes[i];
    size_t l = 0, r = i;   // first posting of h
    while (l < r) {
        const size_t mid = (l + r) >> 1;
        if (hashes[mid] < h) l = mid + 1;
        else r = mid;
    }
    const size_t far = l + max_postings;
    stop[i] = far < n && hashes[far] == h ? 1 : 0;
}

// ---------------------------------------------------------------- query

// one block: offsets (bytes) -> triple offsets; info[0] = triples in the batch
__global__ void pk_qprep(const uint64_t* __restrict__ off, size_t nq, uint64_t* __restrict__ toff,
                         uint64_t* __restrict__ info, uint32_t* __restrict__ err) {
    bool bad = false;
    for (size_t i = threadIdx.x; i <= nq; i += kThreads) {
        const uint64_t o = off[i];
        toff[i] = o >> 4;
        bad |= (o & 15) != 0;
        if (i == 0) bad |= o != 0;
        else bad |= o < off[i - 1];
    }
    if (bad) atomicOr(err, kErrOffsets);
    if (threadIdx.x == 0) info[0] = off[nq] >> 4;
}

// per record of the batch: ad = t_a << 10 | d and qh = query << 32 | hash
__global__ void pk_qkeys(const uint32_t* __restrict__ rec, size_t n, const uint64_t* __restrict__ toff, size_t nq,
                         uint64_t* __restrict__ ad, uint64_t* __restrict__ qh, uint32_t* __restrict__ err) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = rec[4 * i], ta = rec[4 * i + 1], tc = rec[4 * i + 3];
    const uint32_t d = tc - ta;
    uint32_t bad = 0;
    if (tc <= ta || d > ucfp::kPkMaxD) bad |= kErrD;
    if (ta >= kMaxTaQuery) bad |= kErrTa;
    if (bad) atomicOr(err, bad);
    size_t l = 0, r = nq;   // the query of record i: the last q with toff[q] <= i
    while (l + 1 < r) {
        const size_t mid = (l + r) >> 1;
        if (toff[mid] <= i) l = mid;
        else r = mid;
    }
    ad[i] = ((uint64_t)(ta & (kMaxTaQuery - 1)) << 10) | (d & 1023u);
    qh[i] = ((uint64_t)l << 32) | h;
}

// The plan as the kernel uses it.  Kept mode reads the kernel argument.  Scaled mode takes it through LDS, which moves
// its eight words and the constants the compiler derives from them (the reciprocal of the step) from scalar to vector
// registers: the kernels sit at the scalar register limit and have vector registers to spare, LDS bounding their
// occupancy.  Ends with a barrier in scaled mode.
template <int kBins>
__device__ __forceinline__ PkMatch plan_for(const PkMatch& m) {
    if constexpr (kBins == 0) {
        return m;
    } else {
        __shared__ PkMatch s_m;
        if (threadIdx.x == 0) s_m = m;
        __syncthreads();
        return s_m;
    }
}

// one block per query: qn[q] = |Q|, votes[q] = V (expanded votes)
template <int kBins>
__global__ __launch_bounds__(kThreads) void pk_qruns(const uint64_t* __restrict__ qh, const uint64_t* __restrict__ qad,
                                                      const uint64_t* __restrict__ toff, Postings P, PkMatch m_arg,
                                                      uint32_t* __restrict__ qn, uint64_t* __restrict__ votes) {
    __shared__ uint64_t s_inc[kThreads], s_qad[kThreads];
    __shared__ uint32_t s_lo[kThreads];
    __shared__ uint64_t s_w[4];
    const uint32_t q = blockIdx.x;
    const PkMatch m = plan_for<kBins>(m_arg);
    uint64_t n_local = 0, v_local = 0;
    for_each_match<kBins>(qh, qad, toff[q], toff[q + 1], P, m, s_inc, s_lo, s_qad, s_w, n_local,
                   [&](bool valid, uint32_t, uint32_t, uint32_t, int32_t jlo, int32_t jhi) {
                       if (valid && jhi >= jlo) v_local += (uint64_t)(jhi - jlo + 1);
                   });
    const uint64_t tq = block_scan_incl(n_local, s_w);
    const uint64_t tv = block_scan_incl(v_local, s_w);
    if (threadIdx.x == kThreads - 1) {
        qn[q] = (uint32_t)tq;
        votes[q] = tv;
    }
}

// one block per query
template <int kBins>
__global__ __launch_bounds__(kThreads) void pk_vote(const uint64_t* __restrict__ qh, const uint64_t* __restrict__ qad,
                                                     const uint64_t* __restrict__ toff, Postings P, PkMatch m_arg,
                                                     const uint32_t* __restrict__ qn, const uint64_t* __restrict__ votes,
                                                     const uint64_t* __restrict__ spill_base,
                                                     const uint64_t* __restrict__ ids, uint32_t k, uint32_t min_votes,
                                                     uint64_t* __restrict__ spill, Outputs out) {
    __shared__ uint64_t s_votes[kLdsVotes];   // the votes; later the candidates
    __shared__ uint64_t s_best[kLdsVotes];    // per distinct ordinal of the query, in ascending order
    __shared__ uint32_t s_ord[kLdsVotes];
    __shared__ uint64_t s_inc[kThreads], s_qad[kThreads];
    __shared__ uint32_t s_lo[kThreads];
    __shared__ uint64_t s_w[4];
    __shared__ uint64_t s_tot;
    __shared__ uint32_t s_rank[ucfp::kPkMaxHyp], s_jof[ucfp::kPkMaxHyp];
    __shared__ uint32_t s_cnt;
    const uint32_t q = blockIdx.x;
    const PkMatch m = plan_for<kBins>(m_arg);
    const uint64_t base = spill_base[q];
    const bool spilling = base != kNoSpill;
    const uint64_t nv = votes[q];
    fill_ranks(m, s_rank, s_jof);
    if (nv == 0) {
        write_hits(nullptr, 0, q, k, 1, m, s_jof, ids, out, [](uint32_t) { return 0ull; });
        return;
    }
    // the votes, in match order
    const uint64_t limit = spilling ? nv : (nv < kLdsVotes ? nv : kLdsVotes);
    uint64_t done = 0, unused = 0;
    for_each_match<kBins>(qh, qad, toff[q], toff[q + 1], P, m, s_inc, s_lo, s_qad, s_w, unused,
                   [&](bool valid, uint32_t ord, uint32_t ap, uint32_t qa, int32_t jlo, int32_t jhi) {
                       const uint32_t cnt = valid && jhi >= jlo ? (uint32_t)(jhi - jlo + 1) : 0u;
                       const uint64_t incl = block_scan_incl(cnt, s_w);
                       if (threadIdx.x == kThreads - 1) s_tot = incl;
                       __syncthreads();
                       const uint64_t pos = done + incl - cnt;
                       for (uint32_t t = 0; t < cnt; t++) {
                           const int32_t j = jlo + (int32_t)t;
                           const uint64_t key = ucfp::pk_vote_key(ord, (uint32_t)j, ucfp::pk_offset(m.smin + j * m.step, qa, ap));
                           if (pos + t < limit) {
                               if (spilling) spill[base + pos + t] = key;
                               else s_votes[pos + t] = key;
                           }
                       }
                       done += s_tot;
                       __syncthreads();
                   });
    if (spilling) return;
    const uint32_t v = (uint32_t)limit;
    uint32_t n = 1;
    while (n < v) n <<= 1;
    for (uint32_t i = v + threadIdx.x; i < n; i += kThreads) s_votes[i] = kEmpty64;
    for (uint32_t i = threadIdx.x; i < v; i += kThreads) s_best[i] = 0;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    bitonic_sort(s_votes, n);
    // per vote the count of its window, folded into the best of its ordinal (dense index = ordinal heads before it)
    uint32_t carry = 0;
    for (uint32_t c = 0; c < v; c += kThreads) {
        const uint32_t i = c + threadIdx.x;
        const bool valid = i < v;
        const uint64_t key = valid ? s_votes[i] : 0;
        const uint32_t ord = ucfp::pk_vote_ord(key);
        const bool head = valid && (i == 0 || ucfp::pk_vote_ord(s_votes[i - 1]) != ord);
        const uint32_t incl = carry + (uint32_t)block_scan_incl(head ? 1u : 0u, s_w);
        if (threadIdx.x == kThreads - 1) s_tot = incl;
        if (valid) {
            const uint32_t cnt = (uint32_t)(window_end(s_votes, i, v, (uint32_t)m.window) - i);
            atomicMax((unsigned long long*)&s_best[incl - 1],
                      (unsigned long long)ucfp::pk_best(cnt, s_rank[ucfp::pk_vote_j(key)], ucfp::pk_vote_delta(key)));
            if (head) s_ord[incl - 1] = ord;
        }
        __syncthreads();
        carry = (uint32_t)s_tot;
        __syncthreads();
    }
    // the qualifying ordinals, packed to the front of s_votes, then sorted
    const uint32_t minv = min_votes > 1 ? min_votes : 1u;
    for (uint32_t i = threadIdx.x; i < carry; i += kThreads) {
        const uint32_t cnt = ucfp::pk_best_count(s_best[i]);
        if (cnt >= minv) s_votes[atomicAdd(&s_cnt, 1u)] = cand_key(cnt, s_ord[i]);
    }
    __syncthreads();
    const uint32_t nc = s_cnt;
    n = 1;
    while (n < nc) n <<= 1;
    for (uint32_t i = nc + threadIdx.x; i < n; i += kThreads) s_votes[i] = kEmpty64;
    __syncthreads();
    bitonic_sort(s_votes, n);
    write_hits(s_votes, n, q, k, qn[q], m, s_jof, ids, out, [&](uint32_t ord) {
        uint32_t l = 0, r = carry;   // s_ord ascends
        while (l < r) {
            const uint32_t mid = (l + r) >> 1;
            if (s_ord[mid] < ord) l = mid + 1;
            else r = mid;
        }
        return s_best[l];
    });
}

// one block per spilled query s: sorted votes spill[soff[s] .. soff[s+1])
__global__ __launch_bounds__(kThreads) void pk_spill_best(const uint64_t* __restrict__ spill, const uint64_t* __restrict__ soff,
                                                           uint32_t n_ord, PkMatch m, uint64_t* __restrict__ best,
                                                           uint32_t* __restrict__ err) {
    __shared__ uint32_t s_rank[ucfp::kPkMaxHyp], s_jof[ucfp::kPkMaxHyp];
    fill_ranks(m, s_rank, s_jof);
    const uint32_t s = blockIdx.x;
    const uint64_t a = soff[s], e = soff[s + 1];
    uint64_t* row = best + (size_t)s * n_ord;
    for (uint64_t i = a + threadIdx.x; i < e; i += kThreads) {
        const uint64_t key = spill[i];
        uint64_t cnt = window_end(spill, i, e, (uint32_t)m.window) - i;
        if (cnt >> ucfp::kPkCountBits) {
            atomicOr(err, kErrCount);
            cnt = (1u << ucfp::kPkCountBits) - 1;
        }
        const uint32_t ord = ucfp::pk_vote_ord(key);
        if (ord < n_ord)
            atomicMax((unsigned long long*)&row[ord],
                      (unsigned long long)ucfp::pk_best((uint32_t)cnt, s_rank[ucfp::pk_vote_j(key)], ucfp::pk_vote_delta(key)));
    }
}

__global__ __launch_bounds__(kThreads) void pk_spill_topk(const uint64_t* __restrict__ best, const uint32_t* __restrict__ spill_q,
                                                           uint32_t n_ord, PkMatch m, const uint32_t* __restrict__ qn,
                                                           const uint64_t* __restrict__ ids, uint32_t k, uint32_t min_votes,
                                                           Outputs out) {
    __shared__ uint64_t s_key[2 * kThreads];
    __shared__ uint32_t s_rank[ucfp::kPkMaxHyp], s_jof[ucfp::kPkMaxHyp];
    fill_ranks(m, s_rank, s_jof);
    const uint32_t s = blockIdx.x;
    const uint64_t* row = best + (size_t)s * n_ord;
    const uint32_t minv = min_votes > 1 ? min_votes : 1u;
    for (uint32_t i = threadIdx.x; i < 2 * kThreads; i += kThreads) s_key[i] = kEmpty64;
    __syncthreads();
    for (uint32_t b = 0; b < n_ord; b += kThreads) {
        const uint32_t o = b + threadIdx.x;
        const uint32_t cnt = o < n_ord ? ucfp::pk_best_count(row[o]) : 0u;
        topk_offer(s_key, k, cnt >= minv ? cand_key(cnt, o) : kEmpty64);
    }
    const uint32_t q = spill_q[s];
    write_hits(s_key, k, q, k, qn[q], m, s_jof, ids, out, [&](uint32_t ord) { return row[ord]; });
}

// empty answers for every query (unknown tenant / empty batch)
__global__ void pk_empty(size_t nq, uint32_t k, Outputs out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq * k) {
        out.ids[i] = kEmpty64;
        out.votes[i] = 0;
        out.offsets[i] = 0;
        out.scales[i] = 0;
        out.scores[i] = -1.0f;
    }
    if (i < nq) out.n[i] = 0;
}

struct Record {   // the triples of a record as given (duplicates included): hash and a' << 33 | d' << 23
    std::vector<uint32_t> hashes;
    std::vector<uint64_t> ents;
};

struct Tenant {
    std::map<uint64_t, Record> recs;   // ascending id = ordinal order
    bool dirty = true;
    size_t postings = 0;               // deduplicated, valid when !dirty
    bool stop_valid = false;           // `stop` follows the postings (made by the first scaled query after a rebuild)
    DevArr hashes, entries, dir, ids, stop;
};

}  // namespace

struct ucfp_panako_index : ucfp::IndexCore {
    uint32_t max_postings = 0;
    std::unordered_map<uint32_t, Tenant> tenants;
    // rebuild workspace
    DevArr b_ent_a, b_ent_b, b_hash_a, b_hash_b, b_cnt, b_off, b_tmp;
    // query workspace
    DevArr q_rec, q_off, q_toff, q_info, q_ad_a, q_ad_b, q_qh_a, q_qh_b, q_tmp, q_qn, q_votes, q_sbase, q_soff, q_sq,
        q_spill_a, q_spill_b, q_best, q_out;
    std::vector<uint64_t> h_votes, h_sbase, h_soff;
    std::vector<uint32_t> h_sq;
};

namespace {

// offsets and every triple of a batch; max_ta = the bound on t_a (records 2^31, queries 2^28)
int check_batch_host(const uint8_t* records, const uint64_t* offsets, size_t n, uint32_t max_ta) {
    if (n && !offsets) return capi_fail(UCFP_E_INVALID, "offsets is NULL");
    if (!n) return UCFP_OK;
    if (offsets[0] != 0) return capi_fail(UCFP_E_INVALID, "offsets[0] must be 0");
    for (size_t i = 0; i < n; i++) {
        if (offsets[i + 1] < offsets[i]) return capi_fail(UCFP_E_INVALID, "offsets decrease at %zu", i);
        if (offsets[i + 1] & 15) return capi_fail(UCFP_E_INVALID, "record bytes of item %zu are not a multiple of 16", i);
    }
    if (offsets[n] && !records) return capi_fail(UCFP_E_INVALID, "records is NULL");
    const size_t m = offsets[n] / 16;
    for (size_t i = 0; i < m; i++) {
        uint32_t r[4];
        memcpy(r, records + 16 * i, 16);
        if (r[3] <= r[1] || r[3] - r[1] > ucfp::kPkMaxD)
            return capi_fail(UCFP_E_INVALID, "triple %zu has t_c - t_a outside 1 ... %u", i, ucfp::kPkMaxD);
        if (r[1] >= max_ta) return capi_fail(UCFP_E_INVALID, "triple %zu has t_a = %u >= %u", i, r[1], max_ta);
    }
    return UCFP_OK;
}

int plan_match(const ucfp_panako_match_config_ex* cfg, PkMatch* m) {
    static const ucfp_panako_match_config_ex dflt = {204, 320, 4, 16, 2, 1, 0, 0};
    if (!cfg) cfg = &dflt;
    if (!ucfp::pk_plan_ex(cfg->scale_min, cfg->scale_max, cfg->scale_step, cfg->window, cfg->slack, cfg->r_slack, cfg->bins,
                          cfg->f_slack, m))
        return capi_fail(UCFP_E_INVALID,
                         "match config out of range: scales 64 <= min <= max <= 1024 in at most %u steps >= 1, window 1 ... 256, "
                         "slack 0 ... 8, r_slack 0 or 1, bins 0 or 1, f_slack 0 ... %u and 0 with bins = 0",
                         ucfp::kPkMaxHyp, ucfp::kPkMaxFSlack);
    return UCFP_OK;
}

// the old struct as the new one: the bins are kept
const ucfp_panako_match_config_ex* widen(const ucfp_panako_match_config* cfg, ucfp_panako_match_config_ex* ex) {
    if (!cfg) return nullptr;
    *ex = {cfg->scale_min, cfg->scale_max, cfg->scale_step, cfg->window, cfg->slack, cfg->r_slack, 0, 0};
    return ex;
}

int rebuild(ucfp_panako_index* ix, Tenant& T, hipStream_t st) {
    size_t n = 0;
    for (auto& kv : T.recs) n += kv.second.hashes.size();
    if (T.recs.size() > kMaxRecords)
        return capi_fail(UCFP_E_INVALID, "too many records in one tenant (%zu > %u)", T.recs.size(), kMaxRecords);
    if (n >= 0xffffffffull) return capi_fail(UCFP_E_INVALID, "too many triples in one tenant (%zu)", n);
    std::vector<uint64_t> h_ents(n), h_ids(T.recs.size());
    std::vector<uint32_t> h_hashes(n);
    size_t o = 0;
    uint32_t ord = 0;
    for (auto& kv : T.recs) {
        const Record& r = kv.second;
        h_ids[ord] = kv.first;
        for (size_t j = 0; j < r.ents.size(); j++) {
            h_ents[o + j] = r.ents[j] | ord;
            h_hashes[o + j] = r.hashes[j];
        }
        o += r.ents.size();
        ord++;
    }
    int rc;
    if ((rc = T.ids.ensure(h_ids.size() * 8)) || (rc = T.dir.ensure((kDirSize + 1) * 4))) return rc;
    if (!h_ids.empty()) HIP_TRY(hipMemcpyAsync(T.ids.p, h_ids.data(), h_ids.size() * 8, hipMemcpyHostToDevice, st));
    size_t p = 0;
    if (n) {
        if ((rc = ix->b_ent_a.ensure(n * 8)) || (rc = ix->b_ent_b.ensure(n * 8)) || (rc = ix->b_hash_a.ensure(n * 4)) ||
            (rc = ix->b_hash_b.ensure(n * 4)))
            return rc;
        uint64_t *ea = ix->b_ent_a.as<uint64_t>(), *eb = ix->b_ent_b.as<uint64_t>();
        uint32_t *ha = ix->b_hash_a.as<uint32_t>(), *hb = ix->b_hash_b.as<uint32_t>();
        HIP_TRY(hipMemcpyAsync(ea, h_ents.data(), n * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ha, h_hashes.data(), n * 4, hipMemcpyHostToDevice, st));
        // two stable passes: by entry (a', d', ordinal) into (eb, hb), then by hash back into (ha, ea)
        const PkHead head{ha, ea};
        if ((rc = sort_pairs(ix->b_tmp, ea, eb, ha, hb, n, 64, st)) || (rc = sort_pairs(ix->b_tmp, hb, ha, eb, ea, n, 32, st)) ||
            (rc = count_heads(head, n, ix->b_cnt, ix->b_off, st, &p)) || (rc = T.hashes.ensure(p * 4)) ||
            (rc = T.entries.ensure(p * 8)) ||
            (rc = compact_heads(head, PkEmit{ha, ea, T.hashes.as<uint32_t>(), T.entries.as<uint64_t>()}, n, ix->b_off, st)))
            return rc;
    } else if ((rc = T.hashes.ensure(0)) || (rc = T.entries.ensure(0))) {
        return rc;
    }
    if ((rc = build_directory(T.hashes.as<uint32_t>(), p, kDirBits, kDirSize, T.dir.as<uint32_t>(), st))) return rc;
    HIP_TRY(hipStreamSynchronize(st));   // the host vectors above go out of scope
    T.postings = p;
    T.dirty = false;
    T.stop_valid = false;
    return UCFP_OK;
}

int do_upsert(ucfp_panako_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* records, const uint64_t* offsets,
              size_t n) {
    int rc = check_batch_host(records, offsets, n, kMaxTaRecord);
    if (rc) return rc;
    if (n && !ids) return capi_fail(UCFP_E_INVALID, "ids is NULL");
    if (!n) return UCFP_OK;
    Tenant& T = ix->tenants[tenant];
    for (size_t i = 0; i < n; i++) {
        const size_t a = offsets[i] / 16, m = (offsets[i + 1] - offsets[i]) / 16;
        Record& r = T.recs[ids[i]];
        r.hashes.resize(m);
        r.ents.resize(m);
        for (size_t j = 0; j < m; j++) {
            uint32_t t[4];
            memcpy(t, records + 16 * (a + j), 16);
            r.hashes[j] = t[0];
            r.ents[j] = ucfp::pk_entry(0, t[1], t[3] - t[1]);
        }
    }
    T.dirty = true;
    return UCFP_OK;
}

int query_impl(ucfp_panako_index* ix, uint32_t tenant, const uint8_t* d_rec, const uint64_t* d_off, size_t nq, uint32_t k,
               uint32_t min_votes, const PkMatch& m, const Outputs& out, hipStream_t st) {
    int rc;
    // 1. the offsets and the triples (checked before anything else, whatever the tenant or k)
    if ((rc = ix->q_toff.ensure((nq + 1) * 8)) || (rc = ix->q_info.ensure(16))) return rc;
    HIP_TRY(hipMemsetAsync(ix->q_info.p, 0, 16, st));
    uint32_t* d_err = reinterpret_cast<uint32_t*>(ix->q_info.as<uint64_t>() + 1);
    const uint64_t* toff = ix->q_toff.as<uint64_t>();
    hipLaunchKernelGGL(pk_qprep, dim3(1), dim3(kThreads), 0, st, d_off, nq, ix->q_toff.as<uint64_t>(),
                       ix->q_info.as<uint64_t>(), d_err);
    HIP_TRY(hipGetLastError());
    uint64_t info[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(info, ix->q_info.p, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (info[1]) return capi_fail(UCFP_E_INVALID, "query offsets must start at 0, not decrease and be multiples of 16");
    const size_t total = (size_t)info[0];
    if (total && !d_rec) return capi_fail(UCFP_E_INVALID, "records is NULL");
    if (total >= 0xffffffffull / 3) return capi_fail(UCFP_E_INVALID, "too many query triples");
    if ((rc = ix->q_ad_a.ensure(total * 8)) || (rc = ix->q_ad_b.ensure(total * 8)) || (rc = ix->q_qh_a.ensure(total * 8)) ||
        (rc = ix->q_qh_b.ensure(total * 8)))
        return rc;
    uint64_t *ad_a = ix->q_ad_a.as<uint64_t>(), *ad_b = ix->q_ad_b.as<uint64_t>();
    uint64_t *qh_a = ix->q_qh_a.as<uint64_t>(), *qh_b = ix->q_qh_b.as<uint64_t>();
    if (total) {
        hipLaunchKernelGGL(pk_qkeys, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const uint32_t*)d_rec, total,
                           toff, nq, ad_a, qh_a, d_err);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(info + 1, d_err, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (info[1] & kErrD) return capi_fail(UCFP_E_INVALID, "a query triple has t_c - t_a outside 1 ... %u", ucfp::kPkMaxD);
        if (info[1] & kErrTa) return capi_fail(UCFP_E_INVALID, "a query triple has t_a >= 2^28");
    }
    if (k == 0) {
        HIP_TRY(hipMemsetAsync(out.n, 0, nq * 4, st));
        return UCFP_OK;
    }
    auto it = ix->tenants.find(tenant);
    if (it == ix->tenants.end() || total == 0) {
        hipLaunchKernelGGL(pk_empty, dim3((unsigned)((nq * k + 255) / 256)), dim3(256), 0, st, nq, k, out);
        HIP_TRY(hipGetLastError());
        return UCFP_OK;
    }
    Tenant& T = it->second;
    if (T.dirty && (rc = rebuild(ix, T, st))) return rc;
    Postings P{T.hashes.as<uint32_t>(), T.entries.as<uint64_t>(), T.dir.as<uint32_t>(), ix->max_postings, nullptr};
    if (m.bins && ix->max_postings && T.postings) {
        if (!T.stop_valid) {
            if ((rc = T.stop.ensure(T.postings))) return rc;
            hipLaunchKernelGGL(pk_mark_stopped, dim3((unsigned)((T.postings + 255) / 256)), dim3(256), 0, st, P.hashes,
                               T.postings, ix->max_postings, T.stop.as<uint8_t>());
            HIP_TRY(hipGetLastError());
            T.stop_valid = true;
        }
        P.stop = T.stop.as<uint8_t>();
    }
    // 2. equal triples of a query next to each other: stable sorts by (a, d), then by (query, hash); |Q| and V
    int qbits = 1;
    while (qbits < 32 && ((size_t)1 << qbits) < nq) qbits++;
    if ((rc = sort_pairs(ix->q_tmp, ad_a, ad_b, qh_a, qh_b, total, 38, st)) ||
        (rc = sort_pairs(ix->q_tmp, qh_b, qh_a, ad_b, ad_a, total, 32 + qbits, st)))
        return rc;
    if ((rc = ix->q_qn.ensure(nq * 4)) || (rc = ix->q_votes.ensure(nq * 8)) || (rc = ix->q_sbase.ensure(nq * 8))) return rc;
    hipLaunchKernelGGL(m.bins ? pk_qruns<1> : pk_qruns<0>, dim3((unsigned)nq), dim3(kThreads), 0, st, qh_a, ad_a, toff, P, m, ix->q_qn.as<uint32_t>(),
                       ix->q_votes.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    ix->h_votes.resize(nq);
    HIP_TRY(hipMemcpyAsync(ix->h_votes.data(), ix->q_votes.p, nq * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // 3. which queries go through global memory
    ix->h_sbase.assign(nq, kNoSpill);
    ix->h_soff.assign(1, 0);
    ix->h_sq.clear();
    bool count_may_overflow = false;
    for (size_t q = 0; q < nq; q++) {
        const uint64_t v = ix->h_votes[q];
        if (v >> 32) return capi_fail(UCFP_E_UNSUPPORTED, "query %zu expands to %llu votes (2^32 or more)", q, (unsigned long long)v);
        if (v > kLdsVotes) {
            ix->h_sbase[q] = ix->h_soff.back();
            ix->h_soff.push_back(ix->h_soff.back() + v);
            ix->h_sq.push_back((uint32_t)q);
            count_may_overflow |= (v >> ucfp::kPkCountBits) != 0;
        }
    }
    const size_t n_spill = ix->h_sq.size(), n_votes = ix->h_soff.back();
    const uint32_t n_ord = (uint32_t)T.recs.size();
    if (n_spill && n_votes >= 0xffffffffull)
        return capi_fail(UCFP_E_UNSUPPORTED, "a query batch expands to %zu votes in global memory (2^32 - 1 or more)", n_votes);
    HIP_TRY(hipMemcpyAsync(ix->q_sbase.p, ix->h_sbase.data(), nq * 8, hipMemcpyHostToDevice, st));
    if (n_spill) {
        if ((rc = ix->q_spill_a.ensure(n_votes * 8)) || (rc = ix->q_spill_b.ensure(n_votes * 8)) ||
            (rc = ix->q_soff.ensure((n_spill + 1) * 8)) || (rc = ix->q_sq.ensure(n_spill * 4)) ||
            (rc = ix->q_best.ensure(n_spill * n_ord * 8)))
            return rc;
        HIP_TRY(hipMemcpyAsync(ix->q_soff.p, ix->h_soff.data(), (n_spill + 1) * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ix->q_sq.p, ix->h_sq.data(), n_spill * 4, hipMemcpyHostToDevice, st));
    }
    // 4. votes: in LDS, or to the spill buffer
    hipLaunchKernelGGL(m.bins ? pk_vote<1> : pk_vote<0>, dim3((unsigned)nq), dim3(kThreads), 0, st, qh_a, ad_a, toff, P, m, ix->q_qn.as<uint32_t>(),
                       ix->q_votes.as<uint64_t>(), ix->q_sbase.as<uint64_t>(), T.ids.as<uint64_t>(), k, min_votes,
                       n_spill ? ix->q_spill_a.as<uint64_t>() : nullptr, out);
    HIP_TRY(hipGetLastError());
    if (n_spill) {
        const uint64_t* so = ix->q_soff.as<uint64_t>();
        if ((rc = sort_segments(ix->q_tmp, ix->q_spill_a.as<uint64_t>(), ix->q_spill_b.as<uint64_t>(), n_votes, n_spill, so,
                                st)))
            return rc;
        HIP_TRY(hipMemsetAsync(ix->q_best.p, 0, n_spill * n_ord * 8, st));
        hipLaunchKernelGGL(pk_spill_best, dim3((unsigned)n_spill), dim3(kThreads), 0, st, ix->q_spill_b.as<uint64_t>(), so,
                           n_ord, m, ix->q_best.as<uint64_t>(), d_err);
        hipLaunchKernelGGL(pk_spill_topk, dim3((unsigned)n_spill), dim3(kThreads), 0, st, ix->q_best.as<uint64_t>(),
                           ix->q_sq.as<uint32_t>(), n_ord, m, ix->q_qn.as<uint32_t>(), T.ids.as<uint64_t>(), k, min_votes, out);
        HIP_TRY(hipGetLastError());
        if (count_may_overflow) {   // only a query of 2^26 votes or more can fill the count field of the packed best
            HIP_TRY(hipMemcpyAsync(info + 1, d_err, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (info[1] & kErrCount) return capi_fail(UCFP_E_UNSUPPORTED, "a window holds 2^26 votes or more");
        }
    }
    return UCFP_OK;
}

int query_args(ucfp_panako_index* ix, const uint64_t* offsets, size_t nq, uint32_t k, const ucfp_panako_match_config_ex* cfg,
               PkMatch* m, const Outputs& out) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (k > UCFP_INDEX_MAX_K) return capi_fail(UCFP_E_INVALID, "k = %u exceeds UCFP_INDEX_MAX_K = %u", k, UCFP_INDEX_MAX_K);
    if (nq > 0x7fffffffu) return capi_fail(UCFP_E_INVALID, "too many queries");
    const int rc = plan_match(cfg, m);
    if (rc) return rc;
    if (nq && (!offsets || !out.n)) return capi_fail(UCFP_E_INVALID, "offsets/out_n is NULL");
    if (nq && k && (!out.ids || !out.votes || !out.offsets || !out.scales || !out.scores))
        return capi_fail(UCFP_E_INVALID, "an output buffer is NULL");
    return UCFP_OK;
}

}  // namespace

extern "C" {

uint32_t ucfp_panako_index_lds_votes(void) { return kLdsVotes; }

int ucfp_panako_index_create(ucfp_ctx* ctx, uint32_t max_postings, uint32_t flags, ucfp_panako_index** out) {
    if (!ctx || !out) return capi_fail(UCFP_E_INVALID, "ctx/out is NULL");
    *out = nullptr;
    if (flags != 0) return capi_fail(UCFP_E_INVALID, "no Panako index flags are defined (got %u)", flags);
    const int rc = ucfp::create_index(ctx, "Panako index", out);
    if (!rc) (*out)->max_postings = max_postings;
    return rc;
}

void ucfp_panako_index_destroy(ucfp_panako_index* ix) {
    if (!ix) return;
    ix->quiesce();
    for (auto& kv : ix->tenants)
        for (DevArr* a : {&kv.second.hashes, &kv.second.entries, &kv.second.dir, &kv.second.ids, &kv.second.stop}) a->release();
    for (DevArr* a : {&ix->b_ent_a, &ix->b_ent_b, &ix->b_hash_a, &ix->b_hash_b, &ix->b_cnt, &ix->b_off, &ix->b_tmp, &ix->q_rec,
                      &ix->q_off, &ix->q_toff, &ix->q_info, &ix->q_ad_a, &ix->q_ad_b, &ix->q_qh_a, &ix->q_qh_b, &ix->q_tmp,
                      &ix->q_qn, &ix->q_votes, &ix->q_sbase, &ix->q_soff, &ix->q_sq, &ix->q_spill_a, &ix->q_spill_b,
                      &ix->q_best, &ix->q_out})
        a->release();
    delete ix;
}

int ucfp_panako_index_upsert(ucfp_panako_index* ix, uint32_t tenant, const uint64_t* ids, const uint8_t* records,
                             const uint64_t* offsets, size_t n) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    return do_upsert(ix, tenant, ids, records, offsets, n);
}

int ucfp_panako_index_upsert_dev(ucfp_panako_index* ix, uint32_t tenant, const uint64_t* d_ids, const uint8_t* d_records,
                                 const uint64_t* d_offsets, size_t n, void* stream) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (!n) return UCFP_OK;
    if (!d_ids || !d_offsets) return capi_fail(UCFP_E_INVALID, "ids/offsets is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t st = (hipStream_t)stream;
    // the record table lives on the host (mutations are bookkeeping; the postings are rebuilt at the next query)
    std::vector<uint64_t> ids(n), offs(n + 1);
    HIP_TRY(hipMemcpyAsync(ids.data(), d_ids, n * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(offs.data(), d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (offs[0] != 0 || offs[n] < offs[0]) return capi_fail(UCFP_E_INVALID, "offsets must start at 0 and not decrease");
    std::vector<uint8_t> rec(offs[n]);
    if (offs[n]) {
        if (!d_records) return capi_fail(UCFP_E_INVALID, "records is NULL");
        HIP_TRY(hipMemcpyAsync(rec.data(), d_records, offs[n], hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return do_upsert(ix, tenant, ids.data(), rec.data(), offs.data(), n);
}

int ucfp_panako_index_delete(ucfp_panako_index* ix, uint32_t tenant, const uint64_t* ids, size_t n, size_t* n_removed) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    if (n && !ids) return capi_fail(UCFP_E_INVALID, "ids is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    size_t removed = 0;
    auto it = ix->tenants.find(tenant);
    if (it != ix->tenants.end()) {
        for (size_t i = 0; i < n; i++) removed += it->second.recs.erase(ids[i]);
        if (removed) it->second.dirty = true;
    }
    if (n_removed) *n_removed = removed;
    return UCFP_OK;
}

int ucfp_panako_index_size(ucfp_panako_index* ix, uint32_t tenant, size_t* records, size_t* postings) {
    if (!ix) return capi_fail(UCFP_E_INVALID, "index is NULL");
    std::lock_guard<std::mutex> lk(ix->mu);
    size_t r = 0, p = 0;
    auto it = ix->tenants.find(tenant);
    if (it != ix->tenants.end()) {
        Tenant& T = it->second;
        if (T.dirty) {
            int rc = ix->begin();
            if (rc || (rc = rebuild(ix, T, ix->own)) || (rc = ix->end(ix->own))) return rc;
        }
        r = T.recs.size();
        p = T.postings;
    }
    if (records) *records = r;
    if (postings) *postings = p;
    return UCFP_OK;
}

int ucfp_panako_index_flush(ucfp_panako_index* ix) { return ucfp::flush_dirty(ix, rebuild); }

int ucfp_panako_index_query_ex_dev(ucfp_panako_index* ix, uint32_t tenant, const uint8_t* d_records, const uint64_t* d_offsets,
                                   size_t nq, uint32_t k, uint32_t min_votes, const ucfp_panako_match_config_ex* cfg,
                                   uint64_t* d_out_ids, uint32_t* d_out_votes, int32_t* d_out_offsets, uint32_t* d_out_scales,
                                   float* d_out_scores, uint32_t* d_out_n, void* stream) {
    const Outputs out{d_out_ids, d_out_votes, d_out_offsets, d_out_scales, d_out_scores, d_out_n};
    PkMatch m;
    int rc = query_args(ix, d_offsets, nq, k, cfg, &m, out);
    if (rc || nq == 0) return rc;
    std::lock_guard<std::mutex> lk(ix->mu);
    if ((rc = ix->begin())) return rc;
    hipStream_t st = (hipStream_t)stream;
    rc = query_impl(ix, tenant, d_records, d_offsets, nq, k, min_votes, m, out, st);
    return ix->end(st, rc);
}

int ucfp_panako_index_query_ex(ucfp_panako_index* ix, uint32_t tenant, const uint8_t* records, const uint64_t* offsets,
                               size_t nq, uint32_t k, uint32_t min_votes, const ucfp_panako_match_config_ex* cfg,
                               uint64_t* out_ids, uint32_t* out_votes, int32_t* out_offsets, uint32_t* out_scales,
                               float* out_scores, uint32_t* out_n) {
    PkMatch m;
    int rc = query_args(ix, offsets, nq, k, cfg, &m, Outputs{out_ids, out_votes, out_offsets, out_scales, out_scores, out_n});
    if (rc || nq == 0) return rc;
    if ((rc = check_batch_host(records, offsets, nq, kMaxTaQuery))) return rc;
    std::lock_guard<std::mutex> lk(ix->mu);
    if ((rc = ix->begin())) return rc;
    hipStream_t st = ix->own;
    const size_t bytes = offsets[nq], nk = nq * k;
    const size_t o_votes = nk * 8, o_offs = o_votes + nk * 4, o_scl = o_offs + nk * 4, o_sc = o_scl + nk * 4, o_n = o_sc + nk * 4;
    if ((rc = ix->q_rec.ensure(bytes)) || (rc = ix->q_off.ensure((nq + 1) * 8)) || (rc = ix->q_out.ensure(o_n + nq * 4)))
        return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync(ix->q_rec.p, records, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(ix->q_off.p, offsets, (nq + 1) * 8, hipMemcpyHostToDevice, st));
    uint8_t* ob = ix->q_out.as<uint8_t>();
    const Outputs dev{(uint64_t*)ob,         (uint32_t*)(ob + o_votes), (int32_t*)(ob + o_offs),
                      (uint32_t*)(ob + o_scl), (float*)(ob + o_sc),     (uint32_t*)(ob + o_n)};
    rc = query_impl(ix, tenant, ix->q_rec.as<uint8_t>(), ix->q_off.as<uint64_t>(), nq, k, min_votes, m, dev, st);
    if (rc) return ix->end_sync(rc);
    if (nk) {
        HIP_TRY(hipMemcpyAsync(out_ids, dev.ids, nk * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_votes, dev.votes, nk * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_offsets, dev.offsets, nk * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_scales, dev.scales, nk * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(out_scores, dev.scores, nk * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(out_n, dev.n, nq * 4, hipMemcpyDeviceToHost, st));
    return ix->end_sync(UCFP_OK);
}

int ucfp_panako_index_query_dev(ucfp_panako_index* ix, uint32_t tenant, const uint8_t* d_records, const uint64_t* d_offsets,
                                size_t nq, uint32_t k, uint32_t min_votes, const ucfp_panako_match_config* cfg,
                                uint64_t* d_out_ids, uint32_t* d_out_votes, int32_t* d_out_offsets, uint32_t* d_out_scales,
                                float* d_out_scores, uint32_t* d_out_n, void* stream) {
    ucfp_panako_match_config_ex ex;
    return ucfp_panako_index_query_ex_dev(ix, tenant, d_records, d_offsets, nq, k, min_votes, widen(cfg, &ex), d_out_ids,
                                          d_out_votes, d_out_offsets, d_out_scales, d_out_scores, d_out_n, stream);
}

int ucfp_panako_index_query(ucfp_panako_index* ix, uint32_t tenant, const uint8_t* records, const uint64_t* offsets, size_t nq,
                            uint32_t k, uint32_t min_votes, const ucfp_panako_match_config* cfg, uint64_t* out_ids,
                            uint32_t* out_votes, int32_t* out_offsets, uint32_t* out_scales, float* out_scores,
                            uint32_t* out_n) {
    ucfp_panako_match_config_ex ex;
    return ucfp_panako_index_query_ex(ix, tenant, records, offsets, nq, k, min_votes, widen(cfg, &ex), out_ids, out_votes,
                                      out_offsets, out_scales, out_scores, out_n);
}

}  // extern "C"
