"""Measures the HTML -> text stage on pages resident in device memory.

    python tools/bench_text_html.py [--pages 100000] [--distinct 512] [--runs 7] [--warmup 2]

Input: `--distinct` generated pages of about 4 KiB of visible text each (markup, script and style blocks, comments,
attributes and character references around it), tiled on the device to `--pages` documents.  Reported, each as the median
of `--runs` timed calls with the smallest and the largest beside it (device events around the call, nothing else queued):

    html      ucfp_text_html_batch_dev over the pages              ms, GB/s of page bytes
    canon     ucfp_text_canon_batch_dev over the stripped bytes    ms, GB/s of stripped bytes: the existing two-pass byte
                                                                   streamer, as the yardstick
    minhash   ucfp_text_minhash_batch_dev (RAW_ASCII) over them    ms, GB/s of stripped bytes: what the stage feeds
    host      an html.parser loop over 1000 of the pages           MB/s of page bytes, one thread

The stripped bytes of the first `--distinct` documents are compared with html.parser's before anything is timed.  Prints
one JSON line."""
import argparse
import json
import os
import random
import statistics
import sys
import time
from html.parser import HTMLParser

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WORDS = ("the quick brown fox jumps over a lazy dog while seven wizards quietly mix potions near this frozen lake and nobody "
         "expects any answer before dawn breaks again over silent northern hills where rivers carry old stories toward "
         "distant harbours full of lanterns markets sailors merchants letters maps").split()
INLINE = {"a", "abbr", "b", "bdi", "bdo", "big", "cite", "code", "data", "del", "dfn", "em", "font", "i", "ins", "kbd", "label",
          "mark", "q", "s", "samp", "small", "span", "strike", "strong", "sub", "sup", "time", "tt", "u", "var", "wbr"}


def gen_page(rng: random.Random, text_bytes: int = 4096) -> str:
    """A page in the shape of an article: head with style and script, a navigation list, paragraphs with inline markup,
    attributes, comments and references.  The visible text is ASCII."""
    def words(n):
        return " ".join(rng.choice(WORDS) for _ in range(n))

    def inline(s):
        r = rng.random()
        if r < 0.10:
            return '<a href="/%s?id=%d&amp;ref=nav" title="%s">%s</a>' % (rng.choice(WORDS), rng.randrange(10 ** 6), words(2), s)
        if r < 0.18:
            tag = ("em", "strong", "span", "code")[rng.randrange(4)]
            return "<%s class='%s'>%s</%s>" % (tag, rng.choice(WORDS), s, tag)
        if r < 0.22:
            return s + rng.choice([" &amp; ", " &lt; ", " &gt; ", " &quot;", "&#39;s ", " &#x2D; "])
        return s
    out = ['<!DOCTYPE html>\n<html lang="en">\n<head>\n<meta charset="utf-8">\n<title>%s</title>\n' % words(5),
           "<style>\nbody > div.main { margin: 0 auto; max-width: 60em }\n%s</style>\n"
           % "".join(".c%d > a:hover { color: #%06x }\n" % (i, rng.randrange(1 << 24)) for i in range(12)),
           '<script type="text/javascript">\nvar cfg = {id: %d, tags: "<b>"};\nfor (var i = 0; i < cfg.id && i > -1; i++) { track("</p>", i); }\n'
           "</script>\n</head>\n<body>\n" % rng.randrange(10 ** 6),
           '<ul class="nav">\n%s</ul>\n' % "".join('<li><a href="/%s">%s</a></li>\n' % (w, w.title()) for w in rng.sample(WORDS, 8))]
    made = 0
    while made < text_bytes:
        n = rng.randrange(20, 90)
        para = " ".join(inline(rng.choice(WORDS)) for _ in range(n))
        made += 6 * n
        out.append('<div class="c%d" id="p%d">\n<h2>%s</h2>\n<p>%s</p>\n<!-- block %d: a > b -- c -->\n</div>\n'
                   % (rng.randrange(12), made, words(4), para, made))
        if rng.random() < 0.3:
            out.append('<img src="/img/%d.png" alt="%s"/><br>\n' % (rng.randrange(10 ** 4), words(3)))
    out.append('<script>window.done = 1 < 2;</script>\n</body>\n</html>\n')
    return "".join(out)


class _Text(HTMLParser):
    def __init__(self):
        super().__init__(convert_charrefs=True)
        self.out, self.raw = [], None

    def handle_starttag(self, tag, attrs):
        if tag not in INLINE:
            self.out.append(" ")
        if tag in ("script", "style"):
            self.raw = tag

    def handle_endtag(self, tag):
        if tag not in INLINE:
            self.out.append(" ")
        if tag == self.raw:
            self.raw = None

    def handle_startendtag(self, tag, attrs):
        if tag not in INLINE:
            self.out.append(" ")

    def handle_data(self, data):
        if self.raw is None:
            self.out.append(data)

    def handle_comment(self, data):
        self.out.append(" ")

    handle_decl = handle_pi = unknown_decl = handle_comment


def host_text(page: str) -> str:
    p = _Text()
    p.feed(page)
    p.close()
    s = "".join(p.out)
    for ch in "\t\n\f\r":
        s = s.replace(ch, " ")
    return " ".join(t for t in s.split(" ") if t)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=100_000)
    ap.add_argument("--distinct", type=int, default=512)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    assert a.runs >= 5 and 1 <= a.distinct <= a.pages

    import torch
    from ucfp_amd import _lib, text
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    ctx = _lib.default_context(0)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream or None

    rng = random.Random(29)
    pages = [gen_page(rng) for _ in range(a.distinct)]
    blobs = [p.encode("utf-8") for p in pages]
    order = np.arange(a.pages) % a.distinct
    lens = np.array([len(b) for b in blobs], np.uint64)[order]
    offs = np.zeros(a.pages + 1, np.uint64)
    np.cumsum(lens, out=offs[1:])
    page_bytes = int(offs[-1])
    base = np.frombuffer(b"".join(blobs), np.uint8)
    reps = -(-a.pages // a.distinct)
    d_html = torch.from_numpy(base.copy()).cuda().repeat(reps)[:page_bytes].contiguous()   # page i is blob i % distinct
    d_offs = torch.from_numpy(offs.view(np.int64)).cuda()
    n = a.pages
    d_text = torch.empty(page_bytes + 64, dtype=torch.uint8, device="cuda")
    d_toff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_flags = torch.empty(n, dtype=torch.int32, device="cuda")

    def html():
        _lib.check(lib.ucfp_text_html_batch_dev(ctx.handle, d_html.data_ptr(), d_offs.data_ptr(), n, d_text.data_ptr(), d_toff.data_ptr(),
                                                d_flags.data_ptr(), stream))

    html()
    torch.cuda.synchronize()
    toff = d_toff.cpu().numpy().view(np.uint64)
    text_bytes = int(toff[-1])
    got = d_text[:int(toff[a.distinct])].cpu().numpy().tobytes()
    for i in range(a.distinct):                       # the device's text is html.parser's
        assert got[int(toff[i]):int(toff[i + 1])].decode("utf-8") == host_text(pages[i]), f"page {i} differs from html.parser"
    assert not d_flags.cpu().numpy().any()

    d_tok = torch.empty(int(lib.ucfp_text_canon_bound(text_bytes)) + 64, dtype=torch.uint8, device="cuda")
    d_tokoff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    d_st = torch.empty(n, dtype=torch.int32, device="cuda")
    d_rec = torch.empty((n, text.MINHASH_BYTES), dtype=torch.uint8, device="cuda")

    def canon():
        _lib.check(lib.ucfp_text_canon_batch_dev(ctx.handle, d_text.data_ptr(), d_toff.data_ptr(), n, d_tok.data_ptr(), d_tokoff.data_ptr(),
                                                 d_st.data_ptr(), stream))

    def minhash():
        _lib.check(lib.ucfp_text_minhash_batch_dev(ctx.handle, d_text.data_ptr(), d_toff.data_ptr(), n, text.RAW_ASCII, text.DEFAULT_K,
                                                   d_rec.data_ptr(), d_st.data_ptr(), stream))

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    def row(ms, nbytes):
        med = statistics.median(ms)
        return {"ms_median": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                "gb_per_s_median": round(nbytes / med / 1e6, 2), "gb_per_s_min": round(nbytes / max(ms) / 1e6, 2),
                "gb_per_s_max": round(nbytes / min(ms) / 1e6, 2), "runs_ms": [round(m, 3) for m in ms]}

    res = {"pages": n, "distinct_pages": a.distinct, "page_bytes": page_bytes, "text_bytes": text_bytes,
           "mean_page_bytes": round(page_bytes / n, 1), "mean_text_bytes": round(text_bytes / n, 1), "runs": a.runs,
           "html": row(timed(html), page_bytes), "canon": row(timed(canon), text_bytes), "minhash": row(timed(minhash), text_bytes)}
    assert not d_st.cpu().numpy().any()

    sample = pages[:min(1000, a.distinct)] * (-(-1000 // a.distinct))
    sample = sample[:1000]
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        for p in sample:
            host_text(p)
        host.append(sum(len(p) for p in sample) / (time.perf_counter() - t0) / 1e6)
    res["host_html_parser"] = {"pages": len(sample), "mb_per_s_median": round(statistics.median(host), 2),
                               "mb_per_s_min": round(min(host), 2), "mb_per_s_max": round(max(host), 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
