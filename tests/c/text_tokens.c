/* The token tables of ucfp_text_*_tokens_batch from plain C: the host validation the host entries run before any device
 * work (ucfp_text_tokens_validate), the grapheme set (ucfp_text_grapheme_covered) and the entries' argument checks, none
 * of which needs a device.  Prints one line per check; exit status 0 iff all hold. */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "ucfp_hip.h"

static int failures = 0;

static void expect(const char* what, int got, int want) {
    printf("%s %d\n", what, got);
    if (got != want) {
        fprintf(stderr, "%s: got %d, want %d (%s)\n", what, got, want, ucfp_last_error());
        failures++;
    }
}

int main(void) {
    /* three documents: tokens {"ab", " "}, {}, {"", "\0c"}; the blob is "ab \0c" */
    const uint64_t tok[] = {0, 2, 3, 3, 5}, doc[] = {0, 2, 2, 4};
    expect("valid", ucfp_text_tokens_validate(tok, doc, 3), UCFP_OK);
    expect("empty", ucfp_text_tokens_validate(NULL, NULL, 0), UCFP_OK);
    expect("null", ucfp_text_tokens_validate(NULL, doc, 3), UCFP_E_INVALID);
    uint64_t bad_tok[5], bad_doc[4];
    memcpy(bad_tok, tok, sizeof tok);
    bad_tok[1] = 4; /* 4 > 3: a decreasing pair */
    expect("tok_decreasing", ucfp_text_tokens_validate(bad_tok, doc, 3), UCFP_E_INVALID);
    memcpy(bad_doc, doc, sizeof doc);
    bad_doc[2] = 1;
    expect("doc_decreasing", ucfp_text_tokens_validate(tok, bad_doc, 3), UCFP_E_INVALID);
    /* only the announced slice of the table is the call's business */
    bad_tok[0] = 99;
    bad_tok[1] = 2;
    expect("slice", ucfp_text_tokens_validate(bad_tok, doc + 1, 2), UCFP_OK);
    /* the entries themselves: caller bugs are reported before any device work */
    uint8_t out[UCFP_MINHASH_BYTES];
    int32_t st = 0;
    expect("tokens_null_ctx", ucfp_text_minhash_tokens_batch(NULL, (const uint8_t*)"ab \0c", tok, doc, 3, 5, out, &st), UCFP_E_INVALID);
    expect("ex_null_ctx", ucfp_text_minhash_batch_ex(NULL, (const uint8_t*)"abc", tok, 1, UCFP_TEXT_RAW_ASCII, UCFP_TEXT_TOK_GRAPHEME, 5, out, &st),
           UCFP_E_INVALID);
    expect("covered_a", ucfp_text_grapheme_covered('a'), 1);
    expect("covered_cr", ucfp_text_grapheme_covered(0x0D), 1);
    expect("covered_hangul_syllable", ucfp_text_grapheme_covered(0xAC00), 1);
    expect("covered_jamo_l", ucfp_text_grapheme_covered(0x1100), 0);
    expect("covered_prepend", ucfp_text_grapheme_covered(0x0D4E), 0);
    expect("covered_combining", ucfp_text_grapheme_covered(0x0301), 0);
    return failures ? 1 : 0;
}
