/* The IDF block of ucfp_hip.h from plain C: the host-only entries (the Q16 log2, the fitted weight, the token key) and
 * the argument checks of the table and SimHash entries, none of which needs a device.  Prints one line per check; exit
 * status 0 iff all hold. */
#include <stdint.h>
#include <stdio.h>

#include "ucfp_hip.h"

static int failures = 0;

static void expect(const char* what, long long got, long long want) {
    printf("%s %lld\n", what, got);
    if (got != want) {
        fprintf(stderr, "%s: got %lld, want %lld (%s)\n", what, got, want, ucfp_last_error());
        failures++;
    }
}

int main(void) {
    expect("log2_1", ucfp_idf_log2_q16(1), 0);
    expect("log2_2", ucfp_idf_log2_q16(2), 1 << 16);
    expect("log2_3", ucfp_idf_log2_q16(3), 103872); /* 65536 log2(3) = 103872.3 */
    expect("log2_max", ucfp_idf_log2_q16(UINT64_MAX), (64 << 16) - 1);
    expect("weight_all", ucfp_idf_weight_q16(10, 10), 0x10000);
    expect("weight_empty", ucfp_idf_weight_q16(0, 0), 0x10000);
    expect("weight_unseen", ucfp_idf_weight_q16(1, 0), 0x20000);
    expect("key_empty", ucfp_text_token_key(NULL, 0) == 0x2D06800538D394C2ull, 1);
    expect("key_differs", ucfp_text_token_key((const uint8_t*)"a", 1) != ucfp_text_token_key((const uint8_t*)"b", 1), 1);
    ucfp_idf_table* t = NULL;
    const uint64_t offs[2] = {0, 3}, key = 5;
    const uint32_t w = 0x10000;
    uint8_t out[UCFP_SIMHASH_BYTES];
    int32_t st = 0;
    size_t n = 0;
    expect("create_null_ctx", ucfp_idf_table_create(NULL, 16, 0, 0, &t), UCFP_E_INVALID);
    expect("add_null_table", ucfp_idf_table_add_batch(NULL, (const uint8_t*)"abc", offs, 1, UCFP_TEXT_RAW_ASCII, UCFP_TEXT_TOK_WORD, &st),
           UCFP_E_INVALID);
    expect("add_tokens_null_table", ucfp_idf_table_add_tokens_batch(NULL, (const uint8_t*)"abc", offs, offs, 1, &st), UCFP_E_INVALID);
    expect("set_null_table", ucfp_idf_table_set_weights(NULL, &key, &w, 1, w), UCFP_E_INVALID);
    expect("finalize_null_table", ucfp_idf_table_finalize(NULL, NULL), UCFP_E_INVALID);
    expect("size_null_table", ucfp_idf_table_size(NULL, NULL, &n, NULL), UCFP_E_INVALID);
    expect("export_null_table", ucfp_idf_table_export(NULL, NULL, NULL, NULL, 0, &n, NULL), UCFP_E_INVALID);
    expect("simhash_null_ctx", ucfp_text_simhash_idf_batch(NULL, NULL, (const uint8_t*)"abc", offs, 1, UCFP_TEXT_RAW_ASCII, UCFP_TEXT_TOK_WORD,
                                                           out, &st),
           UCFP_E_INVALID);
    expect("simhash_tokens_null_ctx", ucfp_text_simhash_idf_tokens_batch(NULL, NULL, (const uint8_t*)"abc", offs, offs, 1, out, &st),
           UCFP_E_INVALID);
    ucfp_idf_table_destroy(NULL);
    return failures ? 1 : 0;
}
