// Stand-alone driver of ucfp_amd/csrc/roaring_parse.h for the host sanitizers (tests/test_index_filter_spec.py builds it with
// -fsanitize=address,undefined and pipes the cases in).
//
// stdin:  cases of  u32 len | len bytes | u32 probes | probes x u64 ids        (little endian, until end of input)
// stdout: one line per case:  "<rc> <cardinality> <containers> <0/1 per probe>"   then "ok <cases>"
// Every filter is copied into a heap block of exactly its length, so a read outside [bytes, bytes + len) is an ASan report;
// each case is parsed twice (validate only, then with the directory) and the two must agree.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../ucfp_amd/csrc/roaring_parse.h"

static bool read_exact(void* dst, size_t n) { return n == 0 || fread(dst, 1, n, stdin) == n; }

int main() {
    size_t cases = 0;
    for (;;) {
        uint32_t len = 0, probes = 0;
        if (fread(&len, 1, 4, stdin) != 4) break;
        uint8_t* bytes = (uint8_t*)malloc(len ? len : 1);
        if (!bytes || !read_exact(bytes, len) || !read_exact(&probes, 4)) return 2;
        if (len == 0) {      // a zero-length filter: a pointer with nothing behind it
            free(bytes);
            bytes = (uint8_t*)malloc(1);
        } else {
            uint8_t* exact = (uint8_t*)malloc(len);
            memcpy(exact, bytes, len);
            free(bytes);
            bytes = exact;
        }
        std::vector<uint64_t> ids(probes);
        if (!read_exact(ids.data(), (size_t)probes * 8)) return 2;
        char e1[160] = "", e2[160] = "";
        uint64_t c1 = 0, c2 = 0;
        ucfp::roaring::Parsed p;
        const int r1 = ucfp::roaring::parse(bytes, len, nullptr, &c1, e1, sizeof e1);
        const int r2 = ucfp::roaring::parse(bytes, len, &p, &c2, e2, sizeof e2);
        if (r1 != r2 || c1 != c2 || strcmp(e1, e2) != 0) {
            printf("validate and parse disagree on case %zu\n", cases);
            return 1;
        }
        if (r1 != 0 && !strstr(e1, " at byte ")) {
            printf("case %zu: no byte offset in '%s'\n", cases, e1);
            return 1;
        }
        std::string line = std::to_string(r1) + " " + std::to_string((unsigned long long)c1) + " " + std::to_string(p.keys.size()) + " ";
        if (r1 == 0) {
            for (size_t i = 0; i < p.ents.size(); i++) {      // the image keeps its alignment promise
                const size_t a = p.ents[i].type == ucfp::roaring::kBitmap ? 8 : p.ents[i].type == ucfp::roaring::kRun ? 4 : 2;
                if (p.ents[i].off % a) {
                    printf("case %zu: container %zu misaligned\n", cases, i);
                    return 1;
                }
            }
            for (uint64_t id : ids) line += ucfp::roaring::contains(p, id) ? '1' : '0';
        }
        puts(line.c_str());
        free(bytes);
        cases++;
    }
    printf("ok %zu\n", cases);
    return 0;
}
