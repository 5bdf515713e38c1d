// Stand-alone driver of csrc/cider_table.h for tests/test_cider_table_host.py (built with -fsanitize=address,undefined; no GPU, no HIP).
// argv[1]: a text file "n_images n_refs V", then per reference a line "image len id id ...".
// Prints  "N <n> <distinct> <slots>",  "K <n> <idf bits, hex> <id> ..." per distinct n-gram,  "R <ref> <n> <norm bits, hex> <entries> <len>".
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "cider_table.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *fh = fopen(argv[1], "r");
    if (!fh) return 2;
    int n_images = 0, n_refs = 0, V = 0;
    if (fscanf(fh, "%d %d %d", &n_images, &n_refs, &V) != 3) return 2;
    std::vector<int32_t> ref_image, toks;
    std::vector<int64_t> off(1, 0);
    for (int r = 0; r < n_refs; ++r) {
        int img = 0, len = 0;
        if (fscanf(fh, "%d %d", &img, &len) != 2) return 2;
        ref_image.push_back(img);
        for (int k = 0; k < len; ++k) {
            int t = 0;
            if (fscanf(fh, "%d", &t) != 1) return 2;
            toks.push_back(t);
        }
        off.push_back((int64_t)toks.size());
    }
    fclose(fh);
    toks.push_back(0);   // (a non-null data() for a corpus of empty references)
    lrcn_cider_host::Tables t;
    const std::string msg = lrcn_cider_host::build_tables(n_images, n_refs, ref_image.data(), off.data(), toks.data(), V, t);
    if (!msg.empty()) {
        fprintf(stderr, "%s\n", msg.c_str());
        return 1;
    }
    for (int n = 1; n <= 4; ++n) {
        const int q = n - 1;
        printf("N %d %" PRId64 " %u\n", n, t.ngrams[q], t.slots[q]);
        for (uint32_t s = 0; s < t.slots[q]; ++s) {
            if (t.keys[q][(size_t)s * n] < 0) continue;
            uint64_t bits;
            memcpy(&bits, &t.idf[q][s], 8);
            printf("K %d %016" PRIx64, n, bits);
            for (int k = 0; k < n; ++k) printf(" %d", t.keys[q][(size_t)s * n + k]);
            printf("\n");
        }
        for (int r = 0; r < n_refs; ++r) {
            uint64_t bits;
            memcpy(&bits, &t.rnorm[q][r], 8);
            printf("R %d %d %016" PRIx64 " %d %d\n", r, n, bits, t.ent_off[q][r + 1] - t.ent_off[q][r], t.ref_len[r]);
        }
    }
    return 0;
}
