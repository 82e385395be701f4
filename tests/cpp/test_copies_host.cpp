// Host test of the per-key code of the permutation mapping from copies (halo2-pse_amd/csrc/copies_elem.h): the cell numbering, the 64-bit
// sort key (label << 32) | cell, its order and the successor rule, at cell ids 0, 2^31 - 1, 2^31 and 2^32 - 1 -- ids whose mapping tables
// no GPU test can afford.  No GPU and no library.  Also a whole small mapping built from these pieces with std::sort, against a
// hand-written answer.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../halo2-pse_amd/csrc/copies_elem.h"

using namespace h2;

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                \
        }                                                              \
    } while (0)

int main() {
    const uint32_t ids[4] = {0u, 0x7fffffffu, 0x80000000u, 0xffffffffu};
    // pack / unpack, every (label, cell) pair of the four ids
    for (uint32_t label : ids)
        for (uint32_t cell : ids) {
            const uint64_t key = cp_key(label, cell);
            CHECK(cp_key_label(key) == label && cp_key_cell(key) == cell);
            CHECK(key == (((uint64_t)label << 32) | cell));
        }
    // order: by label first, then by cell, both unsigned -- 2^31 above 2^31 - 1, 2^32 - 1 above all
    std::vector<uint64_t> want;
    for (uint32_t label : ids)
        for (uint32_t cell : ids) want.push_back(cp_key(label, cell));
    for (size_t a = 0; a < want.size(); a++)
        for (size_t b = 0; b < want.size(); b++) CHECK(cp_key_lt(want[a], want[b]) == (a < b));
    std::vector<uint64_t> got(want.rbegin(), want.rend());
    std::sort(got.begin(), got.end(), [](uint64_t a, uint64_t b) { return cp_key_lt(a, b); });
    CHECK(got == want);
    CHECK(cp_key(0xffffffffu, 0xffffffffu) == CP_PAD_KEY);
    for (uint64_t key : want) CHECK(key == CP_PAD_KEY || cp_key_lt(key, CP_PAD_KEY));

    // cell ids: k = 28 with 16 columns reaches 2^32 - 1; k = 0 is one row per column
    CHECK(cp_cell(0, 0, 28) == 0u && cp_cell(7, 0x0fffffffu, 28) == 0x7fffffffu && cp_cell(8, 0, 28) == 0x80000000u);
    CHECK(cp_cell(15, 0x0fffffffu, 28) == 0xffffffffu && cp_cell(65534, 0, 0) == 65534u);
    for (uint32_t id : ids) {
        CHECK(cp_cell(cp_cell_column(id, 28), cp_cell_row(id, 28), 28) == id);
        CHECK(cp_cell(cp_cell_column(id, 16), cp_cell_row(id, 16), 16) == id);
        CHECK(cp_cell_column(id, 0) == id && cp_cell_row(id, 0) == 0u);
    }
    CHECK(cp_cell_column(0x80000000u, 28) == 8u && cp_cell_row(0x80000000u, 28) == 0u && cp_cell_column(0xffffffffu, 16) == 65535u);

    // successor: the next key's cell under the same label, else back to the label; the list's end is CP_PAD_KEY
    CHECK(cp_successor(cp_key(0, 0), cp_key(0, 0x7fffffffu)) == 0x7fffffffu);
    CHECK(cp_successor(cp_key(0, 0x7fffffffu), cp_key(0, 0x80000000u)) == 0x80000000u);
    CHECK(cp_successor(cp_key(0, 0x80000000u), cp_key(0, 0xffffffffu)) == 0xffffffffu);
    CHECK(cp_successor(cp_key(0, 0xffffffffu), CP_PAD_KEY) == 0u);
    CHECK(cp_successor(cp_key(0, 0xffffffffu), cp_key(5, 5)) == 0u);
    CHECK(cp_successor(cp_key(0x7fffffffu, 0x80000000u), cp_key(0x80000000u, 0x80000000u)) == 0x7fffffffu);
    CHECK(cp_successor(cp_key(0x80000000u, 0xfffffffeu), CP_PAD_KEY) == 0x80000000u);

    // a whole mapping from these pieces: k = 28, 16 columns, the components {0, 2^31 - 1, 2^31, 2^32 - 1} and {5, 2^31 + 5}, each key twice
    std::vector<uint64_t> keys;
    for (uint32_t cell : ids) keys.push_back(cp_key(0, cell)), keys.push_back(cp_key(0, cell));
    keys.push_back(cp_key(5, 0x80000005u));
    keys.push_back(cp_key(5, 5));
    keys.push_back(CP_PAD_KEY);
    std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b) { return cp_key_lt(a, b); });
    std::vector<std::pair<uint32_t, uint32_t>> edges;
    for (size_t i = 0; i < keys.size(); i++) {
        const uint64_t next = i + 1 < keys.size() ? keys[i + 1] : CP_PAD_KEY;
        if (keys[i] == CP_PAD_KEY || next == keys[i]) continue;
        edges.push_back({cp_key_cell(keys[i]), cp_successor(keys[i], next)});
    }
    const std::vector<std::pair<uint32_t, uint32_t>> want_edges = {{0u, 0x7fffffffu}, {0x7fffffffu, 0x80000000u}, {0x80000000u, 0xffffffffu},
                                                                  {0xffffffffu, 0u},          {5u, 0x80000005u},         {0x80000005u, 5u}};
    CHECK(edges == want_edges);

    if (failures) {
        std::fprintf(stderr, "test_copies_host: %d checks failed\n", failures);
        return 1;
    }
    std::printf("test_copies_host: ok\n");
    return 0;
}
