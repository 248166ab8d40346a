// Stand-alone check of csrc/item_slice.h (no GPU): for every film shape below, every slice start and every slice length 1..64, the carried
// form item_slice_at equals the division form item_divide for every item of the slice — slices that straddle a chunk, a tile and a tile
// row included. Built with -fsanitize=address,undefined by tests/test_item_slice_host.py.
#include <cstdio>
#include <cstdlib>
#include "../gradient-based-path-tracing_amd/csrc/item_slice.h"

int main() {
    const unsigned tiles_xs[] = {1, 2, 3, 7, 32}, tile_rows[] = {1, 2, 5}, chunk_counts[] = {1, 2, 6, 64};
    unsigned long long compared = 0, chunk_wraps = 0, tile_steps = 0, row_wraps = 0;
    for (unsigned tiles_x : tiles_xs) for (unsigned rows : tile_rows) for (unsigned chunks : chunk_counts) {
        const unsigned num_slots = tiles_x * rows * 256u, num_items = num_slots * chunks;
        for (unsigned start = 0; start < num_items; start++) {
            const gd::ItemSlice s = gd::item_slice_begin(start, num_slots, tiles_x);
            const unsigned max_len = (num_items - start < gd::kItemSliceMax) ? num_items - start : gd::kItemSliceMax;
            // item start + d belongs to every slice of length > d: comparing d = 0 .. max_len - 1 covers every length 1 .. max_len
            for (unsigned d = 0; d < max_len; d++) {
                const gd::ItemParts a = gd::item_slice_at(s, d, num_slots, tiles_x), b = gd::item_divide(start + d, num_slots, tiles_x);
                if (a.c != b.c || a.pin != b.pin || a.tx != b.tx || a.ty != b.ty) {
                    std::printf("MISMATCH tiles_x %u rows %u chunks %u start %u d %u: carried (c %u pin %u tx %u ty %u) divided (c %u pin %u tx %u ty %u)\n",
                                tiles_x, rows, chunks, start, d, a.c, a.pin, a.tx, a.ty, b.c, b.pin, b.tx, b.ty);
                    return 1;
                }
                if (b.c >= chunks || b.tx >= tiles_x || b.ty >= rows) { std::printf("division form out of range\n"); return 1; }
                compared++;
                chunk_wraps += (b.c != s.c0);
                tile_steps += (b.c == s.c0 && (b.tx != s.tx0 || b.ty != s.ty0));
                row_wraps += (b.c == s.c0 && b.ty != s.ty0);
            }
        }
    }
    // the cases the carry exists for must have occurred
    if (!chunk_wraps || !tile_steps || !row_wraps) { std::printf("a carry case never occurred\n"); return 1; }
    std::printf("item_slice_check ok: %llu items compared, %llu behind a chunk wrap, %llu behind a tile step, %llu behind a row wrap\n",
                compared, chunk_wraps, tile_steps, row_wraps);
    return 0;
}
