// item_slice.h — work items of the persistent kernels taken apart without a division per item (no HIP dependency: the kernels include it
// through render_device.h, tests/item_slice_check.cpp includes it on the host).
//
// item = chunk * num_slots + slot, slot = tile * 256 + pixel_in_tile, tile = ty * tiles_x + tx (render_device.h: item_to_pixel). A refill
// hands a wave a slice of at most 64 consecutive items. The slice's first item is taken apart once, with the two divisions, on values the
// whole wave shares; item `start + d`, d <= 63, follows by carry:
//   * num_slots is a multiple of 256 and at least 256 > 64, so the slice crosses at most one chunk boundary, and what lies behind the
//     boundary are the first d' < 64 slots of the next chunk: tile 0, pixel d';
//   * otherwise 64 slots cross at most one tile boundary (256 slots per tile): tx + 1, and tx == tiles_x wraps to the next tile row.
#pragma once

#if defined(__HIPCC__)
#define GDPT_ITEM_HD __host__ __device__ inline
#else
#define GDPT_ITEM_HD inline
#endif

namespace gd {

constexpr unsigned kItemSliceMax = 64;      // items per slice at most (one per lane of a wave)

struct ItemParts { unsigned c, pin, tx, ty; };      // chunk, pixel in the 16x16 tile (row-major), tile column, tile row

// The division form: one 32-bit division for the chunk, one for the tile row.
GDPT_ITEM_HD ItemParts item_divide(unsigned item, unsigned num_slots, unsigned tiles_x) {
    ItemParts p;
    p.c = item / num_slots;
    const unsigned pt = item - p.c * num_slots;
    const unsigned tile = pt >> 8;
    p.pin = pt & 255u;
    p.ty = tile / tiles_x; p.tx = tile - p.ty * tiles_x;
    return p;
}

struct ItemSlice { unsigned c0, pt0, tx0, ty0; };   // the slice's first item: chunk, slot in the chunk, tile column, tile row

GDPT_ITEM_HD ItemSlice item_slice_begin(unsigned start, unsigned num_slots, unsigned tiles_x) {
    const ItemParts p = item_divide(start, num_slots, tiles_x);
    ItemSlice s;
    s.c0 = p.c; s.pt0 = start - p.c * num_slots; s.tx0 = p.tx; s.ty0 = p.ty;
    return s;
}

// Item `start + d` of the slice, d < kItemSliceMax. Equal to item_divide(start + d, ...) for num_slots a multiple of 256, >= 256.
GDPT_ITEM_HD ItemParts item_slice_at(const ItemSlice &s, unsigned d, unsigned num_slots, unsigned tiles_x) {
    ItemParts p;
    const unsigned pt = s.pt0 + d;
    p.pin = pt & 255u;                                   // (num_slots is a multiple of 256: the chunk wrap leaves the low bits alone)
    if (pt >= num_slots) { p.c = s.c0 + 1; p.tx = 0; p.ty = 0; return p; }
    p.c = s.c0;
    const bool step = (pt >> 8) != (s.pt0 >> 8);
    p.tx = s.tx0 + (step ? 1u : 0u); p.ty = s.ty0;
    if (p.tx == tiles_x) { p.tx = 0; p.ty = s.ty0 + 1; }
    return p;
}

} // namespace gd
