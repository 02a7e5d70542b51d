// The voxel cell table lr_voxel.hip and lr_overlap.hip share (not part of the ABI): open addressing over the packed cell key, 2..4 slots
// per point.  Every point claims its cell's slot with a 64-bit compare-and-swap; the slot's words (smallest point index, count) are then
// lowered / raised with integer atomics, so nothing depends on the order the threads run in.  What differs between the two users -- the
// rule that turns a coordinate into a cell, and how the arrays are addressed -- stays with them.
#pragma once
#include "lr_prims.h"

#define LR_CELL_EMPTY 0xffffffffffffffffull          // no key: a packed key has its top bit clear
// three cell coordinates, each in 0 .. 2^21 - 1, in one word
__device__ __forceinline__ unsigned long long lr_cells_pack(unsigned long long x, unsigned long long y, unsigned long long z) { return (x << 42) | (y << 21) | z; }
// slots of the table of a cloud of n points: a power of two, at least 1024 and at least 2 n
__host__ __device__ inline size_t lr_cells_capacity(size_t n)
{
    size_t c = 1024;
    while (c < 2 * (n > 0 ? n : 1)) c <<= 1;
    return c;
}
// the slot of `key` in keys[0 .. mask], claimed if nobody has yet.  At most n of the >= 2 n slots are ever taken: an empty one is met.
__device__ __forceinline__ unsigned lr_cells_claim(unsigned long long *__restrict__ keys, unsigned mask, unsigned long long key)
{
    unsigned s = (unsigned)lr_mix64(key) & mask;
    for (;;) {
        const unsigned long long prev = atomicCAS(&keys[s], LR_CELL_EMPTY, key);
        if (prev == LR_CELL_EMPTY || prev == key) break;
        s = (s + 1) & mask;
    }
    return s;
}
// is point i the first (smallest index) of its cell?  first[s] = atomicMin of the indices that claimed slot s; slot = slot_of[i], the slot
// of point i (for the callers that go on to the slot's other words), negative for a dropped point
__device__ __forceinline__ bool lr_cells_is_first(const int32_t *__restrict__ first, const int32_t *__restrict__ slot_of, int i, int &slot)
{
    slot = slot_of[i];
    return slot >= 0 && first[slot] == i;
}
