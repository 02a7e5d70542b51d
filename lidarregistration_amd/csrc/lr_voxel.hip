// Voxel de-duplication of a raw LiDAR cloud on gfx950 -- the step between the reference's cloud cache and the hot path.
//
// Replaces ME.utils.sparse_quantize(xyz / voxel_size, return_index=True) as the reference's loaders call it
// (Experiments/dataloader/generic_balanced_loader.py:62-63, voxel_size 0.3; MinkowskiEngine 0.5.4, Requirements/
// conda_GC_full.yml:106 -- not vendored: parity unpinned, restated in oracle/oracle.py::sparse_quantize): coordinates are
// floored to integer cells and one point per occupied cell is kept -- the FIRST one in input order -- with the kept indices
// returned in ascending order, so that xyz[sel] keeps the scan order of the cloud.
//
// Structure (HBM-bound integer work, three small launches): every point claims the slot of its packed cell key (3 x 21 bits) in the
// open-addressing table of lr_cells.h and lowers the slot's point index with atomicMin (so the result does not depend on the order the
// threads run in); a point is kept iff it is its cell's minimum; ordered compaction = per-block counts + prefix + scatter.  The table,
// the hash and the compaction steps are the shared ones (lr_cells.h, lr_prims.h); this file owns the cell rule -- the floor of the
// coordinate, biased by 2^20 -- and its three kernels over plain arrays.
#include "lr_internal.h"
#include "lr_cells.h"
#include <math.h>

#define LR_VX_BIAS (1 << 20)          // cells are stored biased: |cell| < 2^20 per axis

__device__ __forceinline__ unsigned long long vx_key(const double *__restrict__ c, int i, bool &ok)
{
    const double fx = floor(c[3 * (size_t)i]), fy = floor(c[3 * (size_t)i + 1]), fz = floor(c[3 * (size_t)i + 2]);
    ok = fabs(fx) < (double)LR_VX_BIAS && fabs(fy) < (double)LR_VX_BIAS && fabs(fz) < (double)LR_VX_BIAS;     // false for NaN / inf too
    const unsigned long long x = (unsigned long long)((long long)fx + LR_VX_BIAS), y = (unsigned long long)((long long)fy + LR_VX_BIAS),
                             z = (unsigned long long)((long long)fz + LR_VX_BIAS);
    return ok ? lr_cells_pack(x, y, z) : 0ull;
}

__global__ void __launch_bounds__(256)
voxel_insert_kernel(const double *__restrict__ coords, int n, unsigned long long *__restrict__ keys, int32_t *__restrict__ first,
                    unsigned cap_mask, int32_t *__restrict__ slot_of)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool ok;
    const unsigned long long k = vx_key(coords, i, ok);
    if (!ok) { slot_of[i] = -1; return; }           // outside the representable grid / non-finite: dropped
    const unsigned s = lr_cells_claim(keys, cap_mask, k);
    atomicMin(&first[s], i);
    slot_of[i] = (int32_t)s;
}

__global__ void __launch_bounds__(256)
voxel_flag_kernel(int n, const int32_t *__restrict__ first, const int32_t *__restrict__ slot_of, uint8_t *__restrict__ keep,
                  int32_t *__restrict__ blk_cnt)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool k = false;
    if (i < n) { int s; k = lr_cells_is_first(first, slot_of, i, s); keep[i] = k ? 1 : 0; }
    lr_block_count(k, blk_cnt);
}

__global__ void __launch_bounds__(256)
voxel_compact_kernel(const double *__restrict__ coords, int n, const uint8_t *__restrict__ keep, const int32_t *__restrict__ blk_cnt,
                     int32_t *__restrict__ sel, int32_t *__restrict__ cells, int32_t *__restrict__ n_sel)
{
    __shared__ int s_w[4], s_p[4];
    const int before = lr_blocks_before(blk_cnt), i = blockIdx.x * 256 + threadIdx.x;
    const bool k = i < n && keep[i] != 0;
    int prefix;
    const int slot = lr_ordered_slot(k, before, s_w, s_p, prefix);
    if (k) {
        sel[slot] = i;
        if (cells) {
#pragma unroll
            for (int a = 0; a < 3; ++a) cells[3 * (size_t)slot + a] = (int32_t)floor(coords[3 * (size_t)i + a]);
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *n_sel = prefix + s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

extern "C" size_t lr_voxel_dedup_scratch_bytes(int n)
{
    const size_t nn = (size_t)(n > 0 ? n : 1), cap = lr_cells_capacity(nn);
    return cap * 8 + cap * 4 + nn * 4 + ((nn + 255) & ~size_t(255)) + (nn / 256 + 2) * 4 + 1024;
}

extern "C" int lr_voxel_dedup(const double *coords, int n, int32_t *sel, int32_t *n_sel, int32_t *cells, void *scratch,
                              size_t scratch_bytes, void *stream)
{
    LR_REQUIRE(n >= 0, LR_EINVAL, "lr_voxel_dedup: negative point count");
    LR_REQUIRE(n_sel && (n == 0 || (coords && sel && scratch)), LR_EINVAL, "lr_voxel_dedup: null pointer");
    LR_REQUIRE(scratch_bytes >= lr_voxel_dedup_scratch_bytes(n), LR_ESIZE, "lr_voxel_dedup: scratch too small (lr_voxel_dedup_scratch_bytes)");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) { LR_HIP(hipMemsetAsync(n_sel, 0, sizeof(int32_t), st)); return LR_OK; }
    LR_TRY_HIP(lr_check_memory_device(scratch, st, "lr_voxel_dedup", nullptr));      // (n == 0 takes no scratch: nothing to check)
    const size_t cap = lr_cells_capacity((size_t)n);
    char *p = reinterpret_cast<char *>(scratch);
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(p); p += cap * 8;
    int32_t *first = reinterpret_cast<int32_t *>(p); p += cap * 4;
    int32_t *slot_of = reinterpret_cast<int32_t *>(p); p += (size_t)n * 4;
    uint8_t *keep = reinterpret_cast<uint8_t *>(p); p += ((size_t)n + 255) & ~size_t(255);
    int32_t *blk_cnt = reinterpret_cast<int32_t *>(p);
    LR_HIP(hipMemsetAsync(keys, 0xff, cap * 8, st));
    LR_HIP(hipMemsetAsync(first, 0x7f, cap * 4, st));
    const int nb = lr_cdiv(n, 256);
    hipLaunchKernelGGL(voxel_insert_kernel, dim3(nb), dim3(256), 0, st, coords, n, keys, first, (unsigned)(cap - 1), slot_of);
    hipLaunchKernelGGL(voxel_flag_kernel, dim3(nb), dim3(256), 0, st, n, (const int32_t *)first, (const int32_t *)slot_of, keep, blk_cnt);
    hipLaunchKernelGGL(voxel_compact_kernel, dim3(nb), dim3(256), 0, st, coords, n, (const uint8_t *)keep, (const int32_t *)blk_cnt, sel, cells, n_sel);
    LR_LAUNCH_CHECK();
    return LR_OK;
}
