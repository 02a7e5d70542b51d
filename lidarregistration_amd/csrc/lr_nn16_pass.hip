// Filter pass of the NN path (contract and error bound: lr_nn16.hip): the f16 matrix-core kernel that both directions prune their
// candidates with, and its launch site (lr_nn16_passb).
#include "lr_nn16_dev.h"
#include <type_traits>

// ------------------------------------------------------------------ filter pass: sample phase + candidate walk in one kernel
// Block = 4 waves x 64 query rows = 256 rows of one column strip.  Column tiles (32 columns) are staged once per block through
// LDS in chunks of LR_PB_CH tiles (register-staged, double-buffered, one barrier per chunk) and shared by the four waves.  LDS
// image: one 64-byte row per column, its four 16-byte pieces XOR-swizzled (lr_lds_off) so that the walk's ds_read_b128 are
// bank-conflict-free for the instruction's lane groups.  Both phases use v_mfma_f32_16x16x32_f16: lane (c, kb) = (lane % 16,
// lane / 16) supplies the 8 K values 8 kb.. of row / column c of a 16-block and receives rows 4 kb + 0..3 of column c.
//
// Phase 1 (forward direction; the reverse direction gets its thresholds from the forward result): the block walks every
// `sstride`-th tile of its strip with the operand roles SWAPPED -- the column fragment is the MFMA's first operand, the query
// rows the second, so a LANE holds one query row per 16-row block and its 4 + 4 accumulator registers of a tile are 8 different
// columns.  The accumulator starts at zero and holds dot16; the lane's value of the tile is
//     b = max_j dot16(i, j) - max_j n1[j]/2      (in-lane maximum tree over the 8 values, one subtraction)
// a LOWER bound of the best g = dot16 - n1[j]/2 among those columns, attained up to the spread of the column norms inside the tile
// (zero for unit-norm descriptors such as FCGF's) -- no per-column operand is read.  Three more ops merge b into the running two
// largest values of the lane; they belong to different tiles, hence to different columns, and the four lanes that share a row see
// disjoint columns, so the second largest after merging the four is a valid lower bound of the row's 2nd largest g (u' = -2 g: an
// upper bound of the 2nd smallest u' -- any valid bound keeps the result exact, a looser one only admits more candidates).  Round 2
// ran this phase as a kernel of its own over every 4th tile (16 us per pair, 13 % of the pair); here it shares the staging buffers
// and the row fragments with the walk, samples every 16th tile (~3 us), and the thresholds it yields are only the START of the walk:
//
// Phase 2: f16 MFMA over ALL tiles of the strip, columns on the lanes.  The accumulator is started at y_i = tau_i / 2 instead of 0,
// so the candidate test u' <= tau_i  <=>  dot16 + y_i >= n1[j]/2 needs no per-element arithmetic: the lane's 16 accumulator
// registers of one 16-column block (the wave's 64 rows) are tested at once.  Two forms, two instantiations (SIGN; both are launched,
// the blocks of the one the pair's column norms do not ask for return at their first branch): with all column norms alike the
// smallest column term is folded into the start values and the test is the AND of 16 sign bits -- 7 v_bitop3_b32 + 1 v_and_b32,
// full rate, no per-column operand --, otherwise the largest of the 16 registers against x_j = n1[j]/2 (7 v_max3 + 1 v_max, half
// rate); + 1 v_cmp + 1 scalar branch.  There is ONE set of 32 accumulator registers: a group of 16 is tested (it holds the previous
// tile) and then handed to the four MFMAs that overwrite it with the current tile, so every test reads its registers four MFMAs
// after they were issued (the hardware does not interlock a vector read of an MFMA result; scheduling barriers keep the MFMAs
// behind the test).  The vector ops of one wave run while the matrix pipe works on another's MFMAs.  What bounds the kernel is the
// board's power limit: a stall that is removed comes back as a lower clock, an instruction that is removed from the fast path does
// not.  The column fragments of tile t+1 are read from LDS one step ahead, which moves the chunk barrier one step
// forward.  Hits are parked in a wave-private LDS list whose fill count lives in a scalar register: no atomics and no LDS round trip
// in the loop.
//
// Thresholds tighten while the walk runs (derive(), below): whenever LR_PB_TIGHTEN new entries have gathered in a list, the four
// waves of the block go through their new entries TOGETHER (they exchange what their lists want at the chunk barrier -- a wave
// in a round keeps its siblings waiting there, so the rounds are taken at the same time), 16 entries per instruction group: the
// entries' columns are gathered and the walk's own MFMA repeated on them with the thresholds of now -- same instruction, same
// operands, same bits --, which yields each entry's row mask and, for single-row entries, the filter value g = dot16 - x_j; the two
// largest g of every row (of the walk: distinct columns) are kept in LDS with two float atomics per entry, y_row <- min(y_row,
// E_row - g2 + ...), and the lanes reload their 16 threshold registers.  The number of hits of a row then grows like
// 2 + 2 ln(tiles / sampled tiles) instead of 2 tiles / sampled tiles, which is what lets the sample be small.  Several strips of one
// row block (single-pair calls) pool their thresholds through atomicMin on an order-preserving integer image (yshare).
#define LR_LDS_ROW 64
// byte offset of 16-byte piece p (K 8p..8p+7) of staged column j of a chunk: rows of 64 bytes, the piece index XOR-swizzled with bits
// 1..2 of the column.  ds_read_b128 is served in four fixed groups of 16 lanes ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ...); with
// the walk's lane map (column = lane % 16, piece = lane / 16) every group then reads 16 different 16-byte slots of the 256-byte bank
// row -- conflict-free (unswizzled 64- or 80-byte rows: 2-way).  Both phases read with that lane map.
__device__ __forceinline__ int lr_lds_off(int j, int p) { return j * LR_LDS_ROW + ((p ^ ((j >> 1) & 3)) << 4); }
#define LR_PB_CH 4               // column tiles per staged chunk
#define LR_PB_WLIST 512          // entries per wave (8 bytes each)
#define LR_PB_DGROUPS 3          // groups of 16 entries derive() has in flight at once (registers: 9 per group)
#define LR_PB_TIGHTEN 48         // new entries of a wave that trigger a tightening round
// (The variants measured against this kernel -- no staging / no tests / no tightening, geometric tightening schedule, per-wave rounds,
// the per-tile fold of phase 1 for the sign form, four waves per SIMD, 8-tile chunks -- are not kept as files: tools/pb_variant.sh rebuilds
// them from history (git show <commit>:...lr_nn16.hip, the single file of that time, with that round's -D switches); none of them is compiled
// into the library.  profiles/r05_pb_ablation.txt has their numbers.)

// The filter pass' FIRST kernel parameter, read only at the END of the kernel and through the kernel-argument segment pointer behind an
// opaque asm: as an ordinary parameter the pointer would sit in two scalar registers across the walk, and the kernel is at its scalar
// register limit (round 6: a fifteen-pointer version of this struct -- the fused verification, docs/HISTORY.md -- cost 17 scalar spills).
struct lr_pb_tail {
    unsigned long long *clk;         // { shader cycles, 100 MHz ticks } summed over the blocks of the launch (lr_workspace_clock), or nullptr
};
__device__ __forceinline__ lr_pb_tail lr_pb_tail_args()
{
    auto ka = __builtin_amdgcn_kernarg_segment_ptr();          // (explicit arguments start at offset 0 of the segment)
    asm volatile("" : "+s"(ka) :: "memory");                   // keeps the compiler from hoisting the load to the top of the kernel
    typedef const unsigned long long __attribute__((opencl_constant)) *cw_t;
    static_assert(sizeof(lr_pb_tail) == 8, "read as one 64-bit word");
    lr_pb_tail t;
    const unsigned long long w = *(cw_t)ka;
    __builtin_memcpy(&t, &w, sizeof t);
    return t;
}

// The one development switch of this file: -DLR_PB_PROBE compiles the hit statistics of tools/pb_micro.hip into the filter pass (waves,
// tests, slow-path visits, hits, derive() rounds, 16-entry groups, 10 ns ticks per phase).  Off in the library: LR_PROBE(...) is empty.
#ifdef LR_PB_PROBE
__device__ unsigned long long lr_pb_stat[16];
#define LR_PROBE(...) __VA_ARGS__
#else
#define LR_PROBE(...)
#endif
#define LR_PB_WAVES 3            // waves per SIMD the filter pass is compiled for
template <bool SIGN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(LR_PB_WAVES, LR_PB_WAVES)))
nn16_passb_kernel(lr_pb_tail tail_first /* read at the end only, through lr_pb_tail_args() */, unsigned long long *clk_on,
                  const _Float16 *__restrict__ Hq, int na_host, const int32_t *__restrict__ rowmap, const int32_t *__restrict__ na_dev,
                  const _Float16 *__restrict__ Hc, const float *__restrict__ nC, int nb,
                  int tiles_per_strip, const float *__restrict__ tau, int32_t *__restrict__ cand_cnt, int32_t *__restrict__ cand,
                  const int32_t *__restrict__ colmap, const float *__restrict__ tile_min, const uint32_t *__restrict__ row_bound,
                  const int32_t *__restrict__ rev_offs, const uint32_t *__restrict__ rev_range, float *__restrict__ yfin, int yfin_stride,
                  uint32_t *__restrict__ yshare, int32_t *__restrict__ form_miss, lr_thr_in thr, lr_pb_grid pg, lr_zargs z)
{
    // 1-D XCD-aware grid -> (row block, strip, pair): the blocks one XCD receives are consecutive row blocks of the same
    // (strip, pair), i.e. they stream the same columns through that XCD's L2
    int logical;
    if (!lr_xcd_block(pg.total, logical)) return;
    const int bx = logical % pg.gx, by = (logical / pg.gx) % pg.gy, pair = logical / (pg.gx * pg.gy);
    if (z.descs) {
        const lr_pair_desc d = z.descs[pair];
        na_host = pg.dir ? d.n1 : d.n0; nb = pg.dir ? d.n0 : d.n1;
    }
    lr_z(Hq, z, pair); lr_z(rowmap, z, pair); lr_z(na_dev, z, pair); lr_z(Hc, z, pair); lr_z(nC, z, pair); lr_z(tau, z, pair);
    lr_z(cand_cnt, z, pair); lr_z(cand, z, pair); lr_z(colmap, z, pair); lr_z(tile_min, z, pair); lr_z(row_bound, z, pair); lr_z(rev_offs, z, pair); lr_z(rev_range, z, pair);
    lr_z(thr.nQ, z, pair); lr_z(thr.range_c, z, pair); lr_z(yfin, z, pair); lr_z(yshare, z, pair);
    // rows: either 0..na_host-1, or (reverse direction) the ordered list rowmap[0..*na_dev-1]; tau, cand_cnt and cand
    // are indexed by the position in that list.  Columns: Hc/nC as they lie; with colmap they are a permuted copy and
    // a candidate's column id is colmap[position].
    const int na = na_dev ? *na_dev : na_host;
    if (bx * LR_BLOCK_ROWS >= na) return;
    // The candidate test of the walk, "some accumulator y_i + dot16 >= x_j", takes two forms -- two instantiations of this kernel, both
    // launched, of which the one the pair's column norms do not ask for returns here.  When the norms are (nearly) all the same -- FCGF
    // descriptors are L2-normalised -- the smallest column term xhat = min_j x_j is folded into the accumulators' start values:
    // y_i - xhat + dot16 >= 0 is then NECESSARY for a hit (x_j >= xhat), a sign test: the AND of 8 sign bits, three v_bitop3_b32 + one
    // v_and_b32 at the full vector rate instead of three v_max3_f32 + one v_max_f32 at half rate, and no per-column operand.  It admits
    // a few pairs more (those between xhat and x_j); derive() applies the exact x_j to every hit anyway.  With spread-out norms that
    // slack would flood the hit lists, so SIGN = false compares with x_j itself (xhat = 0).  (A NaN, infinite, overflowing or
    // non-positive norm anywhere in the column cloud: the plain test -- the prep kernel reports such a norm as a minimum of 0, and
    // an infinite maximum fails `max_nc < inf`; with `inf - min <= 1e-4 inf` alone one overflowing column selected the sign form.)
    float max_nc = 0.0f, min_nc = 0.0f;
    if (thr.range_c) { max_nc = thr.range_c[0]; min_nc = thr.range_c[1]; }
    // (the trailing `&& true` is dead text that the compiler does not treat as dead: without it both instantiations come out with a different
    // schedule, and so they do when `trig` below is made const.  Both go when the kernel is next changed and measured on purpose.)
    const bool sign_ok = thr.range_c != nullptr && min_nc > 0.0f && max_nc < LR_INF && max_nc - min_nc <= 1e-4f * max_nc && true;
    if (sign_ok != SIGN) {
        // (launched alone on the strength of the previous call's norms, and this call's ask for the other form: say so -- the exact
        // kernel then re-does every row by the full scan, and the next call launches the right one)
        if (pg.only && form_miss && bx == 0 && by == 0 && threadIdx.x == 0) { lr_z(form_miss, z, pair); *form_miss = 1; }
        return;
    }
    const float xhat = SIGN ? 0.5f * min_nc : 0.0f;
    __shared__ int s_limit[4];
    // (LR_OPT_CLOCK_PROBE: shader cycles and 100 MHz ticks of every block that walks, summed per workspace -> lr_workspace_clock: the
    // clock the power-limited walk really ran at, the one thing that tells a 3 % change of the kernel from a 3 % slower box)
    __shared__ unsigned long long s_clk[2];
    if (clk_on && threadIdx.x == 0) { s_clk[0] = __builtin_amdgcn_s_memtime(); s_clk[1] = __builtin_amdgcn_s_memrealtime(); }
    constexpr int CH = LR_PB_CH;
    constexpr int XOFF = CH * 32 * LR_LDS_ROW;
    constexpr int BUF = XOFF + (SIGN ? 0 : CH * 32 * 4);      // (the sign form stages no per-column operand, in either phase)
    // The two chunk buffers are SEPARATE arrays on purpose: the walk fills one by LDS-direct loads while it reads the other, and the
    // compiler's wait-count pass puts a vmcnt(0) in front of every LDS read that MAY alias a pending LDS-direct load -- with one array
    // that was every fragment read behind the loads, i.e. the prefetch became synchronous (round 5: found in the ISA).
    __shared__ __attribute__((aligned(16))) unsigned char lds_a[BUF];
    __shared__ __attribute__((aligned(16))) unsigned char lds_b[BUF];
    // (with 8-tile chunks the plain form, which also stages x_j, gives up an eighth of its list to stay at three blocks per CU)
    constexpr int WL = (LR_PB_CH >= 8 && !SIGN) ? (LR_PB_WLIST * 7) / 8 : LR_PB_WLIST;
    __shared__ uint2 wlist[4][WL];   // per wave: entries as above (mask empty until derive() has seen the entry)
    // per row of the block: y = tau/2 (what the accumulators start from), the row's error term, the two largest g of the walk
    __shared__ __attribute__((aligned(16))) float s_Y[LR_BLOCK_ROWS];
    __shared__ float s_D[LR_BLOCK_ROWS], s_N1[LR_BLOCK_ROWS], s_N2[LR_BLOCK_ROWS];
    __shared__ unsigned s_att[2];      // [0]: what the four waves' hit lists want (one byte per wave)
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int c16 = lane & 15, kb = lane >> 4;
    const int row0 = bx * LR_BLOCK_ROWS + wave * 64;
    LR_PROBE(int n_visits = 0, n_hits = 0, n_rounds = 0, n_groups = 0, n_tk_derive = 0, n_tk_flush = 0, n_tk_a = 0, n_tk_b = 0;
             const unsigned long long tk_start = __builtin_amdgcn_s_memrealtime(); unsigned long long tk_walk = 0;)
    int ntiles = (nb + 31) >> 5;
    int my_strips = pg.gy;           // strips this row block really uses (the ordered reverse pass: as many as its column prefix is worth)
    if (tile_min) {
        // Ordered reverse pass (lr_nn16_reverse): a column can only win a row if its key (a lower bound of its distance to every row
        // it does not point at) is <= the row's bound.  Rows lie by descending bucket of their bound, columns by ascending bucket of
        // their key (one monotone map, nn16_rev_order_kernel), so the block's FIRST row has its largest bucket b and the columns
        // that can matter to the block are the first offs[b + 1] of the order (the end of bucket b): three
        // dependent loads by one thread instead of 256 bounds + all tile minima reduced by the block -- most of the (row block, strip)
        // blocks of this launch only find out here that they are not needed.
        if (tid == 0) {
            const float lo = __uint_as_float(rev_range[0]), scale = rs_scale(lo, __uint_as_float(rev_range[1]));
            const float sv = __uint_as_float(row_bound[rowmap[bx * LR_BLOCK_ROWS]]);
            const int b = rs_bucket(sv, lo, scale);        // (bucket b of the column order ends where bucket b + 1 starts)
            s_limit[0] = ((b + 1 < LR_RS_BUCKETS ? rev_offs[b + 1] : nb) + 31) >> 5;
        }
        __syncthreads();
        ntiles = min(ntiles, s_limit[0]);
        // as many of the offered strips as the prefix is worth (a full-length row block uses all of them)
        my_strips = min(pg.gy, (ntiles + tiles_per_strip - 1) / tiles_per_strip);
        if (by >= my_strips) return;
        tiles_per_strip = (ntiles + my_strips - 1) / my_strips;
    }
    const int t_begin = by * tiles_per_strip;
    const int t_end = min(ntiles, t_begin + tiles_per_strip);
    const int nchunks = t_end > t_begin ? (t_end - t_begin + CH - 1) / CH : 0;

    // Both phases run on v_mfma_f32_16x16x32_f16 (all 32 K in one instruction; under the board's power limit it sustains ~20 % more
    // flops than 32x32x16, tools/mfma_clock.hip): lane (c, kb) = (lane % 16, lane / 16) supplies K bytes 16 kb.. of row / column c of
    // a 16-block and receives rows 4 kb + 0..3, column c of the 16 x 16 result.  Row fragments of the wave's four 16-row blocks -- the
    // same registers serve as the MFMA's first operand (phase 2: rows x columns) and as its second (phase 1: columns x rows):
    f16x8 a16[4];
#pragma unroll
    for (int rbk = 0; rbk < 4; ++rbk) {
        int row = min(row0 + 16 * rbk + c16, na - 1);
        if (rowmap) row = rowmap[row];
        a16[rbk] = *reinterpret_cast<const f16x8 *>(Hq + (size_t)row * 32 + 8 * kb);
    }

    f32x4 stage[CH / 2];
    float stage_n = 0.0f;        // raw norm of the staged column: NOT touched until store_chunk, so that the compiler's
                                 // s_waitcnt for it lands after the tile loop instead of right behind the prefetch

    // ---------------------------------------------------------------- thresholds of the block's 256 rows -> LDS
    // given (reverse direction), or made here by phase 1: U = need-th smallest sampled u' = -2 * (need-th largest g);
    // tau = U + 2E + sqrt band 2^-21 (n0 + U + E) + rounding slop; y = tau/2; +inf when fewer than `need` tiles were sampled
    {
        const int rw = bx * LR_BLOCK_ROWS + tid;
        // error term of the row for thresholds made from a filter value found during the walk: y = E' - g (+ 2e-6 |g|)
        float Dv = LR_INF;
        if (thr.nQ && rw < na) {
            const float scale = thr.nQ[rowmap ? rowmap[rw] : rw] + max_nc;
            Dv = lr_nn16_err(scale) + 8e-6f * scale;
        }
        s_D[tid] = Dv; s_N1[tid] = -LR_INF; s_N2[tid] = -LR_INF;
        if (tau) s_Y[tid] = rw < na ? 0.5f * tau[rw] : -LR_INF;          // rows past the end never pass the test
        else {
            // ---- phase 1: every sstride-th tile of the strip, rows on the lanes
            // (a batched call's stride is planned for its LARGEST column cloud.  A pair with fewer tiles takes what lr_nn16_plan_fwd's rule
            // gives its own strip, never more than the call's: at the call's stride a strip of a few tiles is sampled once or not at all,
            // fewer than `need` samples are no threshold, every column is a candidate, the segments overflow and the exact stage re-does
            // the wave's rows by the full scan -- 119 552 of the 196 609 rows of a 300-column pair next to a 2^21-column one)
            int sstride = thr.sstride;
            if (z.descs) sstride = min(sstride, max(pg.gy > 1 ? min(ntiles >> 6, 16) : min((t_end - t_begin) >> 5, 32), 1));
            const int nsamp = t_end > t_begin ? (t_end - t_begin + sstride - 1) / sstride : 0;     // tiles this block samples
            const int nsch = (nsamp + CH - 1) / CH;
            constexpr bool P1E = SIGN;      // (see fold() below)
            auto tile_s = [&](int c, int k) { return t_begin + (c * CH + k) * sstride; };
            auto load_s = [&](int c) {
#pragma unroll
                for (int q = 0; q < CH / 2; ++q) {
                    const int p = tid + 256 * q;
                    const int col = tile_s(c, p >> 7) * 32 + ((p >> 2) & 31);
                    stage[q] = *reinterpret_cast<const f32x4 *>(reinterpret_cast<const unsigned char *>(Hc) + (size_t)min(col, nb - 1) * 64 + (p & 3) * 16);
                }
                const int lc = tid & (CH * 32 - 1);
                const int col = tile_s(c, lc >> 5) * 32 + (lc & 31);
                if constexpr (!P1E) stage_n = nC[min(col, nb - 1)];      // (columns past the end repeat the last one: same tile, same norm)
            };
            auto store_s = [&](int buf) {
#pragma unroll
                for (int q = 0; q < CH / 2; ++q) {
                    const int p = tid + 256 * q;
                    *reinterpret_cast<f32x4 *>(&(buf ? lds_b : lds_a)[lr_lds_off(p >> 2, p & 3)]) = stage[q];
                }
                if constexpr (P1E) return;
                // largest x_j = n1[j]/2 of every tile of the chunk: the threads tid < CH*32 hold one column each, 32 per tile
                float xm = 0.5f * stage_n;
#pragma unroll
                for (int k = 16; k >= 1; k >>= 1) xm = fmaxf(xm, __shfl_xor(xm, k));
                if (tid < CH * 32 && (tid & 31) == 0) *reinterpret_cast<float *>(&(buf ? lds_b : lds_a)[XOFF + (tid >> 5) * 4]) = xm;
            };
            float m1[4], m2[4];           // running two largest (lane, tile) maxima of the lane's four rows (one per 16-row block)
#pragma unroll
            for (int rbk = 0; rbk < 4; ++rbk) { m1[rbk] = -LR_INF; m2[rbk] = -LR_INF; }
            // The phase is software-pipelined like the walk: two accumulator sets, the MFMAs of tile k are issued into one while tile k - 1
            // is folded out of the other (the fold is inline asm -- no canonicalising v_max x, x, x -- and reads its registers at least
            // eight MFMAs after they were issued: the hardware does not interlock a vector read of an MFMA result and the compiler does
            // not see inside the asm, so scheduling barriers pin the order); the LDS fragments of tile k + 1 are requested before the
            // MFMAs of tile k.  Unpipelined (round 3) the phase took 1.75x the walk's time per tile: 9 % of a block's lifetime.
            // P1E (all column norms alike): the lane keeps ELEMENTWISE running maxima of its accumulators instead -- register
            // g of row block rbk collects columns 4 kb + g and 16 + 4 kb + g of every sampled tile, one v_max3 per register and tile (16
            // per tile instead of 32 half-rate ops); the 4 registers x 4 lanes of a row are 16 disjoint column classes, so the two largest
            // class maxima belong to different columns, and g >= dot16 - max_nc / 2 bounds the filter value from below
            f32x4 runm[4];
#pragma unroll
            for (int rbk = 0; rbk < 4; ++rbk) runm[rbk] = f32x4{ -LR_INF, -LR_INF, -LR_INF, -LR_INF };
            auto fold = [&](const f32x4 &lo4, const f32x4 &hi4, int rbk, float xmax) {
                if constexpr (P1E) {
                    asm("v_max3_f32 %0, %0, %4, %8\n\tv_max3_f32 %1, %1, %5, %9\n\tv_max3_f32 %2, %2, %6, %10\n\tv_max3_f32 %3, %3, %7, %11"
                        : "+v"(runm[rbk][0]), "+v"(runm[rbk][1]), "+v"(runm[rbk][2]), "+v"(runm[rbk][3])
                        : "v"(lo4[0]), "v"(lo4[1]), "v"(lo4[2]), "v"(lo4[3]), "v"(hi4[0]), "v"(hi4[1]), "v"(hi4[2]), "v"(hi4[3]));
                    return;
                }
                float t, lo;
                asm("v_max3_f32 %0, %2, %3, %4\n\tv_max3_f32 %0, %0, %5, %6\n\tv_max3_f32 %0, %0, %7, %8\n\tv_max_f32 %0, %0, %9\n\t"
                    "v_sub_f32 %0, %0, %10\n\tv_min_f32 %1, %11, %0"
                    : "=&v"(t), "=&v"(lo)
                    : "v"(lo4[0]), "v"(lo4[1]), "v"(lo4[2]), "v"(lo4[3]), "v"(hi4[0]), "v"(hi4[1]), "v"(hi4[2]), "v"(hi4[3]), "v"(xmax), "v"(m1[rbk]));
                asm("v_max_f32 %0, %0, %1" : "+v"(m1[rbk]) : "v"(t));
                asm("v_max_f32 %0, %0, %1" : "+v"(m2[rbk]) : "v"(lo));
            };
            const f32x4 zero4 = { 0, 0, 0, 0 };
            const int frag16s = lr_lds_off(c16, kb);
            f32x4 sA[8], sB[8];           // [rbk]: columns 0..15 of the tile, [4 + rbk]: columns 16..31
            bool pend = false;            // the set that was filled last awaits its fold (false: its tile does not count)
            float pend_x = 0.0f;
            if (nsch > 0) {
                load_s(0); store_s(0);
                __syncthreads();
                for (int c = 0; c < nsch; ++c) {
                    const int buf = c & 1;
                    if (c + 1 < nsch) load_s(c + 1);
                    // fragments of tile k: lane (c, kb) reads piece kb of columns c and 16 + c; in the result the lane holds query row c
                    // of a row block and registers g <-> columns 4 kb + g of the column block
                    const unsigned char *lbuf = buf ? lds_b : lds_a;
                    const unsigned char *bp = &lbuf[frag16s];
                    f16x8 b0 = *reinterpret_cast<const f16x8 *>(bp), b1 = *reinterpret_cast<const f16x8 *>(bp + 16 * LR_LDS_ROW);
                    float xmax = *reinterpret_cast<const float *>(&lbuf[XOFF]);
#pragma unroll
                    for (int k = 0; k < CH; ++k) {
                        f16x8 n0 = b0, n1 = b1; float nx = xmax;
                        if (k + 1 < CH) {
                            n0 = *reinterpret_cast<const f16x8 *>(bp + (k + 1) * 32 * LR_LDS_ROW);
                            n1 = *reinterpret_cast<const f16x8 *>(bp + (k + 1) * 32 * LR_LDS_ROW + 16 * LR_LDS_ROW);
                            nx = *reinterpret_cast<const float *>(&lbuf[XOFF + (k + 1) * 4]);
                        }
                        f32x4 (&cur)[8] = (k & 1) ? sB : sA;
                        const f32x4 (&prev)[8] = (k & 1) ? sA : sB;
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int rbk = 0; rbk < 4; ++rbk) {
                            cur[rbk] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b0, a16[rbk], zero4, 0, 0, 0);
                            cur[4 + rbk] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b1, a16[rbk], zero4, 0, 0, 0);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        if (pend) {
#pragma unroll
                            for (int rbk = 0; rbk < 4; ++rbk) fold(prev[rbk], prev[4 + rbk], rbk, pend_x);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                        // Tiles past the end of the strip (the last chunk may reach beyond it) are not counted -- and neither is a
                        // PARTIAL last tile: its staged image repeats the cloud's last column in the padding, so a row whose best
                        // column is that one would get the same column as its best and its second best from two of the four lanes
                        // that share the row (the merge below relies on the lanes seeing disjoint columns) -- a threshold one
                        // neighbour too tight (found by tools/soak_fr.py, round 3; the walk of phase 2 still visits that tile).
                        pend = tile_s(c, k) < t_end && (tile_s(c, k) + 1) * 32 <= nb;
                        pend_x = xmax;
                        b0 = n0; b1 = n1; xmax = nx;
                    }
                    if (c + 1 < nsch) store_s(buf ^ 1);
                    __syncthreads();
                }
                if (pend) {      // the last tile sits in set B (CH is even); an explicit wait covers the MFMA write latency
                    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
                    for (int rbk = 0; rbk < 4; ++rbk) fold(sB[rbk], sB[4 + rbk], rbk, pend_x);
                }
            }
            if constexpr (P1E) {
                // the two largest of the lane's four class maxima per row block; x_j <= max_nc / 2 for every column
                const float xg = 0.5f * max_nc;
#pragma unroll
                for (int rbk = 0; rbk < 4; ++rbk) {
                    const float a = fmaxf(runm[rbk][0], runm[rbk][1]), b = fminf(runm[rbk][0], runm[rbk][1]);
                    const float c = fmaxf(runm[rbk][2], runm[rbk][3]), d = fminf(runm[rbk][2], runm[rbk][3]);
                    m1[rbk] = fmaxf(a, c) - xg;
                    m2[rbk] = fmaxf(fminf(a, c), fmaxf(b, d)) - xg;
                }
            }
            // the four lanes of a row (kb = 0..3: disjoint columns) merge their pairs in two exchange rounds; lane kb = 0 writes the row's
            // start value
#pragma unroll
            for (int rbk = 0; rbk < 4; ++rbk) {
#pragma unroll
                for (int o = 16; o <= 32; o <<= 1) {
                    const float c1 = __shfl_xor(m1[rbk], o), c2 = __shfl_xor(m2[rbk], o);
                    const float hi = fmaxf(m1[rbk], c1), lo = fminf(m1[rbk], c1);
                    m2[rbk] = fmaxf(lo, fmaxf(m2[rbk], c2));
                    m1[rbk] = hi;
                }
                const int rl = wave * 64 + 16 * rbk + c16, row = bx * LR_BLOCK_ROWS + rl;
                if (kb == 0) {
                    float yv = -LR_INF;
                    if (row < na) {
                        const float U = -2.0f * (thr.need >= 2 ? m2[rbk] : m1[rbk]);
                        const float scale = thr.nQ[rowmap ? rowmap[row] : row] + max_nc;
                        const float E = lr_nn16_err(scale);
                        yv = 0.5f * (U + 2.0f * E + 6e-6f * scale + 2e-6f * fabsf(U));
                    }
                    s_Y[rl] = yv;
                }
            }
        }
        __syncthreads();
    }
    // Several column strips per row block (single-pair and small-batch calls): the strips' blocks run at the same time and each finds
    // thresholds for the same rows from its own columns.  A threshold is a property of the ROW -- any valid upper bound of its need-th
    // smallest u' holds for every column -- so the strips pool them: one atomicMin per row on an order-preserving integer image of y
    // (yshare, set to +inf by the prep kernel), here after the sample phase and then once per tightening round.  The returned value
    // is what the other strips had found by then.  (A rendezvous of the strips after the sample phase -- a bounded spin on an arrival
    // counter -- was measured and dropped: the strips of a row block are dispatched too far apart, 127 against 110 us for one pair.)
    const bool pooled = yshare != nullptr && thr.nQ != nullptr && my_strips > 1;
    if (pooled) {
        const int rw = bx * LR_BLOCK_ROWS + tid;
        if (rw < na) {
            const float yv = s_Y[tid];
            if (yv == yv) { const float other = lr_ord_dec(atomicMin(&yshare[rw], lr_ord_enc(yv))); if (other < yv) s_Y[tid] = other; }
        }
        __syncthreads();
    }

    // the lane's 4 x 4 threshold registers: register g of row block rbk <-> row 16 rbk + 4 kb + g of the wave
    f32x4 y4[4];
    auto load_y = [&]() {
#pragma unroll
        for (int rbk = 0; rbk < 4; ++rbk) y4[rbk] = *reinterpret_cast<const f32x4 *>(&s_Y[wave * 64 + 16 * rbk + 4 * kb]);
#pragma unroll
        for (int rbk = 0; rbk < 4; ++rbk) y4[rbk] -= xhat;          // (xhat = 0 unless SIGN: x - 0 is x)
    };
    load_y();
    LR_PROBE(tk_walk = __builtin_amdgcn_s_memrealtime();)
    // Staging of the walk: buffer loads STRAIGHT INTO LDS (buffer_load_dwordx4 ... lds: no staging registers, no ds_write; the chunk's
    // position is a scalar offset; rows past the end of the cloud read as zeros through the range check of the buffer descriptor, and
    // whatever such a column -- or a column past the end of the strip -- makes of the test is masked by derive() and flush()).
    // A wave instruction of 64 lanes x 16 bytes fills 1 KB of LDS from M0 onwards in lane order = 16 columns; the XOR swizzle of the
    // LDS image is folded into the lane's GLOBAL address: lane L fetches piece (L & 3) ^ ((L >> 3) & 3) of column L >> 2 of its group.
    // Wave w owns the groups w NQ .. w NQ + NQ - 1 of a chunk; consecutive groups are 1 KB apart in both address spaces (the
    // instruction's offset field applies to both).  The loads of chunk c + 2 are issued right behind the barrier of chunk c (every read
    // of the buffer they go to was complete before that barrier) and awaited -- vmcnt(0) -- before the barrier of chunk c + 1.
    static_assert(CH % 4 == 0, "the staging maps 4 waves onto groups of 16 columns");
    constexpr int NQ = CH * 2 / 4;          // 1 KB groups per wave and chunk
    const __amdgpu_buffer_rsrc_t rsrcH = __builtin_amdgcn_make_buffer_rsrc(const_cast<_Float16 *>(Hc), 0, nb * 64, 0x27000);
    const __amdgpu_buffer_rsrc_t rsrcN = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(nC), 0, nb * 4, 0x27000);
    const int ld_voff = wave * NQ * 1024 + (lane >> 2) * 64 + (((lane & 3) ^ ((lane >> 3) & 3)) << 4);
    const int st_noff = (tid & (CH * 32 - 1)) * 4;
    auto load_chunk = [&](auto bufc, int c) {
        constexpr int buf = decltype(bufc)::value;
        const int col0 = (t_begin + c * CH) * 32;       // wave-uniform
        __attribute__((address_space(3))) void *dst = (__attribute__((address_space(3))) void *)((buf ? lds_b : lds_a) + wave * NQ * 1024);
        static_assert(NQ == 2 || NQ == 4, "chunks of 4 or 8 tiles");      // (the offset field must be a literal)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcH, dst, 16, ld_voff, col0 * 64, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcH, dst, 16, ld_voff, col0 * 64, 1024, 0);
        if constexpr (NQ == 4) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcH, dst, 16, ld_voff, col0 * 64, 2048, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcH, dst, 16, ld_voff, col0 * 64, 3072, 0);
        }
        if constexpr (!SIGN) stage_n = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrcN, st_noff, col0 * 4, 0));
    };
    // the chunk's loads have landed (caller: vmcnt(0)); what is left is the plain form's x_j = n1[j]/2 (+inf masks columns past the end
    // of the cloud or of the strip)
    auto finish_chunk = [&](auto bufc, int c) {
        constexpr int buf = decltype(bufc)::value;
        if constexpr (!SIGN) {
            const int col = (t_begin + c * CH) * 32 + (tid & (CH * 32 - 1));
            const bool ok = col < nb && (col >> 5) < t_end;
            if (tid < CH * 32) *reinterpret_cast<float *>(&(buf ? lds_b : lds_a)[XOFF + tid * 4]) = ok ? 0.5f * stage_n : LR_INF;
        }
    };
    typedef std::integral_constant<int, 0> c0_t;
    typedef std::integral_constant<int, 1> c1_t;
    // per-lane byte offsets of the fragment / x_j of tile 0 of the current and the other buffer; tile k adds a constant.  The lane
    // reads piece kb of columns c and 16 + c of the tile, and their x_j
    const int frag16 = lr_lds_off(c16, kb), x_lane = XOFF + c16 * 4;
    auto read_b = [&](auto bufc, int k, f16x8 &b0, f16x8 &b1, f32x2 &xj) {
        constexpr int buf = decltype(bufc)::value;
        const unsigned char *lbuf = buf ? lds_b : lds_a;          // (buf is a compile-time value)
        b0 = *reinterpret_cast<const f16x8 *>(&lbuf[frag16 + k * 32 * LR_LDS_ROW]);
        b1 = *reinterpret_cast<const f16x8 *>(&lbuf[frag16 + k * 32 * LR_LDS_ROW + 16 * LR_LDS_ROW]);
        if constexpr (!SIGN) {      // (the sign form of the test reads no per-column operand)
            xj.x = *reinterpret_cast<const float *>(&lbuf[x_lane + k * 32 * 4]);
            xj.y = *reinterpret_cast<const float *>(&lbuf[x_lane + k * 32 * 4 + 64]);
        }
    };
    int wcnt = 0;            // entries in this wave's list (wave-uniform: lives in a scalar register)
    const unsigned lanecode = (unsigned)c16 | ((unsigned)kb << 22);      // the lane's part of an entry: column within the 16-block | lane group
    // The slow paths (derive(), flush(); a hit in the plain form) work out the lane's coordinates afresh: values that only they use would
    // otherwise be kept in registers across the hot loop (or spilled to scratch memory and fetched back on every visit: +4 us per pair)
    auto cold_lane = [&]() { int l; asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l)); return l; };
    int wdone = 0;           // ... of which the tightening has seen this many
    int trig = LR_PB_TIGHTEN;      // new entries that make the wave ask for a tightening round
    // what the wave's list wants (bit 0: a tightening round, bit 1: to be emptied): recomputed where wcnt / wdone change (the slow path of
    // a hit, derive(), flush()) -- not at every chunk -- and posted to the block only when it differs from what was posted last
    int wposted = 0, wnext = 0;      // the wish posted last; the fill count from which the list wants something
    // The wave owns one segment of the candidate store: seg[(row block, wave, strip)][seg_cap] entries { column, code | mask }
    // exactly as they lie in its LDS list.  Emptying the list is a compacting copy with plain stores -- no atomics, nothing
    // to wait for; nn16_exact_kernel expands the masks and bins the entries by row.  seg_fill < 0: the segment overflowed
    // (duplicate-heavy input), the wave's 64 rows go through the exact full-row scan.
    // (the LR_NN16_SEG entries of the wave's rows are divided among the strips the row block really uses)
    const int seg_cap = lr_seg_cap(my_strips);
    uint2 *__restrict__ seg = reinterpret_cast<uint2 *>(cand) + (size_t)(bx * 4 + wave) * LR_NN16_SEG + (size_t)by * seg_cap;
    int seg_fill = 0;
    const bool tightening = thr.nQ != nullptr;
    auto my_wish = [&]() { return (wcnt >= WL / 2 ? 2 : 0) | ((tightening && wcnt - wdone >= trig) ? 1 : 0); };
    auto set_next = [&]() { wnext = tightening ? min(wdone + trig, WL / 2) : WL / 2; };      // (my_wish() != 0 <=> wcnt >= wnext)
    set_next();
    // One round over the new entries [wdone, wcnt) of the wave's list (wave-local).  The slow path of the walk only parks { column,
    // register group } of a hit; WHICH of the group's 8 rows passed, and with what filter value, is worked out here, 16 entries at a
    // time, by the matrix pipe itself: lane (c, kb) fetches K slice kb of the column of entry e0 + c (one 16-byte gather), four
    // v_mfma_f32_16x16x32_f16 with the row fragments and the thresholds of NOW give it y_i + dot16 of that column against rows
    // 16 rbk + 4 kb + 0..3 -- the same instruction on the same operands as the walk, so the same bits -- and the lane whose kb is the
    // entry's compares the group's 8 registers with x_j: 2 vector instructions per entry and register instead of 16 per hit and wave.
    // Thresholds only ever decrease, so a mask taken against the thresholds of now is a subset of the one the walk saw and still a
    // superset of what the final thresholds admit; an entry that no longer passes any row is dropped on the spot.
    // update: (forward direction, and the reverse one when it is given the rows' error terms) the two largest g of every row ->
    // y -> threshold registers.  An entry with a single row keeps its g = dot16 - x_j for the drop tests of flush() and
    // nn16_exact_kernel.
    auto derive = [&](bool update) {
        const int lane = cold_lane(), c16 = lane & 15, kb = lane >> 4;      // (shadow the kernel's)
        const int nlist = min(wcnt, WL);
        __builtin_amdgcn_s_setprio(3);      // the wave's three siblings wait for it at the next chunk barrier (60.1 -> 59.3 us per pair)
        LR_PROBE(++n_rounds; n_groups += (nlist - wdone + 15) >> 4; const unsigned long long tk0 = __builtin_amdgcn_s_memrealtime();)
        constexpr int DG = SIGN ? LR_PB_DGROUPS : (LR_PB_DGROUPS > 2 ? 2 : LR_PB_DGROUPS);      // (the plain form holds the x_j operands too: a third group would spill)
        for (int e0 = wdone; e0 < nlist; e0 += 16 * DG) {
            // a few groups of 16 entries per pass: all their gathers are in flight before the first MFMA (one L2 latency per pass)
            uint2 v[DG]; f16x8 bf[DG]; float xn[DG];
#pragma unroll
            for (int g = 0; g < DG; ++g) {
                v[g] = wlist[wave][min(e0 + 16 * g + c16, WL - 1)];
                const int col = (int)(v[g].x & LR_PB_COLMASK);
                bf[g] = __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrcH, col * 64 + kb * 16, 0, 0));
                xn[g] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrcN, col * 4, 0, 0));
            }
            LR_PROBE({ const unsigned long long ta = __builtin_amdgcn_s_memrealtime(); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); n_tk_a += (int)(__builtin_amdgcn_s_memrealtime() - ta); })
#pragma unroll
            for (int g = 0; g < DG; ++g) {
                if (e0 + 16 * g >= nlist) break;              // (wave-uniform)
                const int e = e0 + 16 * g + c16;
                const bool valid = e < nlist;
                const int col = (int)(v[g].x & LR_PB_COLMASK);
                // padding columns (past the end of the cloud or of the strip) pass the walk's test only when the threshold is +inf
                const float x = (valid && col < nb && (col >> 5) < t_end) ? 0.5f * xn[g] - xhat : LR_INF;      // (xhat = 0 unless SIGN)
                f32x4 d[4];
#pragma unroll
                for (int rbk = 0; rbk < 4; ++rbk) d[rbk] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a16[rbk], bf[g], y4[rbk], 0, 0, 0);
                if (valid && lr_pb_kb(v[g].x) == kb) {
                    // bit 4 rbk + k <-> register k of row block rbk; set unless acc < x (a NaN accumulator -- non-finite f16 operands --
                    // stays a candidate: rows with such operands are re-done by the exact full-row scan, columns only add candidates
                    // the exact stage orders)
                    unsigned mask = 0u;
#pragma unroll
                    for (int rbk = 0; rbk < 4; ++rbk)
#pragma unroll
                        for (int k = 0; k < 4; ++k) mask |= (d[rbk][k] < x) ? 0u : (1u << (4 * rbk + k));
                    uint2 w = make_uint2(v[g].x, mask);              // mask 0: the entry is dropped when the list is emptied
                    if (update && mask != 0u && (mask & (mask - 1u)) == 0u) {
                        const int b = __builtin_ctz(mask);
                        const int rl = wave * 64 + lr_pb_row(kb, b);
                        // (the one register that passed is the largest of the 16)
                        float m = fmaxf(fmaxf(fmaxf(d[0][0], d[0][1]), fmaxf(d[0][2], d[0][3])), fmaxf(fmaxf(d[1][0], d[1][1]), fmaxf(d[1][2], d[1][3])));
                        m = fmaxf(m, fmaxf(fmaxf(fmaxf(d[2][0], d[2][1]), fmaxf(d[2][2], d[2][3])), fmaxf(fmaxf(d[3][0], d[3][1]), fmaxf(d[3][2], d[3][3]))));
                        // the register holds y_row + dot16, so g = dot16 - x_j = (register - x_j) - y_row
                        const float gv = (m - x) - s_Y[rl];
                        const float old = atomicMax(&s_N1[rl], gv);
                        atomicMax(&s_N2[rl], fminf(old, gv));
                        // (kept rounded UP to 16 bits next to the mask: the form the candidate store carries; the drop tests -- flush() now, the
                        // exact kernel against the final threshold -- then only ever keep more than the exact value would)
                        const unsigned gb = __float_as_uint(gv);
                        const unsigned up16 = (gb & 0x80000000u) ? (gb >> 16) : ((gb + 0xffffu) >> 16);      // towards +inf
                        w.y |= up16 << 16;
                        w.x |= LR_PB_HASG;
                    }
                    wlist[wave][e] = w;
                }
            }
        }
        LR_PROBE(const unsigned long long tb = __builtin_amdgcn_s_memrealtime();)
        wdone = nlist;
        set_next();
        if (update) {
            // lane = row: y <- min(y, E' - g_need + 2e-6 |g_need|)   (g_need: the need-th largest g of the walk so far; -inf: no change)
            const int rl = wave * 64 + lane;
            const float gn = thr.need >= 2 ? s_N2[rl] : s_N1[rl];
            const float yn = (s_D[rl] - gn) + 2e-6f * fabsf(gn);
            float yv = s_Y[rl];
            if (yn < yv) yv = yn;                           // (NaN compares false: the row keeps its threshold)
            // (the exchange as a plain load at the start of the round + an atomic nobody waits for: no change, 96.4 us either way -- round 5)
            if (pooled && row0 + lane < na && yv == yv) {   // pool with the row block's other strips
                const float other = lr_ord_dec(atomicMin(&yshare[row0 + lane], lr_ord_enc(yv)));
                if (other < yv) yv = other;
            }
            s_Y[rl] = yv;
            load_y();
        }
        LR_PROBE(asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); n_tk_b += (int)(__builtin_amdgcn_s_memrealtime() - tb); n_tk_derive += (int)(__builtin_amdgcn_s_memrealtime() - tk0);)
        __builtin_amdgcn_s_setprio(0);
    };
    auto flush = [&]() {
        if (wdone < wcnt) derive(tightening);
        const int lane = cold_lane();
        LR_PROBE(const unsigned long long tkf = __builtin_amdgcn_s_memrealtime();)
        if (wcnt > WL) seg_fill = -1;       // more hits between two chunk boundaries than the list holds
        else if (seg_fill >= 0) {
            for (int e0 = 0; e0 < wcnt; e0 += 64) {
                const int e = e0 + lane;
                uint2 v = make_uint2(0u, 0u);
                if (e < wcnt) v = wlist[wave][e];
                const int col = (int)(v.x & LR_PB_COLMASK);
                // padding columns pass the test only when tau is +inf
                bool keep = e < wcnt && (v.y & 0xffffu) != 0u && col < nb && (col >> 5) < t_end;
                if (v.x & LR_PB_HASG) {
                    // g of the entry against the row's threshold of NOW (candidate <=> g >= -y): what an earlier, looser threshold let
                    // in is dropped here (g as derive() left it: rounded UP to 16 bits); the exact kernel repeats the test against the final threshold
                    const float gv = __uint_as_float(v.y & 0xffff0000u);
                    const int rl = wave * 64 + lr_pb_row(lr_pb_kb(v.x), __builtin_ctz((v.y & 0xffffu) | 0x8000u));
                    const float yr = s_Y[rl];
                    if (gv + 1e-5f * (fabsf(gv) + fabsf(yr)) < -yr) keep = false;
                }
                const unsigned long long kb = __builtin_amdgcn_ballot_w64(keep);
                const int pos = seg_fill + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(kb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)kb, 0u));
                const int nk = __builtin_popcountll(kb);
                if (seg_fill + nk > seg_cap) { seg_fill = -1; break; }
                if (keep) { if (colmap) v.x = (unsigned)colmap[col] | (v.x & ~LR_PB_COLMASK); seg[pos] = v; }
                seg_fill += nk;
            }
        }
        wcnt = 0; wdone = 0; set_next();
        LR_PROBE(n_tk_flush += (int)(__builtin_amdgcn_s_memrealtime() - tkf);)
    };
    // candidate test of the lane's 16 accumulator registers of column block cb (16 columns x the wave's 64 rows).
    // A hit only parks { column, lane group } -- a handful of vector instructions and one LDS write; everything else about it is worked
    // out later, 16 entries per instruction group (derive()).
    auto check = [&](const f32x4 &r0, const f32x4 &r1, const f32x4 &r2, const f32x4 &r3, float x, int tile, int cb) {
        bool mine_hit;
        if constexpr (SIGN) {
            // two interleaved chains of three-input ANDs over the 16 sign bits (one asm block: no hazard padding between the halves)
            int sa, sb;
            asm("v_bitop3_b32 %0, %2, %3, %4 bitop3:0x80\n\tv_bitop3_b32 %1, %10, %11, %12 bitop3:0x80\n\t"
                "v_bitop3_b32 %0, %0, %5, %6 bitop3:0x80\n\tv_bitop3_b32 %1, %1, %13, %14 bitop3:0x80\n\t"
                "v_bitop3_b32 %0, %0, %7, %8 bitop3:0x80\n\tv_bitop3_b32 %1, %1, %15, %16 bitop3:0x80\n\t"
                "v_bitop3_b32 %0, %0, %1, %9 bitop3:0x80\n\tv_and_b32 %0, %0, %17"
                : "=&v"(sa), "=&v"(sb)
                : "v"(r0[0]), "v"(r0[1]), "v"(r0[2]), "v"(r0[3]), "v"(r1[0]), "v"(r1[1]), "v"(r1[2]), "v"(r1[3]),
                  "v"(r2[0]), "v"(r2[1]), "v"(r2[2]), "v"(r2[3]), "v"(r3[0]), "v"(r3[1]), "v"(r3[2]), "v"(r3[3]));
            mine_hit = sa >= 0;                        // the AND of the sign bits is clear: some register is not negative
        } else {
            float ma, mb;
            asm("v_max3_f32 %0, %2, %3, %4\n\tv_max3_f32 %1, %10, %11, %12\n\t"
                "v_max3_f32 %0, %0, %5, %6\n\tv_max3_f32 %1, %1, %13, %14\n\t"
                "v_max3_f32 %0, %0, %7, %8\n\tv_max3_f32 %1, %1, %15, %16\n\t"
                "v_max3_f32 %0, %0, %1, %9\n\tv_max_f32 %0, %0, %17"
                : "=&v"(ma), "=&v"(mb)
                : "v"(r0[0]), "v"(r0[1]), "v"(r0[2]), "v"(r0[3]), "v"(r1[0]), "v"(r1[1]), "v"(r1[2]), "v"(r1[3]),
                  "v"(r2[0]), "v"(r2[1]), "v"(r2[2]), "v"(r2[3]), "v"(r3[0]), "v"(r3[1]), "v"(r3[2]), "v"(r3[3]));
            mine_hit = ma >= x;
        }
        const unsigned long long hit = __builtin_amdgcn_ballot_w64(mine_hit);
        if (__builtin_expect(hit != 0ull, 0)) {       // rare: keeps the common path a fall-through
            if (mine_hit) {
                const int pos = wcnt + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(hit >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)hit, 0u));
                // (the column is worked out here, not on the fast path: tile is wave-uniform)
                unsigned lc = lanecode;
                if constexpr (!SIGN) { const int ln = cold_lane(); lc = (unsigned)(ln & 15) | ((unsigned)(ln >> 4) << 22); }      // (the plain form has no register to spare for it)
                if (pos < WL) wlist[wave][pos] = make_uint2((unsigned)(tile * 32 + cb * 16) | lc, 0u);
            }
            wcnt += __builtin_popcountll(hit);
            LR_PROBE(++n_visits; n_hits += __builtin_popcountll(hit);)
        }
    };

    f16x8 b0, b1;
    f32x2 xN = { LR_INF, LR_INF }, xC = { LR_INF, LR_INF };
    // ONE set of accumulators (32 registers): a group of 16 -- one 16-column block against the wave's 64 rows -- is tested while it holds
    // the previous tile and then handed to the four MFMAs that overwrite it with the current tile, so every test reads its registers four
    // MFMAs after they were issued and nothing is double-buffered (the 32 registers this saves keep the kernel at LR_PB_WAVES = 3 waves per SIMD)
    f32x4 acc[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[q][cb][g] = -LR_INF;

    // one pipeline step: tests of the previous tile group by group, each followed by the MFMAs of tile (c, k) into the registers just
    // tested; LDS read of the next tile (par = c & 1: the buffer chunk c lies in -- a compile-time value, the loop below is unrolled by
    // two chunks so that no buffer offset is computed, swapped or selected at run time)
    auto step = [&](int c, int k, auto parc) {
        constexpr int par = decltype(parc)::value;
        f16x8 n0, n1; f32x2 nx;
        if (k + 1 < CH) read_b(std::integral_constant<int, par>{}, k + 1, n0, n1, nx);
        else read_b(std::integral_constant<int, par ^ 1>{}, 0, n0, n1, nx);
        const int tileC = t_begin + c * CH + k - 1;
#define MF(rbk, cb, b) acc[rbk][cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a16[rbk], b, y4[rbk], 0, 0, 0)
        // (the scheduling barriers keep the MFMAs behind the test of the registers they overwrite: hoisted above it they would need
        // a second set of accumulators -- and the kernel its row fragments from scratch memory)
        check(acc[0][0], acc[1][0], acc[2][0], acc[3][0], xC.x, tileC, 0);
        __builtin_amdgcn_sched_barrier(0);
        MF(0, 0, b0); MF(1, 0, b0); MF(2, 0, b0); MF(3, 0, b0);
        __builtin_amdgcn_sched_barrier(0);
        check(acc[0][1], acc[1][1], acc[2][1], acc[3][1], xC.y, tileC, 1);
        __builtin_amdgcn_sched_barrier(0);
        MF(0, 1, b1); MF(1, 1, b1); MF(2, 1, b1); MF(3, 1, b1);
        __builtin_amdgcn_sched_barrier(0);
#undef MF
        b0 = n0; b1 = n1; xC = xN; xN = nx;
    };
    auto drain = [&]() {
        const int tileC = t_begin + nchunks * CH - 1;
        check(acc[0][0], acc[1][0], acc[2][0], acc[3][0], xC.x, tileC, 0);
        check(acc[0][1], acc[1][1], acc[2][1], acc[3][1], xC.y, tileC, 1);
    };
    if (nchunks > 0) {
        load_chunk(c0_t{}, 0);
        __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): chunk 0 has landed (and everything older: row fragments, thresholds)
        finish_chunk(c0_t{}, 0);
        if (nchunks > 1) load_chunk(c1_t{}, 1);
        if (tid == 0) s_att[0] = 0u;
        __syncthreads();
        read_b(c0_t{}, 0, b0, b1, xN);
        // The walk is a loop nest: the inner loop is the hot one and contains no tightening code (the compiler then keeps the threshold
        // registers loop-invariant and its wait counts exact); it is left whenever a hit list wants attention.
        // The four waves of a block attend to their lists TOGETHER: a wave in derive() keeps its three siblings waiting
        // at the next chunk barrier, so 4 x ~11 rounds per block, one wave at a time, stall the block four times as often as ~12 rounds
        // that all four take at once.  Every wave keeps what its list wants in one byte of an LDS word (written only when it changes),
        // reads all four wishes behind the chunk barrier and acts at the end of the chunk.  (The decision need not be block-uniform: a wave
        // acts on its own list only, and neither derive() nor flush() contains a barrier.)
        // What a chunk boundary costs is the wave's own instruction stream (round 5, tools/r5_pmc_micro.sh: a wave issues one instruction
        // per ~5 cycles whatever its class, and at three waves per SIMD it has 48 cycles per MFMA): per 32 MFMAs the boundary used to
        // be 34 scalar + 12 vector instructions -- bounds tests, buffer parity, exec save / restore around the one-lane write, materialised
        // booleans.  Now: the two chunks of a buffer pair are separate code (offsets are immediates), the last two chunks of the strip
        // run as a tail with the bounds tests, and a wish is posted only when it changes.
        int c = 0;
        int wish = 0;
        auto chunk = [&](auto parc, auto tailc) {
            constexpr int par = decltype(parc)::value;
            constexpr bool tail = decltype(tailc)::value != 0;
            unsigned wishes = 0u;
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                if (k == CH - 1) {
                    // the last step of a chunk reads the first fragment of the next one: make that chunk visible now.  All
                    // reads of the buffer it goes to were issued before the previous barrier (the step above read this
                    // chunk's own last tile), so one barrier per chunk still orders everything.
                    if (!tail || c + 1 < nchunks) { __builtin_amdgcn_s_waitcnt(0x0F70); finish_chunk(std::integral_constant<int, par ^ 1>{}, c + 1); }      // vmcnt(0): chunk c + 1 has landed
                    // (one scalar comparison per chunk; the wish is worked out and written when the list reaches the mark; a round
                    // follows at the end of this very chunk -- the wave reads its own byte behind the barrier -- and takes it back)
                    if (__builtin_expect(wcnt >= wnext, 0)) {
                        const int wm = my_wish();
                        if (lane == 0) reinterpret_cast<unsigned char *>(&s_att[0])[wave] = (unsigned char)wm;
                        wposted = wm; wnext = 0x7fffffff;
                    }
                    __syncthreads();
                    // (requested here, looked at behind the chunk's last step)
                    wishes = s_att[0];
                    if (!tail || c + 2 < nchunks) load_chunk(std::integral_constant<int, par>{}, c + 2);      // (into the buffer chunk c has just been read out of)
                }
                step(c, k, parc);
            }
            // (the four bytes as they are: which bit is set is looked at outside the loop)
            wish = (int)__builtin_amdgcn_readfirstlane(wishes);
            ++c;
        };
        typedef std::integral_constant<int, 0> body_t;
        typedef std::integral_constant<int, 1> tail_t;
        while (c < nchunks) {
            wish = 0;
            // The hot loop takes two chunks per iteration, buffer 0 then buffer 1, as straight-line code (`body`: chunks c + 1 and c + 2
            // exist, nothing is tested).  An odd chunk on its own -- the walk resumes at one after a round, or it is the strip's last --
            // and the last two chunks of the strip run through the `tail` form with the bounds tests.
            if (c & 1) chunk(c1_t{}, tail_t{});
            else if (c + 3 < nchunks) {
                do { chunk(c0_t{}, body_t{}); if (wish) break; chunk(c1_t{}, body_t{}); } while (!wish && c + 3 < nchunks);
            } else chunk(c0_t{}, tail_t{});
            wish = (wish & 0x02020202) ? 2 : (wish ? 1 : 0);
            if (wish && wposted) { if (lane == 0) reinterpret_cast<unsigned char *>(&s_att[0])[wave] = 0; wposted = 0; }
            if (wish & 2) flush();
            else if (wish) { if (wdone < wcnt) derive(true); }
        }
        // drain: the last tile of the last chunk sits in the accumulators.  The inline-asm tests below read MFMA results the
        // compiler cannot see them read (no automatic wait states): inside the loop every such read is at least two
        // MFMAs behind its producer; here an explicit wait covers the 8-pass MFMA write latency.
        asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
        drain();
        flush();           // (with a last tightening round: the entries get their g, the rows their final thresholds)
    }
    if (lane == 0) {
        int32_t *cw = cand_cnt + (bx * 4 + wave) * (pg.gy + 1);
        cw[by] = seg_fill;                     // entries in this wave's segment (< 0: overflow)
        if (by == 0) cw[pg.gy] = my_strips;    // how the wave's store is divided (read by nn16_exact_kernel)
    }
    LR_PROBE(if (lane == 0) {
        atomicAdd(&lr_pb_stat[0], 1ull); atomicAdd(&lr_pb_stat[1], (unsigned long long)nchunks * CH * 4); atomicAdd(&lr_pb_stat[2], (unsigned long long)n_visits);
        atomicAdd(&lr_pb_stat[3], (unsigned long long)n_hits); atomicAdd(&lr_pb_stat[4], (unsigned long long)n_rounds); atomicAdd(&lr_pb_stat[5], (unsigned long long)n_groups);
        const unsigned long long tk_end = __builtin_amdgcn_s_memrealtime();
        atomicAdd(&lr_pb_stat[6], (unsigned long long)n_tk_derive); atomicAdd(&lr_pb_stat[7], (unsigned long long)n_tk_flush);
        atomicAdd(&lr_pb_stat[8], tk_walk - tk_start); atomicAdd(&lr_pb_stat[9], tk_end - tk_start);
        atomicAdd(&lr_pb_stat[10], (unsigned long long)n_tk_a); atomicAdd(&lr_pb_stat[11], (unsigned long long)n_tk_b);
    })
    // the rows' final thresholds (wave-local: every wave writes its own 64 rows): nn16_exact_kernel drops the entries they exclude
    if (yfin) {
        const int rw = row0 + lane;
        if (rw < na) yfin[(size_t)by * yfin_stride + rw] = tightening ? s_Y[wave * 64 + lane] : LR_INF;
    }
    if (threadIdx.x == 0) {
        const lr_pb_tail tl = lr_pb_tail_args();
        if (tl.clk) {
            atomicAdd(&tl.clk[0], __builtin_amdgcn_s_memtime() - s_clk[0]);
            atomicAdd(&tl.clk[1], __builtin_amdgcn_s_memrealtime() - s_clk[1]);
        }
    }
}

// ------------------------------------------------------------------ host side
// which form of the filter pass a single-pair call launches alone: what the range kernel of an earlier call on this workspace found
// for the column cloud (0: cloud 0 = reverse pass, 1: cloud 1 = forward pass); 0 = unknown (first call, batched call): launch both.
// The hint is only trusted when TWO calls in a row read the same value: a workspace that alternates between unit-norm and other
// clouds (the harness' calibration call next to user calls) would otherwise guess wrong on every call and pay the exact kernel's
// full scan each time, silently -- it launches both forms instead, the cost of an empty launch.  A miss that still
// happens (the first call of a changed workload) is reported in lr_pair_result.reserved[2].
static int lr_nn16_form_hint(const lr_call &c, int col_cloud)
{
    lr_workspace *ws = c.ws;
    if (c.pairs != 1 || !ws->form_host) return 0;
    const int h = *reinterpret_cast<const volatile int32_t *>(&ws->form_host[col_cloud]);
    const int prev = ws->form_prev[col_cloud];
    ws->form_prev[col_cloud] = h;
    return ((h == 1 || h == 2) && h == prev) ? h : 0;
}

// The launch site of the filter pass, bracketed by the direction's stage-timer events.  Both forms of the walk's candidate test; the
// blocks of the one the column norms do not ask for return at once.  A single-pair call launches only the form the column cloud's
// norms asked for in the PREVIOUS call on this workspace (lr_nn16_form_hint: a flag the range kernel leaves in pinned host memory; no
// synchronisation, any value is safe): if this call's norms ask for the other form, the launched kernel flags the miss and the exact
// kernel re-does every row by the full scan -- correct, slow once, and the next call launches the right form.  (An empty launch costs
// 4.7 us: 9.4 of a single pair's 346 us of kernels.)
int lr_nn16_passb(const lr_call &c, const lr_pb_args &a)
{
    lr_workspace *ws = c.ws;
    // 1-D XCD-aware grid over (row block, strip, pair), padded to a multiple of 8
    const int total = a.row_blocks * a.strips * c.pairs;
    const dim3 grid(8 * lr_cdiv(total, 8));
    LR_TRY_HIP(lr_timer_mark(c, a.dir ? LR_EV_REV_FILTER_BEGIN : LR_EV_FWD_FILTER_BEGIN));
    const int only = lr_nn16_form_hint(c, a.dir ? 0 : 1);      // (the columns of the reverse pass are cloud 0)
    int32_t *miss = ws->counters + (a.dir ? LR_CNT_FORM_MISS_R : LR_CNT_FORM_MISS_F);
    unsigned long long *clk = ws->clock_probe ? ws->clk_dev : (unsigned long long *)nullptr;
    const lr_pb_tail tl = { clk };
    const lr_pb_grid pg = { a.row_blocks, a.strips, total, a.dir, only };
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, c.st, tl, clk, a.Hq, a.na, a.rowmap, a.na_dev, a.Hc, a.nC, a.nb, a.tps, a.tau, ws->cand_cnt, ws->cand,
                           a.colmap, a.tile_min, a.row_bound, a.rev_offs, a.rev_range, a.yfin, a.yfin_stride, a.yshare, miss, a.thr, pg, c.z);
    };
    if (only != 2) launch(nn16_passb_kernel<true>);
    if (only != 1) launch(nn16_passb_kernel<false>);
    return lr_timer_mark(c, a.dir ? LR_EV_REV_FILTER_END : LR_EV_FWD_FILTER_END);
}
