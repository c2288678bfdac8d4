/* Distance-map verification of the ensemble (tmg_edt.hip): how far a member's event set lies from the target's.  The exact Euclidean
 * distance transform of a binary field on the device, and the integer sums from which the host forms the mean error distance, the
 * directed, symmetric and partial (quantile) Hausdorff distances and Baddeley's delta (Baddeley 1992; Dubuisson & Jain 1994;
 * Gilleland 2011).  Squared pixel distances are integers and distances are held in fixed point, so only integer adds, mins, maxes
 * and atomics touch an output: every output is bitwise reproducible, independent of the chunking and of the run, and equal to an
 * int64 reference.  A header of its own: tmglow_hip.h (which defines tmg_stream_t) does not include it.
 *
 * THE DEFINITIONS.  An event e (1 <= K <= 4) is (channel, direction): x > thr[b][e] for direction 1, x < thr[b][e] for 0, strict,
 * on raw normalised device floats; a value that compares false (NaN, an infinity on the wrong side) is in no event.  The rows are
 * the S members, then the target.  A is a member's event set and O the target's, subsets of the H x W pixels; nothing outside the
 * field is in a set (the domain is not periodic).
 *   d2_A(p) = min over q in A of (drow^2 + dcol^2), an integer in pixel units, exact over the whole field and never truncated;
 *             INF = 2^30 when A is empty.
 *   c       the cutoff, an integer in 1 .. 255.
 *   w_A(p)  = 256 c if d2_A(p) >= c^2, else isqrt(65536 d2_A(p)): floor(256 d), the distance in 1/256 pixel, below 2^16.  The integer
 *             square root is exact: a float estimate is corrected by integer compares until r^2 <= n < (r + 1)^2.
 *
 * THE LAYOUT, of one kept step.
 *   pair [B][K][S][11] int64   nA, nO, nAO: pixels in A, in O, in both
 *                              sOA1, sOA2: the sums over p in O of w_A and of w_A^2 (the misses: how far observed event pixels are
 *                              from the forecast); sAO1, sAO2: over p in A of w_O and w_O^2 (the false alarms)
 *                              sD1, sD2: over all pixels of |w_A - w_O| and of (w_A - w_O)^2
 *                              hOA = max over p in O of d2_A(p), uncut: -1 when O is empty, INF when A is empty and O is not;
 *                              hAO alike with A and O swapped
 *   hist [B][K][S][2][c + 1] int64   over p in O the count by min(floor(sqrt(d2_A)), c); over p in A likewise of d2_O
 *   msum [B][K][HW] int32      the sum over the members fed so far of w_A(p)
 *   dmap [B][K][HW] int32      d2_O(p), the target's map, written by the call with m0 = 0
 *   count [B][K][S + 1] int32  the set sizes of the rows; a row whose count is 0 is not searched
 *   scratch [S + 1][B][K][H][ceil(W / 64)] 64-bit words of the indicators, bit l of word j is column 64 j + l
 * and over the steps folded by tmg_ens_edt_step:
 *   tmem, ttgt [B][K][HW] int64   the sums over the steps of msum and of w_O
 * The chunk call with m0 = 0 presets pair (0, the two maxima -1), hist, count and msum with a launch of its own: no memset.
 *
 * THE KERNELS' SHAPE.  The mask kernel reads the chunk's NHWC rows once for all K events, one wave per 64 consecutive pixels of an
 * image row: the compare's lane mask is one word of the indicator.  The distance kernel is separable: g(i', j), the distance along
 * row i' from column j to the nearest set pixel of that row (32768 when the row has none: its square is INF), comes from the row's
 * words by count-leading / count-trailing-zero operations, and d2(i, j) = min over i' of (i - i')^2 + g(i', j)^2.  One block of 256
 * threads owns a band of 64 rows of a strip of 64 columns of one (row, case, event), 16 pixels per thread in registers; the source
 * rows come tile by tile (the tile's words by one coalesced load into LDS, then 64 rows of g as uint16 in LDS), the band's own
 * tile first, then the tiles above and below at growing distance dt, until no pixel of the block has
 * best > (64 (dt - 1) + 1)^2; inside a tile a pixel walks away from its own row and stops at di^2 >= best.  The target's d2_O goes to dmap in a launch of its own before the members'; a member's d2_A stays in
 * registers and is combined with d2_O into the eleven sums (int32 / int64 per thread, LDS per block, one 64-bit integer atomic per
 * non-zero entry), the histograms (int32 in LDS, 64-bit atomics) and an int32 atomic add of w_A into msum.  The histogram bin is
 * w >> 8, which equals min(floor(sqrt(d2)), c) for every d2, as floor(floor(256 x) / 256) = floor(x). */
#ifndef TMGLOW_HIP_EDT_H
#define TMGLOW_HIP_EDT_H

#include "tmglow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmg_ens_edt_plan launches nothing: the launch plan of tmg_ens_edt_chunk for dims = {S, B, H, W, K, c}, which the launch body
 * itself calls.  out (16 host integers) = {tile_w, band, strips, bands, grid_x, grid_y, grid_z, blocks, threads, lds_bytes,
 * mask_grid_x, scratch_words, pair_words, hist_words, count_words, map_words}:
 *   tile_w, band             = 64, 64: a block's strip of columns and band of rows, also the rows of a source tile
 *   strips, bands            = ceil(W / 64), ceil(H / 64)
 *   grid_x, grid_y, grid_z   = strips bands K, S, B: the members' distance grid of the call with k = S (the target's has grid_y = 1);
 *                            blocks = their product, of threads = 256
 *   lds_bytes                the LDS of the distance kernel: its static tables (10320 bytes) and the source tile's indicator words,
 *                            8 * 64 * strips bytes (dynamic): at most 43088
 *   mask_grid_x              = ceil(H strips / 4): the mask kernel's blocks per row and case, four waves each
 *   scratch_words            = (S + 1) B K H strips 64-bit words; pair_words = 11 B K S and hist_words = 2 (c + 1) B K S 64-bit
 *                            words; count_words = B K (S + 1) and map_words = B K H W 32-bit words (msum and dmap each)
 * S, B, H, W >= 1, 1 <= K <= 4, 1 <= c <= 255, else -1; S > 1024, B > 65535, H or W > 4096, H W >= 2^31 - 256: -2; a null
 * pointer: -3. */
int tmg_ens_edt_plan(const int64_t* dims, int64_t* out);

/* tmg_ens_edt_chunk handles one chunk of k whole members: y holds the chunk's rows, [k][B][HW] pixels of C fp32 channels, pixel
 * stride y_d[0], channel offset y_d[1] (tmg_ens_iscale_chunk's rule: channel slices of wider buffers work); target: [B][HW] pixels
 * of C channels, pixel stride t_d[0], channel offset t_d[1]; thr [B][K] device floats; ev: K x (channel, direction) host integers.
 * It writes the indicator words of the members m0 .. m0 + k - 1 and adds their sums into pair, hist and msum.  The call with m0 = 0
 * first presets pair, hist, count and msum, and forms the target's words and dmap.  dims = {k, B, H, W, C, S, m0, K, c}.
 * The plan's limits, 2 <= C <= 4, k >= 1, 0 <= m0, m0 + k <= S, every channel in 0 .. C - 1, every direction 0 or 1,
 * y_d[0] >= y_d[1] + C, y_d[1] >= 0 (t_d alike), else -1; the plan's -2, and y, target or the maps beyond the index ranges: -2; a
 * null pointer: -3.  Every code comes before any launch. */
int tmg_ens_edt_chunk(const void* y, const int64_t* y_d, const void* target, const int64_t* t_d, const void* thr, const int64_t* ev,
                      void* scratch, void* count, void* dmap, void* msum, void* pair, void* hist, const int64_t* dims, tmg_stream_t st);

/* tmg_ens_edt_step, once per step that counts for the time maps, after its last chunk: tmem += msum, ttgt += w_O (from dmap).
 * dims = {B, H, W, K, c}, the plan's limits and codes; a null pointer: -3.  Every code comes before the launch. */
int tmg_ens_edt_step(const void* msum, const void* dmap, void* tmem, void* ttgt, const int64_t* dims, tmg_stream_t st);

/* tmg_ens_edt_fixed is the host's statement of the kernels' w: out[i] = w(d2[i]) for n host integers 0 <= d2[i] <= 2^30 and the
 * cutoff c, through the same float estimate and integer fix-up.  n < 0, c outside 1 .. 255 or a d2 outside its range: -1; a null
 * pointer: -3.  It touches no device. */
int tmg_ens_edt_fixed(const int64_t* d2, int64_t n, int64_t c, int64_t* out);

#ifdef __cplusplus
}
#endif

#endif
