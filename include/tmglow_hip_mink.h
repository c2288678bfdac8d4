/* Excursion-set morphology of the ensemble (tmg_mink.hip): the raw counts from which the host forms the three Minkowski functionals
 * of the 2-D excursion sets of a field as the level moves: area, boundary length and Euler characteristic (the "genus curve").
 * Integer compares, min, max and adds only (int32 inside a block, then one 64-bit integer global atomic per non-zero entry and
 * block): integer sums do not depend on their order, so every output is bitwise reproducible, independent of the chunking and of
 * the member group, and equal to an int64 reference.  A header of its own: tmglow_hip.h (which defines tmg_stream_t) does not
 * include it.
 *
 * THE DEFINITIONS.  A field f (1 <= F <= 4) is one of the C channels, fields[f], all distinct.  Per case b and field f the ladder
 * is thr[(b * F + f) * J + j], j = 0 .. J - 1, 1 <= J <= 32: raw normalised device floats, non-decreasing as the callers build them.
 * The rank of a pixel is r = #{j : x > thr_j}, strict compares: NaN and -Inf have rank 0, +Inf has rank J (against finite
 * thresholds), and a NaN threshold is above no value.  The excursion set of level j is E_j = {r > j}; for a non-decreasing ladder
 * that is {x > thr_j}, and for any other ladder the tables are those of {r > j} (the rank does not depend on the ladder's order:
 * the tables are those of the sorted ladder).  The rows are R = S + 1: the S members, then the target as row S.  Per row, case,
 * field and level j five counts over the H x W field, of in-field pixels, pairs and quads only (nothing outside the field is in
 * a set, and a pair or quad that leaves the field is not counted):
 *   N   pixels in E_j                                     Nh  horizontally adjacent pairs with both pixels in
 *   Nv  vertically adjacent pairs with both pixels in     Nq  2 x 2 quads with all four pixels in
 *   Nd  2 x 2 quads with exactly two pixels in, on a diagonal
 * From these the host forms edges = 4 N - 2 Nh - 2 Nv (exposed unit edges, the field's border included), chi4 = N - Nh - Nv + Nq
 * (4-connected pieces minus their 8-connected holes) and chi8 = chi4 - Nd (8-connected pieces minus 4-connected holes).
 *
 * THE LAYOUT, of one kept step.
 *   table [B][F][R][J][5] int64   (N, Nh, Nv, Nq, Nd) per case, field, row and level
 * The chunk call with m0 = 0 zeroes the whole table with a launch of its own before anything is added: no memset.
 *
 * THE KERNEL'S SHAPE.  The counts come from ranks, at a cost per pixel that does not depend on J.  With a, b, c, d the ranks of a
 * quad's pixels (a the upper left, b its right neighbour, c the one below, d the diagonal one): the pixel is in E_j for j < a,
 * the pairs for j < min(a, b) and j < min(a, c), the quad for j < min(a, b, c, d); the quad is a diagonal pair of E_j for
 * max(b, c) <= j < min(a, d) or max(a, d) <= j < min(b, c), of which at most one is not empty.  So a block keeps, per row and
 * field, four histograms over 0 .. J of a, min(a, b), min(a, c) and min(a, b, c, d), whose sums over the bins above j are N, Nh,
 * Nv, Nq, and a fifth that takes +1 at the lower and -1 at the upper end of the diagonal interval, whose sum over the bins up to
 * j is Nd.  A pixel outside the field has rank 0: bin 0 is never read, and no quad that leaves the field is a diagonal pair, as
 * two of its pixels on a side have rank 0.
 * One block of 256 threads per tile of 64 rows x 63 columns of one case and one group of group(k) members (or the target: one more
 * block row in the call with m0 = 0), all F fields.  Wave w owns the rows 16 w .. 16 w + 15 of the tile and loads 17, the last being
 * the halo row that the next wave or tile owns; lane l < 63 owns column l and lane 63 is the halo column that the next tile owns, so
 * every pixel, pair and quad is counted by exactly one lane of one tile.  A load is 64 consecutive pixels of a row.  The rank is a
 * binary search (6 reads) in the block's copy of the ladder, sorted in LDS; the right neighbour's rank is a lane exchange, the
 * lower one's the lane's next register.  A lane walks down its column and keeps the four bins of the four histograms, packed into
 * one key, and a run count in registers, adding to LDS (int32 atomics) only when the key changes, and at the end of its 16 rows,
 * where a wave whose lanes all hold one key adds once: smooth fields add rarely.  The diagonal histogram is added to directly:
 * diagonal pairs are rare where fields are smooth, and spread over the bins where they are not.  A bin holds at most 64 * 63 = 4032
 * < 2^31 per row and field: int32 inside a block, 64-bit from the global atomic on.  Lanes whose pixels lie outside the field
 * (their addresses clamped into it, their rank 0) stay for every exchange and barrier. */
#ifndef TMGLOW_HIP_MINK_H
#define TMGLOW_HIP_MINK_H

#include "tmglow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmg_ens_mink_plan launches nothing: the launch plan of tmg_ens_mink_chunk for dims = {S, B, H, W, F, J}, which the launch body
 * itself calls.  out (12 host integers) = {tile_h, tile_w, tiles_x, tiles_y, grid_x, grid_y, grid_z, blocks, threads, group,
 * lds_bytes, table_words}:
 *   tile_h, tile_w           = 64, 63; tiles_x, tiles_y = ceil(W / 63), ceil(H / 64)
 *   group                    = group(S), where group(k), the members one block takes of a chunk of k, is min(k, G) with G the
 *                            larger of 4, 2 for which tiles_x tiles_y B ceil(k / G) >= 1024, else 1: a block sorts the ladders
 *                            and sums the histograms once for its members, but takes them one after the other, and the kernel is
 *                            bound by the length of a block's work: many short blocks fill the chip.  The counts do not depend on
 *                            it.
 *   grid_x, grid_y, grid_z   = tiles_x tiles_y, ceil(S / group) + 1, B: the grid of the call with k = S, m0 = 0 (the last block row
 *                            is the target's; a call with m0 > 0 has none); blocks = their product, of threads = 256
 *   lds_bytes                the (static) LDS of the kernel
 *   table_words              = B F (S + 1) J 5 64-bit words
 * S, B, H, W >= 1, 1 <= F <= 4, 1 <= J <= 32, else -1; S > 1024, B > 65535, H W >= 2^31 - 256: -2; a null pointer: -3. */
int tmg_ens_mink_plan(const int64_t* dims, int64_t* out);

/* tmg_ens_mink_chunk handles one chunk of k whole members: y holds the chunk's rows, [k][B][HW] pixels of C fp32 channels, pixel
 * stride y_d[0], channel offset y_d[1] (tmg_ens_iscale_chunk's rule: channel slices of wider buffers work), read straight from the
 * NHWC rows; target: [B][HW] pixels of C channels, pixel stride t_d[0], channel offset t_d[1]; thr [B][F][J] device floats; fields:
 * F host integers, distinct channels.  It adds the counts of the members m0 .. m0 + k - 1 into their rows of table.  The call with
 * m0 = 0 first zeroes the whole table and also adds the target's row S.  The rows are independent: there is no step call.
 * dims = {k, B, H, W, C, S, m0, F, J}.  The plan's limits, 2 <= C <= 4, k >= 1, 0 <= m0, m0 + k <= S, every field in 0 .. C - 1 and
 * no field twice, y_d[0] >= y_d[1] + C, y_d[1] >= 0 (t_d alike), else -1; the plan's -2, and y or target beyond the index ranges:
 * -2; a null pointer: -3.  Every code comes before any launch. */
int tmg_ens_mink_chunk(const void* y, const int64_t* y_d, const void* target, const int64_t* t_d, const void* thr, const int64_t* fields,
                       void* table, const int64_t* dims, tmg_stream_t st);

#ifdef __cplusplus
}
#endif

#endif
