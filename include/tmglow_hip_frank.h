/* Multivariate rank histograms of the ensemble members against the target (tmg_frank.hip): the pre-ranks of the average-rank and
 * band-depth histograms (Thorarinsdottir, Scheuerer & Heinz 2016; modified band depth of Lopez-Pintado & Romo 2009).  Comparisons
 * and integer sums only, no atomics: every output is bitwise reproducible, independent of the chunking, and equal to an int64
 * reference.  A header of its own: tmglow_hip.h (which defines tmg_stream_t) does not include it.
 *
 * THE DEFINITIONS.  Rows x_0 .. x_{S-1} are the members and x_S is the target, raw normalised fp32, in the planar buffer
 * xs [S + 1][B][C][HW] that tmg_ens_score_store fills (the target as a one-member chunk into row S).  Per case b, channel c, pixel
 * p and row i, over the S other rows j != i:
 *   lt = #{j : x_j < x_i}, eq = #{j : x_j == x_i}, gt = S - lt - eq
 *   A  = 2 lt + eq                                  the average-rank term: twice the mid-rank minus a constant
 *   D  = C(S,2) - C(lt,2) - C(gt,2)                 the band-depth term: the pairs of other rows whose closed band [min, max] holds
 *                                                   x_i; lt gt without ties; C(n,2) = n (n - 1) / 2, so S = 1 gives 0
 *   O  = [lt == S or gt == S], target row only      the target lies strictly outside the members' range
 * Non-finite rows are not supported: the outputs of a pixel that holds one are unspecified; no access leaves the buffers and the
 * other pixels are unaffected. */
#ifndef TMGLOW_HIP_FRANK_H
#define TMGLOW_HIP_FRANK_H

#include "tmglow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmg_ens_frank_plan launches nothing: the launch plan of tmg_ens_frank_step for dims = {S, B, C, HW}, which the launch body itself
 * calls.  out (7 host integers) = {nblk, grid_x, grid_y, grid_z, threads, rec_words, ws_words}:
 *   nblk        = ceil(HW / 256) pixel blocks; the grid is (nblk, C, B) blocks of threads = 256, one thread per pixel
 *   rec_words   = 2 (S + 1) + 1 int32 words per block: the sums of (A, D) of rows 0 .. S over the block's pixels, then the sum of O
 *   ws_words    = B C nblk rec_words: the workspace ws [B][C][nblk][rec_words] in 32-bit words
 * S, B, HW >= 1, 2 <= C <= 4, else -1; S > 1024, B > 65535 or sizes beyond the index ranges: -2; a null pointer: -3. */
int tmg_ens_frank_plan(const int64_t* dims, int64_t* out);

/* tmg_ens_frank_step runs once per kept step, after the step's S members and the target are stored in xs.  Two launches: the pixel
 * blocks write their records into ws (int32: per pixel A <= 2048 and D <= 523 776, 256 pixels stay under 2^31); then per (b, c) the
 * records are summed over the blocks in block order as int64 into
 *   pre_raw [B][Tk][C][S + 1][2] int64 at step t: sum_p A_i(p) and sum_p D_i(p), the target last
 *   outside [B][Tk][C] int64 at step t: sum_p O(p)
 * flags & 1: the step goes into tout [B][C][HW] int32, O(p) summed over such steps; it holds t_before of them (t_before = 0: it is
 * written, not read, so it needs no memset).  Without the flag tout is not touched.
 * dims = {S, B, HW, C, Tk, t, t_before, flags}.  The plan's limits, Tk >= 1, 0 <= t < Tk, t_before >= 0, else -1; sizes beyond the
 * index ranges or S > 1024: -2; a null pointer among xs, ws, pre_raw, outside, and tout with flags & 1: -3; ws_words under the
 * plan's: -1.  Every code comes before any launch. */
int tmg_ens_frank_step(const void* xs, void* ws, int64_t ws_words, void* pre_raw, void* outside, void* tout, const int64_t* dims,
                       tmg_stream_t st);

#ifdef __cplusplus
}
#endif

#endif
