/* Event durations of the ensemble members and of the target (tmg_spell.hip): spells, gaps and their censored ends along the time
 * window, per-pixel persistence maps.  A streaming state machine: one 32-bit word of state per (row, case, event, pixel) is carried
 * from step to step.  Comparisons and integer adds only (LDS int32 atomics, then one 64-bit integer global atomic per non-empty
 * entry): integer sums do not depend on their order, so every output is bitwise reproducible, independent of the chunking, and equal
 * to an int64 reference.  A header of its own: tmglow_hip.h (which defines tmg_stream_t) does not include it.
 *
 * THE DEFINITIONS.  An event k (1 <= K <= 4) is (channel ev[2k], direction ev[2k + 1]: 1 for x > thr, 0 for x < thr, both strict)
 * with the raw threshold thr[b * K + k] (device floats), as in tmglow_hip_event.h.  A value that compares false is in no event: NaN
 * in either direction, +-Inf on the side it cannot be on.  Rows 0 .. S - 1 are the members, row S is the target.  The window is the
 * Tn >= 2 steps t = 0 .. Tn - 1 in the order they are fed.  Per row r, case b, event k and pixel p, e_t in {0, 1} is the event
 * indicator at step t.  A run is a maximal stretch of equal e_t, of polarity 1 (a spell) or 0 (a gap), of length l >= 1 and of class
 *   complete  it starts after step 0 and ends before step Tn - 1
 *   left      it contains step 0 and not step Tn - 1          right   it contains step Tn - 1 and not step 0
 *   both      it covers the whole window
 * Only complete runs enter the length histogram: bin j - 1 holds those of length j for j < L, bin L - 1 those of length >= L
 * (1 <= L <= 64).
 *
 * THE LAYOUTS.
 *   state [S + 1][B][K][HW] uint32   bits 0..14 the current run's length, bit 15 its polarity, bits 16..30 the row's longest
 *                                    polarity-1 run so far, bit 31 "the current run contains step 0".  Step 0 writes it and does
 *                                    not read it: no memset.  Tn <= 32767 keeps both lengths in their 15 bits.
 *   table [B][K][S + 1][2][L + 7] int64, per (case, event, row, polarity), pooled over the pixels:
 *                                    [0 .. L) the histogram of the complete runs, [L] the sum of their lengths, [L + 1 .. L + 4) the
 *                                    numbers of left, right and both runs, [L + 4 .. L + 7) the sums of their lengths.  The step
 *                                    call of step 0 with row0 = 0 zeroes it before its own launch: no memset.
 *   maps [7][B][K][HW] int32         0 sum over members and steps of e_t, 1 sum over members of the number of polarity-1 runs of
 *                                    any class, 2 / 3 the sum / the maximum over the members of each member's longest polarity-1 run
 *                                    of any class (0 without one), 4, 5, 6 the target's e_t sum, number of polarity-1 runs and longest
 *                                    one.  Planes 0, 1 (4, 5) are written by the members' first chunk (the target's call) of step 0 and
 *                                    added to afterwards; planes 2, 3, 6 are written by tmg_ens_spell_finalize.  S Tn < 2^31. */
#ifndef TMGLOW_HIP_SPELL_H
#define TMGLOW_HIP_SPELL_H

#include "tmglow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmg_ens_spell_plan launches nothing: the launch plan of tmg_ens_spell_step and tmg_ens_spell_finalize for dims = {S, B, HW, K, L,
 * Tn}, which the launch bodies themselves call.  out (10 host integers) = {blocks, threads, group, lds_bytes, state_words, grid_x,
 * grid_y, row_words, table_words, fin_lds_bytes}:
 *   grid_x, grid_y  = ceil(HW / 256), B; blocks = grid_x grid_y blocks of threads = 256, one thread per pixel of one case
 *   group           = G: the rows of a chunk are taken G at a time; the block's LDS table holds the ended runs of one group,
 *                     [G][K][2][L + 3] int32 (histogram, length sum, left count, left length sum), lds_bytes of it; G is the
 *                     largest count in 1..8 whose table stays within 16 KiB
 *   state_words     = (S + 1) B K HW 32-bit words of state
 *   row_words       = L + 7; table_words = B K (S + 1) 2 row_words 64-bit words
 *   fin_lds_bytes   = the LDS of the finalize kernel, [G][K][2][4] int32 (right count, right length sum, both count, both sum)
 * S, B, HW >= 1, 1 <= K <= 4, 1 <= L <= 64, Tn >= 2, else -1; S > 1024, B > 65535, Tn > 32767, S Tn >= 2^31, HW >= 2^31 - 256 or
 * state_words >= 2^40: -2; a null pointer: -3. */
int tmg_ens_spell_plan(const int64_t* dims, int64_t* out);

/* tmg_ens_spell_step advances the state machine of one chunk of k whole rows by window step t: y holds the chunk's rows, [k][B][HW]
 * pixels of C fp32 channels, pixel stride y_d[0], channel offset y_d[1] (tmg_ens_event_count's rule: channel slices of wider buffers
 * work), read straight from the NHWC rows.  The members come as chunks with row0 + k <= S; the same entry is called once more per
 * step with the target as a one-row chunk, k = 1 and row0 = S.  Every row is fed every step exactly once, steps in order.  A run that
 * ends at this step is counted as complete or left into table; maps planes 0, 1 (row0 < S) or 4, 5 (row0 = S) advance.
 * dims = {k, B, HW, C, S, row0, K, L, Tn, t}.  The plan's limits, 2 <= C <= 4, k >= 1, 0 <= row0, row0 + k <= S or (row0 = S and
 * k = 1), 0 <= t < Tn, every channel in 0 .. C - 1, every direction 0 or 1, y_d[0] >= y_d[1] + C, y_d[1] >= 0, else -1; the plan's
 * -2, and y beyond the index ranges: -2; a null pointer: -3.  Every code comes before any launch. */
int tmg_ens_spell_step(const void* y, const int64_t* y_d, const void* thr, const int64_t* ev, void* state, void* table, void* maps,
                       const int64_t* dims, tmg_stream_t st);

/* tmg_ens_spell_finalize is called once, after step Tn - 1 of every row: the run of every (row, case, event, pixel) that is still
 * open is counted as right or, when it contains step 0, as both into table, and every row's longest polarity-1 run is folded over
 * the members into maps planes 2 (sum) and 3 (maximum) and, for the target, plane 6.
 * dims = {S, B, HW, K, L, Tn}: the plan's codes; a null pointer: -3.  Every code comes before any launch. */
int tmg_ens_spell_finalize(const void* state, void* table, void* maps, const int64_t* dims, tmg_stream_t st);

#ifdef __cplusplus
}
#endif

#endif
