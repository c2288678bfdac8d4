/* Phase averages of the ensemble members and of the target on the shedding phase (tmg_phase.hip: every row is labelled with the sector
 * of the angle of its two coefficients on a pair of the target's POD modes, then added to the accumulators of its sector; no
 * transcendental, no atomics, no LDS, no workspace: bitwise reproducible for every chunking).  Included by tmglow_hip.h (which defines
 * tmg_stream_t): do not include it on its own. */
#ifndef TMGLOW_HIP_PHASE_H
#define TMGLOW_HIP_PHASE_H

/* tmg_ens_phase_plan launches nothing: the launch plan of tmg_ens_phase_accum for dims = {S, B, C, HW, NB}, which the launch body
 * itself calls.  plan (6 host integers) = {TILE, NT, NB, B, ws, vec}:
 *   TILE  pixels of one block (256 threads): 1024 on the vector path (4 consecutive pixels per thread), 256 on the scalar path
 *   NT    = ceil(HW / TILE) pixel tiles; the grid is NT x NB x B blocks, one per (pixel tile, sector, case); tile i covers the pixels
 *         [i TILE, min(HW, (i + 1) TILE)), every pixel exactly once
 *   ws    workspace floats: always 0
 *   vec   1: the vector path, 16-byte loads and stores, which a call takes when HW % 4 == 0 AND its rows are dense (pixel stride == C,
 *         channel offset 0) AND the bases of the rows, of m and of acc are 16-byte aligned; the plan assumes dense aligned rows, so
 *         vec = (HW % 4 == 0), and a call whose rows are a channel slice or whose bases are not aligned takes the scalar path (TILE 256)
 * S, B, HW >= 1, 2 <= C <= 4, NB one of 4, 8, 16, 32, else -1; NB > 32, S > 1024, B > 65535 or sizes beyond the index ranges: -2; a
 * null pointer: -3. */
int tmg_ens_phase_plan(const int64_t* dims, int64_t* plan);

/* tmg_ens_phase_label: one int32 label per row (s, b) of k B rows, s < k members (or k = 1: the target), b < B cases.  The row's two
 * raw coefficient sums are read at coef + b c_d[0] + s c_d[1] + pair[0] and + pair[1] (element strides of the caller's coef_raw view
 * that starts at member m0 and step t; pair: two distinct mode indices, host integers), the label is written at
 * lab + b l_d[0] + s l_d[1].  g [B][2] (device fp32): the factors 1 / (HW sqrt(lam)) of the pair.  tab (8 HOST floats): tab[0] = thr,
 * the gate, finite and >= 0; tab[1 .. NB / 4 - 1] the tangents tan(2 pi q / NB), q = 1 .. NB / 4 - 1, finite, positive, increasing.
 *   x = fl(g[b][0] raw_i), y = fl(g[b][1] raw_j); label -1 when fl(fl(x x) + fl(y y)) < thr; else the sector 0 .. NB - 1 of the angle
 *   of (x, y) from the positive x axis towards positive y: the quadrant from the signs (x > 0, y >= 0: 0; x <= 0, y > 0: 1; x < 0,
 *   y <= 0: 2; x >= 0, y < 0: 3), inside it the count of the q with fl(t_q |x|) <= |y| (quadrants 0 and 2) or fl(t_q |y|) <= |x|
 *   (quadrants 1 and 3).  A point exactly on an edge belongs to the higher sector; (0, 0) that passes the gate (thr = 0) is sector 0.
 * Every operation is rounded on its own.  dims = {k, B, NB}.  Codes as tmg_ens_phase_plan; strides >= 0, a valid pair and table, else -1. */
int tmg_ens_phase_label(const void* coef, const int64_t* c_d, const int64_t* pair, const void* g, const float* tab, void* lab,
                        const int64_t* l_d, const int64_t* dims, tmg_stream_t st);

/* tmg_ens_phase_accum: rows [k B][HW] pixels of C fp32 channels, pixel stride t_d[0], channel offset t_d[1] (raw normalised values;
 * row s B + b is member s of case b), labels at lab + b l_d[0] + s l_d[1] as tmg_ens_phase_label wrote them.  Device tables:
 * a [B][C] the scales, m [B][C][HW] the target's time mean (normalised).  acc [B][NB][Q][HW] fp32, Q = 2 C + 1: for every row with
 * label n >= 0, in member order, with d_c = fl(a_c fl(x_c - m_c)),
 *   acc[b][n][c] += d_c,  acc[b][n][C + c] += fl(d_c d_c)  (c < C),  acc[b][n][2 C] += fl(d_0 d_1)        fp32, no contraction
 * The running value is loaded before the first add and stored once: the additions into one element run steps in order, members in
 * order for every chunking.  A sector without a row of the chunk is neither read nor written; a row with label -1 is not read.
 * dims = {k, B, HW, C, NB}.  Codes as tmg_ens_phase_plan, and t_d[0] >= t_d[1] + C, t_d[1] >= 0, strides >= 0, else -1. */
int tmg_ens_phase_accum(const void* rows, const int64_t* t_d, const void* lab, const int64_t* l_d, const void* a, const void* m, void* acc,
                        const int64_t* dims, tmg_stream_t st);

#endif
